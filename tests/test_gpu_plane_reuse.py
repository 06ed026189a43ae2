"""Reuse of the all-steps text plane across sample() calls: runs on the MI355X only (-m gpu).

A sample() call whose prompts and styles hold the same bits as the previous call's, at the same shape and schedule and with
unchanged weights, skips the text side and reads the plane the earlier call left in the handle.  Every comparison is
torch.equal, no tolerance, and the reference always comes from a FRESH handle created with DHW_PLANE_REUSE=0 (every call of
such a handle evaluates the text side), never from the handle under test.  `last` is the device flag of the most recent call
(model.plane_reuse()): 1 = the text-side kernels returned at once.

Shapes: bf16, 2 layers, synthetic weights and inputs; B = 3 (odd: one (step, prompt) pair per workgroup of the layer kernel)
and B = 4 (even), L = 40, Lt = 9, T = 4 — the smallest that still run the fused text-side kernels and a real plane."""
import os

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec

pytestmark = pytest.mark.gpu

L, LT, T = 40, 9, 4
PERTURBED = "text_style_model.text_ffn.3.bias"   # a text-side weight: a plane of the old weights gives other samples
_INPUTS, _REFS = {}, {}


def _weights(perturbed=False):
    sd = {k: torch.from_numpy(v.copy()) for k, v in spec.synthetic_state_dict(2).items()}
    if perturbed:
        sd[PERTURBED] += 0.25
    return sd


def _model(env=None, perturbed=False):
    """A model whose handle exists (the switches are read at dhw_create, which the first device call runs)."""
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=4, max_L=48, max_Lt=LT).eval()
    m.load_state_dict(_weights(perturbed), strict=True)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        m._ensure_handle(torch.device("cuda", torch.cuda.current_device()), 4, 48, LT, 14)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return m


def _inputs(which, B=3):
    """(text, style) on the device, fresh tensors every time.  'A' / 'B': two sets of prompts and styles; 'A_tok': A with one
    token changed; 'A_z' / 'A_nz' / 'A_ulp': A with style[1, 3, 7] = 0.0 / -0.0 / the next float after A's value."""
    if not _INPUTS:
        _INPUTS["A"] = spec.synthetic_inputs(4, L, LT, seed=31, pad=1, T=1)
        _INPUTS["B"] = spec.synthetic_inputs(4, L, LT, seed=32, pad=2, T=1)
    src = _INPUTS["B" if which == "B" else "A"]
    text, style = src["text"][:B].copy(), src["style"][:B].copy()
    if which == "A_tok":
        text[0, 2] = text[0, 2] % 72 + 1
    if which == "A_z":
        style[1, 3, 7] = 0.0
    if which == "A_nz":
        style[1, 3, 7] = -0.0
    if which == "A_ulp":
        style[1, 3, 7] = np.nextafter(style[1, 3, 7], np.float32(np.inf))
    return torch.from_numpy(text).cuda(), torch.from_numpy(style).cuda()


def _sample(m, text, style, seed=5, T_=T, **kw):
    return dhg_amd.sample(m, text, style, L=L, T=T_, seed=seed, **kw).cpu()


def _ref(which, B=3, seed=5, T_=T, perturbed=False):
    """The first call of a fresh handle created with DHW_PLANE_REUSE=0; computed once, shared, never changed."""
    key = (which, B, seed, T_, perturbed)
    if key not in _REFS:
        m = _model({"DHW_PLANE_REUSE": "0"}, perturbed)
        out = _sample(m, *_inputs(which, B), seed=seed, T_=T_)
        assert m.plane_reuse() == (0, 1, 0) and torch.isfinite(out).all()
        _REFS[key] = out
    return _REFS[key]


def _last(m):
    return m.plane_reuse()[0]


@pytest.mark.parametrize("B", [3, 4])
def test_same_inputs_reuse_the_plane_and_a_new_seed_does_too(B):
    m = _model()
    text, style = _inputs("A", B)
    first = _sample(m, text, style)
    assert _last(m) == 0
    second = _sample(m, text, style)
    assert _last(m) == 1
    assert torch.equal(first, _ref("A", B)) and torch.equal(second, first)
    other_seed = _sample(m, text, style, seed=6)
    assert m.plane_reuse() == (1, 3, 2)
    assert torch.equal(other_seed, _ref("A", B, seed=6)) and not torch.equal(other_seed, first)
    # equal CONTENT in other tensors is reused as well: the compare reads bits, not pointers
    again = _sample(m, *_inputs("A", B))
    assert _last(m) == 1 and torch.equal(again, first)


def test_the_switch_turns_reuse_off():
    m = _model({"DHW_PLANE_REUSE": "0"})
    text, style = _inputs("A")
    for _ in range(2):
        assert torch.equal(_sample(m, text, style), _ref("A")) and _last(m) == 0


def test_one_token_changed_in_place_is_seen():
    m = _model()
    text, style = _inputs("A")
    _sample(m, text, style)
    ptr = text.data_ptr()
    text[0, 2] = text[0, 2] % 72 + 1
    assert text.data_ptr() == ptr
    out = _sample(m, text, style)
    assert _last(m) == 0 and torch.equal(out, _ref("A_tok")) and not torch.equal(out, _ref("A"))


def test_one_style_element_changed_by_one_ulp_or_in_sign_of_zero_is_seen():
    m = _model()
    text, style = _inputs("A")
    _sample(m, text, style)
    style[1, 3, 7] = torch.nextafter(style[1, 3, 7], torch.tensor(float("inf"), device="cuda"))
    out = _sample(m, text, style)
    assert _last(m) == 0 and torch.equal(out, _ref("A_ulp"))
    style[1, 3, 7] = 0.0
    out = _sample(m, text, style)
    assert _last(m) == 0 and torch.equal(out, _ref("A_z"))
    assert torch.equal(_sample(m, text, style), _ref("A_z")) and _last(m) == 1
    style[1, 3, 7] = -0.0                      # equal as a float, other bits
    out = _sample(m, text, style)
    assert _last(m) == 0 and torch.equal(out, _ref("A_nz"))


def test_a_b_a():
    m = _model()
    a, b = _inputs("A"), _inputs("B")
    assert torch.equal(_sample(m, *a), _ref("A"))
    assert torch.equal(_sample(m, *b), _ref("B")) and _last(m) == 0
    assert torch.equal(_sample(m, *a), _ref("A")) and _last(m) == 0
    assert not torch.equal(_ref("A"), _ref("B"))


def _strokes(B=3):
    g = torch.Generator().manual_seed(77)
    s = torch.randn((B, L, 3), generator=g)
    s[..., 2] = (s[..., 2] > 0.5).float()
    return s.cuda()


def _between_score(m, text, style):
    assert torch.isfinite(dhg_amd.score(m, _strokes(), text, style, levels=[1, 2], T=T, seed=9)).all()


def _between_forward(m, text, style):
    tb, sb = _inputs("B")
    eps, _, _ = m(_strokes()[..., :2].contiguous(), tb, torch.tensor([0.9, 0.3, 0.6]).cuda(), sb)
    assert torch.isfinite(eps).all()


def _between_ddim(m, text, style):
    tb, sb = _inputs("B")
    assert torch.isfinite(dhg_amd.sample_ddim(m, tb, sb, L=L, T=T, steps=2, seed=9)).all()


def _between_cond(m, text, style):
    assert torch.isfinite(dhg_amd.sample(m, text, style, L=L, T=T, seed=9, known=_strokes(), t_start=2)).all()


def _between_attention(m, text, style):
    tb, sb = _inputs("B")
    mean, _ = dhg_amd.attention(m, _strokes()[..., :2].contiguous(), tb, torch.tensor([0.9, 0.3, 0.6]).cuda(), sb, layer=-1)
    assert torch.isfinite(mean).all()


def _between_ragged(m, text, style):
    tb, sb = _inputs("B")
    assert torch.isfinite(dhg_amd.sample(m, tb, sb, L=L, T=T, seed=9, lengths=[8, 40, 24])).all()


def _between_other_T(m, text, style):
    assert torch.isfinite(_sample(m, text, style, T_=5)).all()


def _between_other_B(m, text, style):
    assert torch.isfinite(_sample(m, *_inputs("A", 4))).all()


def _between_set_graph(m, text, style):
    assert _lib.lib().dhw_set_graph(m._handle, 0) == 0


# what runs between two sample(A) calls -> the flag the second one must report, where the code claims one: the eager entries
# write the per-call text buffers of the workspace and never the plane or the staging buffers (1); the others change the tag,
# the staged prompts or a switch (0)
BETWEEN = {
    "score": (_between_score, 1), "forward": (_between_forward, 1), "sample_ddim": (_between_ddim, 1), "attention": (_between_attention, 1),
    "cond_t_start": (_between_cond, 0), "ragged_other_prompts": (_between_ragged, 0), "other_T": (_between_other_T, 0),
    "other_B": (_between_other_B, 0), "set_graph": (_between_set_graph, 0),
}


@pytest.mark.parametrize("name", list(BETWEEN))
def test_sample_after_each_other_entry(name):
    between, last = BETWEEN[name]
    m = _model()
    text, style = _inputs("A")
    assert torch.equal(_sample(m, text, style), _ref("A"))
    between(m, text, style)
    out = _sample(m, text, style)
    assert torch.equal(out, _ref("A")), name
    assert _last(m) == last, name
    assert torch.equal(_sample(m, text, style), _ref("A")) and _last(m) == 1, name   # and the call after it reuses again


def test_weights_reloaded():
    m = _model()
    text, style = _inputs("A")
    assert torch.equal(_sample(m, text, style), _ref("A"))
    m.load_state_dict(_weights(perturbed=True), strict=True)
    out = _sample(m, text, style)
    assert _last(m) == 0 and torch.equal(out, _ref("A", perturbed=True)) and not torch.equal(out, _ref("A"))
    assert torch.equal(_sample(m, text, style), out) and _last(m) == 1


def test_a_schedule_of_two_chunks_never_reuses():
    m = _model()
    text, style = _inputs("A")
    for _ in range(2):
        assert torch.equal(_sample(m, text, style, T_=66), _ref("A", T_=66)) and _last(m) == 0


def test_persistent_step_handle_reuses():
    m = _model({"DHW_PERSIST": "1"})
    text, style = _inputs("A")
    assert torch.equal(_sample(m, text, style), _ref("A")) and _last(m) == 0
    assert torch.equal(_sample(m, text, style), _ref("A")) and _last(m) == 1


def test_profile_rows_of_a_reused_call_report_no_work():
    m = _model()
    text, style = _inputs("A")
    _sample(m, text, style)
    m.profile(True)
    try:
        out = _sample(m, text, style)
        rows = {r["label"]: r for r in m.profile_results()}
    finally:
        m.profile(False)
    assert _last(m) == 1 and torch.equal(out, _ref("A"))
    for label, n in (("ts.fused", 1), ("enc.text_fused", 4)):
        assert rows[label]["launches"] == n and rows[label]["flops"] == 0 and rows[label]["bytes"] == 0, rows[label]
    assert rows["convblock.fused"]["flops"] > 0
    # ... and of a call that evaluates the text side they report it
    m.profile(True)
    try:
        _sample(m, *_inputs("B"))
        rows = {r["label"]: r for r in m.profile_results()}
    finally:
        m.profile(False)
    assert _last(m) == 0 and rows["ts.fused"]["flops"] > 0 and rows["enc.text_fused"]["flops"] > 0
