"""Attention maps on the host side (no GPU needed): the CPU helper the GPU tests use as their yardstick (tests/align_ref.py)
reproduces the oracle's own layer from its probabilities; ``spans`` and ``rewrite_mask`` on hand-made alignments; every
argument of ``attention`` / ``align`` / ``return_attention`` is checked with ValueError before any device is touched; the
C-ABI declares, exports and binds dhw_attention and dhw_attention_shape.

The helper's proof: film(affine1, LN(dense(P V))) + x against the oracle's ``<layer>.x2`` tap, bound 1e-5 on values of order
1 (fp32 throughout; SDPA inside the oracle and the explicit softmax here differ in summation order only).  Measured on the
CPU at B=3, L=136, Lt=7, synthetic_state_dict(2): 1.4e-6, 1.4e-6, 9.5e-7, 1.4e-6 for enc3, enc5, att_layers.0, att_layers.1."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, Lt = 3, 136, 7
LAYERS = align_ref.layer_names(2)
_CACHE = {}


def _sd():
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}


def _case():
    """Inputs and the helper's maps of all four layers, built once and shared."""
    if not _CACHE:
        inp = spec.synthetic_inputs(B, L, Lt, seed=5, T=1)
        text = torch.from_numpy(inp["text"])
        text[1, -2:] = 0
        strokes, style = torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["style"])
        sigma = torch.tensor([0.9, 0.5, 0.2])
        _CACHE.update(text=text, strokes=strokes, style=style, sigma=sigma,
                      maps={n: align_ref.attention(_sd(), strokes, text, sigma, style, n) for n in LAYERS})
    return _CACHE


# ---------------------------------------------------------------- the helper, proven before it is used as a yardstick
@pytest.mark.parametrize("name", LAYERS)
def test_helper_probabilities_reproduce_the_oracles_layer(name):
    m = _case()["maps"][name]
    err = (m["x2"] - m["x2_tap"]).abs().max().item()
    print(f"{name}: max |x2 from the helper's P - oracle tap| = {err:.2e} (bound 1e-5), |x2| max {m['x2_tap'].abs().max().item():.2f}")
    assert err <= 1e-5
    P = m["probs"]
    heads = {"enc3": 3, "enc5": 4}.get(name, 6)
    shift = {"enc3": 1, "enc5": 2}.get(name, 3)
    assert tuple(P.shape) == (B, heads, L >> shift, Lt)
    assert (P.sum(dim=-1) - 1).abs().max().item() <= Lt * 2.0 ** -22
    assert torch.equal(m["mean"], align_ref.head_mean(P)) and torch.equal(m["token"], align_ref.first_argmax(m["mean"]))
    assert align_ref.spread(P, _case()["text"]) > 0.01   # the map is not flat: a comparison against it means something


def test_masked_keys_are_exactly_zero():
    c = _case()
    for name in LAYERS:
        P = c["maps"][name]["probs"]
        assert (P[1, :, :, -2:] == 0).all() and (P[1, :, :, :-2] > 0).all() and (P[0] > 0).all()


def test_all_pad_prompt_gets_uniform_attention():
    c = _case()
    text = c["text"].clone()
    text[2] = 0
    for name in ("enc3", "att_layers.1"):
        P = align_ref.attention(_sd(), c["strokes"], text, c["sigma"], c["style"], name)["probs"]
        assert torch.allclose(P[2], torch.full_like(P[2], 1.0 / Lt), rtol=0, atol=1e-7)


def test_ragged_helper_is_each_sample_alone():
    c = _case()
    lens = [136, 40, 8]
    r = align_ref.attention(_sd(), c["strokes"], c["text"], c["sigma"], c["style"], "enc5", lengths=lens)
    assert torch.allclose(r["probs"][0], c["maps"]["enc5"]["probs"][0], rtol=0, atol=1e-6)   # the full-length row is the uniform one (torch's CPU kernels: not bitwise across batch sizes)
    assert (r["probs"][1, :, 10:] == 0).all() and (r["mean"][2, 2:] == 0).all() and (r["token"][2, 2:] == -1).all() and (r["token"][2, :2] >= 0).all()


# ---------------------------------------------------------------- spans and rewrite_mask on a hand-made alignment
TOKEN = torch.tensor([[0, 0, 1, 1, 1, 3, 3, 3],
                      [2, 2, 0, 2, -1, -1, -1, -1]], dtype=torch.int32)


def test_spans_on_a_hand_made_token_array():
    spans = dhg_amd.token_spans(TOKEN, 4)
    assert spans[0] == [(0, 2), (2, 5), None, (5, 8)]     # token 2 never wins
    assert spans[1] == [(2, 3), None, (0, 4), None]        # the hull of a token's rows; rows past the length name nothing
    al = dhg_amd.Alignment(torch.zeros((2, 8, 4)), TOKEN, lengths=[8, 4])
    assert al.spans == spans


def test_rewrite_mask_on_a_hand_made_token_array():
    al = dhg_amd.Alignment(torch.zeros((2, 8, 4)), TOKEN, lengths=[8, 4])
    m = dhg_amd.rewrite_mask(al, 1, 3)
    assert m.dtype == torch.bool and tuple(m.shape) == (2, 8)
    assert m.tolist() == [[True, True, False, False, False, True, True, True],
                          [False, False, True, False, False, False, False, False]]
    m = dhg_amd.rewrite_mask(al, [0, 2], [1, 3])
    assert m.tolist() == [[False, False, True, True, True, True, True, True],
                          [False, False, True, False, False, False, False, False]]
    assert dhg_amd.rewrite_mask(al, 2, 2).tolist() == [[True] * 8, [True] * 4 + [False] * 4]    # an empty range keeps every valid row
    uniform = dhg_amd.Alignment(torch.zeros((1, 8, 4)), TOKEN[:1])
    assert dhg_amd.rewrite_mask(uniform, 3, 4).tolist() == [[True] * 5 + [False] * 3]
    for lo, hi, msg in ((2, 1, "tok_lo <= tok_hi"), (-1, 2, "0 <= tok_lo"), ([0], 2, "tok_lo has 1 entries"), (0.5, 2, "integer"), (0, [1, True], "not an integer")):
        with pytest.raises(ValueError, match=msg):
            dhg_amd.rewrite_mask(al, lo, hi)


# ---------------------------------------------------------------- validation before any device access
def _model(train=False):
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=2, max_L=64, max_Lt=4)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    return m.train() if train else m.eval()


def _no_device(monkeypatch, m):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the attention arguments were checked")
    monkeypatch.setattr(m, "_device", boom)
    monkeypatch.setattr(m, "_ensure_handle", boom)


GOOD = dict(strokes=torch.zeros((2, 64, 2)), text=torch.ones((2, 4), dtype=torch.int64), sigma=torch.full((2, 1), 0.5), style_vector=torch.zeros((2, 14, 1280)))

BAD_ATTENTION = [
    (dict(strokes=torch.zeros((2, 64, 3))), r"strokes must be \[B, T, 2\]"),
    (dict(strokes=torch.zeros((2, 64))), r"strokes must be \[B, T, 2\]"),
    (dict(strokes=torch.zeros((2, 64, 2), dtype=torch.int64)), "floating-point"),
    (dict(strokes=np.zeros((2, 64, 2), np.float32)), "floating-point tensor"),
    (dict(strokes=torch.zeros((2, 60, 2))), "multiple of 8"),
    (dict(text=torch.ones((3, 4), dtype=torch.int64)), r"text must be \[B = 2"),
    (dict(text=torch.ones((2, 4))), "integer token ids"),
    (dict(sigma=torch.zeros(3)), "one value per sample"),
    (dict(style_vector=torch.zeros((2, 14, 1000))), r"style_vector must be \[B, S, 1280\]"),
    (dict(lengths=[64]), "lengths has 1 entries"),
    (dict(lengths=[64, 12]), r"lengths\[1\] = 12"),
    (dict(layer=4), r"layer = 4 must lie in \[-4, 4\)"),
    (dict(layer=-5), "layer = -5"),
    (dict(layer="enc4"), "is not an EncoderLayer"),
    (dict(layer=1.5), "must be an integer"),
    (dict(heads=1), "heads = 1 must be a bool"),
]


@pytest.mark.parametrize("kw,msg", BAD_ATTENTION)
def test_attention_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    a = {**GOOD, **kw}
    extra = {k: a.pop(k) for k in ("lengths", "layer", "heads") if k in a}
    with pytest.raises(ValueError, match=msg):
        dhg_amd.attention(m, a["strokes"], a["text"], a["sigma"], a["style_vector"], **extra)


@pytest.mark.parametrize("kw", [dict(), dict(layer="enc3"), dict(layer=0, heads=True), dict(layer=-4, lengths=[8, 64]), dict(layer=np.int64(3))])
def test_valid_attention_arguments_get_as_far_as_the_device(monkeypatch, kw):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.attention(m, GOOD["strokes"], GOOD["text"], GOOD["sigma"], GOOD["style_vector"], **kw)


BAD_ALIGN = [
    (dict(strokes=torch.zeros((2, 64, 2))), r"strokes must be \[B,L,3\]"),
    (dict(strokes=torch.zeros((2, 64, 3), dtype=torch.int32)), "floating-point"),
    (dict(strokes=torch.zeros((2, 60, 3))), "multiple of 8"),
    (dict(level=60), r"level = 60 must be an integer in \[0, T = 60\)"),
    (dict(level=-1), "level = -1"),
    (dict(level=2, T=2), r"\[0, T = 2\)"),
    (dict(level=0.5), "level = 0.5"),
    (dict(T=0), "T = 0"),
    (dict(layer="mha"), "is not an EncoderLayer"),
    (dict(lengths=[64, 60]), r"lengths\[1\] = 60"),
]


@pytest.mark.parametrize("kw,msg", BAD_ALIGN)
def test_align_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    kw = dict(kw)
    strokes = kw.pop("strokes", torch.zeros((2, 64, 3)))
    with pytest.raises(ValueError, match=msg):
        dhg_amd.align(m, strokes, GOOD["text"], GOOD["style_vector"], **kw)


def test_valid_align_arguments_get_as_far_as_the_device(monkeypatch):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.align(m, torch.zeros((2, 64, 3)), GOOD["text"], GOOD["style_vector"], lengths=[64, 8], level=3, layer="att_layers.0")


def test_return_attention_validation(monkeypatch):
    m = _model()
    _no_device(monkeypatch, m)
    args = (GOOD["strokes"], GOOD["text"], GOOD["sigma"], GOOD["style_vector"])
    for bad, msg in (("enc9", "is not an EncoderLayer"), (7, "layer = 7"), (2.0, "must be an integer")):
        with pytest.raises(ValueError, match=msg):
            m(*args, return_attention=bad)
    with pytest.raises(ValueError, match=r"lengths\[0\] = 4"):
        m(*args, lengths=[4, 64], return_attention=True)
    for ok in (True, 0, "att_layers.1", -1):
        with pytest.raises(AssertionError, match="device was touched"):
            m(*args, return_attention=ok)
    # inference only: train mode, or gradient recording on parameters that require gradients
    t = _model(train=True)
    _no_device(monkeypatch, t)
    with pytest.raises(ValueError, match="inference-only"):
        t(*args, return_attention=True)
    with pytest.raises(ValueError, match="inference-only"):
        dhg_amd.attention(t, *args)
    t.eval()
    with pytest.raises(ValueError, match="inference-only"):   # (eval() keeps requires_grad: still a grad-recording call)
        t(*args, return_attention="enc3")
    with torch.no_grad(), pytest.raises(AssertionError, match="device was touched"):
        t(*args, return_attention="enc3")


def test_layer_index_numbering():
    f = dhg_amd.model.attention_layer_index
    assert [f(n, 2) for n in ("enc3", "enc5", "att_layers.0", "att_layers.1")] == [0, 1, 2, 3]
    assert f(True, 2) == 3 and f(-1, 2) == 3 and f(-4, 2) == 0 and f(True, 4) == 5 and f(0, 2) == 0


# ---------------------------------------------------------------- the C-ABI
def test_attention_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    l = _lib.lib()
    for name, nargs in (("dhw_attention", 16), ("dhw_attention_shape", 5)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert hasattr(l, name) and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    # a null handle is refused by the argument checks, which run before any HIP call: this answers without a GPU
    assert l.dhw_attention(None, None, None, None, None, 1, 8, 1, None, 0, None, None, None, None, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    assert callable(dhg_amd.attention) and callable(dhg_amd.align) and callable(dhg_amd.rewrite_mask)


def test_attention_shape_values():
    l = _lib.lib()
    C = _lib.C
    want = {40: [(3, 20), (4, 10), (6, 5), (6, 5)], 488: [(3, 244), (4, 122), (6, 61), (6, 61)]}
    for Lq, rows in want.items():
        for layer, (heads, n) in enumerate(rows):
            H, N = C.c_int(-1), C.c_int(-1)
            assert l.dhw_attention_shape(None, layer, Lq, C.byref(H), C.byref(N)) == 0
            assert (H.value, N.value) == (heads, n), (Lq, layer)
    for layer, Lq, what in ((-1, 40, "layer = -1"), (0, 44, "L = 44"), (0, 0, "L = 0")):
        assert l.dhw_attention_shape(None, layer, Lq, None, None) == -1
        msg = l.dhw_last_error(None).decode()
        assert what in msg and "dhw_attention_shape" in msg


# ---------------------------------------------------------------- the command line
def test_infer_cli_align_dispatch(monkeypatch, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake_align(prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, **kw):
        seen.update(prompts=prompts, strokes=strokes_path, source=source)
        tok = dhg_amd.Tokenizer()
        token = torch.tensor([[0, 0, 1, 1, 2, 2, 2, 2], [1, 1, 1, 1, -1, -1, -1, -1]], dtype=torch.int32)
        al = dhg_amd.Alignment(torch.zeros((2, 1, 3)), token, lengths=[8, 4])
        return al, [tok.encode("ab"), tok.encode("c")], [8, 4]

    monkeypatch.setattr(dhg_amd, "align_file", fake_align)
    f = tmp_path / "lines.txt"
    f.write_text("ab\nc\n")
    monkeypatch.chdir(tmp_path)
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--align", "old.npy", "--output", "page"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert seen == dict(prompts=["ab", "c"], strokes="old.npy", source="style.npy")
    assert lines[:5] == ["line 0: 'a' rows 0..2", "line 0: 'b' rows 2..4", "line 0: '<end>' rows 4..8", "line 1: 'c' no rows", "line 1: '<end>' rows 0..4"]
    z = np.load(tmp_path / "page_align.npz")
    assert sorted(z.files) == ["lengths", "mean", "token"] and z["token"].shape == (2, 8) and z["lengths"].tolist() == [8, 4]
    assert not list(tmp_path.glob("*.png"))
    for bad in (["--score", "x.npy"], ["--restyle", "x.npy"], ["--candidates", "2"], ["--save-strokes", "y.npy"]):
        with pytest.raises(SystemExit):
            infer.main(["--prompts-file", str(f), "style.npy", "--align", "old.npy", *bad])
    with pytest.raises(SystemExit):
        infer.main(["one prompt", "style.npy", "--align", "old.npy"])
