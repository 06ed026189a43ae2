"""Attention maps (include/dhw.h dhw_attention; ``attention``, ``align``, ``rewrite_mask``, ``model(..., return_attention=)``):
which text token each stroke row attends to.  Runs on the MI355X only (-m gpu).

Contract (include/dhw.h, rules 1-6): eps / pen are the forward's, bit for bit; the probabilities are the fp32 softmax of the
stored Q and K; mean and token follow from the returned probabilities exactly; a ragged row equals its alone run, bitwise;
the call leaves the sampler's cached graphs alone.

Against the CPU helper (tests/align_ref.py, proven on the CPU by tests/test_align_cpu.py) the bound is four times the error
the first MI355X run measured against that helper, per precision, over every layer of cases A and B:
    fp32   measured 3.278e-07 (probs; mean 1.490e-07)   bound 1.311e-06
    bf16   measured 2.507e-03 (probs; mean 1.170e-03)   bound 1.003e-02
(the fp32 figure is two to three fp32 ulps of a probability near 0.25: the order of the 64-term dot product and of the
softmax sums; the bf16 figure is the bf16 rounding of the stored Q and K, 2^-9 relative, through logits of order 1)
and it has to stay below 1/100 (fp32) and 1/4 (bf16) of the reference's own contrast — the median over rows of max - min over
the valid keys, 0.083 / 0.098 / 0.092 / 0.134 for enc3 / enc5 / att_layers.0 / att_layers.1 on these weights — so that the
comparison can tell the right map from a flat one.  Every oracle test prints error, bound and contrast before it asserts.

Shapes: A = (B=2, L=40, Lt=5): Lq = 20 / 10 / 5, one partial 16-row tile.  B = (B=3, L=136, Lt=7, lens 136 / 40 / 8):
Lq = 68 / 34 / 17, a full tile plus one row, and a sample of one row at L/8.  The last two tokens of prompt 1 are padding.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_ref  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = {"fp32": 4 * 3.278e-7, "bf16": 4 * 2.507e-3}   # 4 x the measured error (module docstring)
CONTRAST_SHARE = {"fp32": 1 / 100, "bf16": 1 / 4}
LAYERS = align_ref.layer_names(2)
CASES = {"A": dict(B=2, L=40, Lt=5, lens=None, seed=5), "B": dict(B=3, L=136, Lt=7, lens=[136, 40, 8], seed=6)}
_MODELS, _CACHE = {}, {}


def _sd(**kw):
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2, **kw).items()}


def fresh_model(prec, **cap):
    m = dhg_amd.DiffusionModel(2, precision=prec, **{**dict(max_B=8, max_L=488, max_Lt=40), **cap}).eval()
    m.load_state_dict(_sd(), strict=True)
    return m


def get_model(prec):
    if prec not in _MODELS:
        _MODELS[prec] = fresh_model(prec)
    return _MODELS[prec]


def case(name):
    """Inputs of case A / B (CPU tensors), built once."""
    if name not in _CACHE:
        c = CASES[name]
        inp = spec.synthetic_inputs(c["B"], c["L"], c["Lt"], seed=c["seed"], T=1)
        text = torch.from_numpy(inp["text"])
        text[1, -2:] = 0
        sigma = torch.tensor([0.9, 0.5, 0.2][:c["B"]])
        _CACHE[name] = dict(strokes=torch.from_numpy(inp["strokes"]), text=text, sigma=sigma, style=torch.from_numpy(inp["style"]), lens=c["lens"], ref={})
    return _CACHE[name]


def reference(name, layer, sd=None):
    """align_ref's maps of one layer of a case, computed once and shared."""
    c = case(name)
    if layer not in c["ref"]:
        c["ref"][layer] = align_ref.attention(sd or _sd(), c["strokes"], c["text"], c["sigma"], c["style"], layer, lengths=c["lens"])
    return c["ref"][layer]


def run(m, c, layer, lens="case", **kw):
    """(mean, token, probs) on the CPU."""
    lens = c["lens"] if lens == "case" else lens
    mean, token, probs = dhg_amd.attention(m, c["strokes"].cuda(), c["text"].cuda(), c["sigma"].cuda(), c["style"].cuda(), lengths=lens, layer=layer, heads=True, **kw)
    return mean.cpu(), token.cpu(), probs.cpu()


# ---------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_oracle(prec, name):
    """Every layer against align_ref; BOUND[prec] (module docstring); error, bound and the reference's contrast are printed first."""
    c, m = case(name), get_model(prec)
    fails = []
    for layer in LAYERS:
        ref = reference(name, layer)
        mean, token, probs = run(m, c, layer)
        assert probs.shape == ref["probs"].shape and mean.shape == ref["mean"].shape and torch.isfinite(probs).all()
        ep, em = (probs - ref["probs"]).abs().max().item(), (mean - ref["mean"]).abs().max().item()
        contrast = align_ref.spread(ref["probs"], c["text"], c["lens"], align_ref.SHIFT.get(layer, 3))
        agree = (token == ref["token"]).float().mean().item()
        print(f"{prec} case {name} {layer}: max |probs - ref| {ep:.3e}, max |mean - ref| {em:.3e}, bound {BOUND[prec]:.1e}, "
              f"reference contrast {contrast:.3f} (bound must stay below {CONTRAST_SHARE[prec] * contrast:.2e}), tokens equal to the reference's {agree:.3f}")
        if not (ep <= BOUND[prec] and em <= BOUND[prec] and BOUND[prec] < CONTRAST_SHARE[prec] * contrast):
            fails.append((layer, ep, em, contrast))
    assert not fails, fails


# ---------------------------------------------------------------- 2. row sums, masked keys
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_rows_sum_to_one_and_masked_keys_are_zero(prec):
    for name in ("A", "B"):
        c = case(name)
        for layer in LAYERS:
            _, _, probs = run(get_model(prec), c, layer)
            Lt, sh = c["text"].shape[1], align_ref.SHIFT.get(layer, 3)
            for b in range(probs.shape[0]):
                n = probs.shape[2] if c["lens"] is None else c["lens"][b] >> sh
                dev = (probs[b, :, :n].double().sum(dim=-1) - 1).abs().max().item()
                assert dev <= Lt * 2.0 ** -22, (name, layer, b, dev)
            assert (probs[1, :, :, -2:] == 0).all() and (probs[0] >= 0).all()
    # an all-pad prompt: 1/Lt everywhere, as the reference gives it
    c = case("A")
    text = c["text"].clone()
    text[0] = 0
    mean, token, probs = dhg_amd.attention(get_model(prec), c["strokes"].cuda(), text.cuda(), c["sigma"].cuda(), c["style"].cuda(), layer=0, heads=True)
    assert torch.allclose(probs[0].cpu(), torch.full((3, 20, 5), 0.2), rtol=0, atol=2 ** -24) and (token[0].cpu() == 0).all()


# ---------------------------------------------------------------- 3. mean and token follow from the returned probabilities
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mean_and_token_follow_from_the_returned_probabilities(prec):
    for name in ("A", "B"):
        c = case(name)
        for layer in LAYERS:
            mean, token, probs = run(get_model(prec), c, layer)
            assert torch.equal(mean, align_ref.head_mean(probs)), (name, layer)     # bitwise: head order, then * fp32(1/H)
            want = align_ref.first_argmax(mean)
            if c["lens"] is not None:
                sh = align_ref.SHIFT.get(layer, 3)
                for b, n in enumerate(c["lens"]):
                    want[b, n >> sh:] = -1
            assert token.dtype == torch.int32 and torch.equal(token, want), (name, layer)
    # each output alone gives the same bits (probs only through the model's call)
    m, c = get_model(prec), case("A")
    _, _, probs = run(m, c, 1)
    e, p, only = m(c["strokes"].cuda(), c["text"].cuda(), c["sigma"].cuda(), c["style"].cuda(), return_attention="enc5")
    assert torch.equal(only.cpu(), probs) and tuple(only.shape) == (2, 4, 10, 5)
    assert torch.equal(m(c["strokes"].cuda(), c["text"].cuda(), c["sigma"].cuda(), c["style"].cuda(), return_attention=True)[2].cpu(), run(m, c, 3)[2])


# ---------------------------------------------------------------- 4. eps / pen are the forward's
def _forward_equal(m, c):
    args = (c["strokes"].cuda(), c["text"].cuda(), c["sigma"].cuda(), c["style"].cuda())
    e0, p0, none = m(*args, lengths=c["lens"])
    assert none is None
    for layer in (0, 3):
        e1, p1, probs = m(*args, lengths=c["lens"], return_attention=layer)
        assert torch.isfinite(e1).all() and torch.equal(e0, e1) and torch.equal(p0, p1), layer
    return probs.cpu()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_outputs_are_bitwise_the_forwards(prec, monkeypatch):
    fused = {n: _forward_equal(get_model(prec), case(n)) for n in ("A", "B")}
    monkeypatch.setenv("DHW_FUSE", "0")   # (read at dhw_create: one launch per GEMM)
    m = fresh_model(prec)
    for n in ("A", "B"):
        probs = _forward_equal(m, case(n))
        ref = reference(n, LAYERS[3])["probs"]
        assert (probs - ref).abs().max().item() <= BOUND[prec]   # the other launch path's map is the model's map too
        assert probs.shape == fused[n].shape


# ---------------------------------------------------------------- 5. ragged rows
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ragged_rows_equal_their_alone_runs(prec):
    c, m = case("B"), get_model(prec)
    dirty = c["strokes"].clone()
    for b, n in enumerate(c["lens"]):
        dirty[b, n:] = float("nan")
    for layer in LAYERS:
        sh = align_ref.SHIFT.get(layer, 3)
        mean, token, probs = run(m, c, layer)
        for b, n in enumerate(c["lens"]):
            one = dict(strokes=c["strokes"][b:b + 1, :n], text=c["text"][b:b + 1], sigma=c["sigma"][b:b + 1], style=c["style"][b:b + 1])
            m1, t1, p1 = run(m, one, layer, lens=None)
            q = n >> sh
            assert torch.equal(probs[b, :, :q], p1[0]) and torch.equal(mean[b, :q], m1[0]) and torch.equal(token[b, :q], t1[0]), (layer, b)
            assert (probs[b, :, q:] == 0).all() and (mean[b, q:] == 0).all() and (token[b, q:] == -1).all() and (token[b, :q] >= 0).all()
        # nothing of strokes past lens[b] is read
        m2, t2, p2 = run(m, dict(c, strokes=dirty), layer)
        assert torch.equal(p2, probs) and torch.equal(m2, mean) and torch.equal(t2, token), layer
    # every length full: the uniform call
    a = case("A")
    for layer in (0, 2):
        u, r = run(m, a, layer, lens=None), run(m, a, layer, lens=[40, 40])
        assert all(torch.equal(x, y) for x, y in zip(u, r))


# ---------------------------------------------------------------- 6. the sampler is left alone
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_attention_call_leaves_the_sampler_alone(prec):
    """The pattern of test_gpu_score's test_score_call_leaves_the_sampler_alone: the graph cache has no public counter, so the
    check is that the replayed sample has the first one's bits (a dropped or re-captured graph would still have to)."""
    m = fresh_model(prec)
    c = case("B")
    tx, sv = c["text"].cuda(), c["style"].cuda()
    kw = dict(L=136, T=3, seed=7, first_sample=2, lengths=c["lens"])
    first = dhg_amd.sample(m, tx, sv, **kw).cpu()                 # captures the graph
    plans = m.persistent_plans()
    al = dhg_amd.align(m, first.cuda(), tx, sv, lengths=c["lens"], T=3, level=1)
    again = dhg_amd.sample(m, tx, sv, **kw).cpu()                 # replays it
    assert torch.isfinite(first).all() and torch.equal(first, again) and m.persistent_plans() == plans
    al2 = dhg_amd.align(m, first.cuda(), tx, sv, lengths=c["lens"], T=3, level=1)
    assert torch.equal(al.mean, al2.mean) and torch.equal(al.token, al2.token)   # bit-deterministic


def test_persistent_step_handle_gives_the_same_map(monkeypatch):
    monkeypatch.setenv("DHW_PERSIST", "1")
    m = fresh_model("bf16")
    got = run(m, case("B"), 2)                                    # handle created under the switch
    monkeypatch.delenv("DHW_PERSIST")
    want = run(get_model("bf16"), case("B"), 2)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


# ---------------------------------------------------------------- 7. errors at the C-ABI
def test_c_abi_rejects_bad_arguments_and_keeps_the_handle():
    m = get_model("bf16")
    c = case("B")
    want = run(m, c, 1)
    Bq, L, Lt = 3, 136, 7
    s, t, sg, sv = c["strokes"].cuda(), c["text"].cuda(), c["sigma"].cuda(), c["style"].cuda()
    eps, pen = torch.full((Bq, L, 2), float("nan"), device="cuda"), torch.full((Bq, L), float("nan"), device="cuda")
    probs = torch.full((Bq * 4 * 34 * Lt + 4,), float("nan"), device="cuda")
    mean = torch.full((Bq * 34 * Lt + 4,), float("nan"), device="cuda")
    token = torch.full((Bq, 34), -7, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(h=m._handle, strokes=s.data_ptr(), text=t.data_ptr(), sigma=sg.data_ptr(), style=sv.data_ptr(), B=Bq, L=L, Lt=Lt, lens=c["lens"], layer=1,
                 probs=probs.data_ptr(), mean=mean.data_ptr(), token=token.data_ptr(), eps=eps.data_ptr(), pen=pen.data_ptr())
        a.update(kw)
        ln = (C.c_int32 * len(a["lens"]))(*a["lens"]) if a["lens"] is not None else None
        rc = _lib.lib().dhw_attention(a["h"], a["strokes"], a["text"], a["sigma"], a["style"], a["B"], a["L"], a["Lt"], ln, a["layer"], a["probs"], a["mean"],
                                      a["token"], a["eps"], a["pen"], st)
        return rc, _lib.lib().dhw_last_error(m._handle).decode()

    for kw, what in ((dict(strokes=None), "strokes"), (dict(text=None), "text"), (dict(sigma=None), "sigma"), (dict(style=None), "style"),
                     (dict(L=140), "L=140"), (dict(B=9), "B=9"), (dict(Lt=41), "Lt=41"), (dict(lens=[136, 44, 8]), "lens[1] = 44"),
                     (dict(layer=4), "layer = 4"), (dict(layer=-1), "layer = -1"), (dict(eps=None), "eps_out"), (dict(pen=None), "pen_out"),
                     (dict(probs=None, mean=None, token=None), "all NULL"),
                     (dict(probs=probs.data_ptr() + 4), "probs_out"), (dict(mean=mean.data_ptr() + 8), "mean_out")):
        rc, msg = call(**kw)
        assert rc == -1 and what in msg and "dhw_attention" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(eps).all() and torch.isnan(probs).all() and (token == -7).all()   # nothing was launched
    rc, msg = call()
    assert rc == 0, msg
    n = Bq * 4 * 34 * Lt
    assert torch.equal(probs[:n].cpu().reshape(Bq, 4, 34, Lt), want[2]) and torch.equal(mean[:Bq * 34 * Lt].cpu().reshape(Bq, 34, Lt), want[0])
    assert torch.equal(token.cpu(), want[1])
    # the shape query on a handle knows the handle's limits
    H, N = C.c_int(), C.c_int()
    assert _lib.lib().dhw_attention_shape(m._handle, 3, 488, C.byref(H), C.byref(N)) == 0 and (H.value, N.value) == (6, 61)
    assert _lib.lib().dhw_attention_shape(m._handle, 4, 488, None, None) == -1 and _lib.lib().dhw_attention_shape(m._handle, 0, 496, None, None) == -1


def test_a_row_without_a_finite_value_gets_token_zero():
    """Rule 3: NaN compares larger than nothing, so a row of `mean` that is NaN throughout gets token 0, never a value outside
    [0, Lt).  NaN strokes make every query NaN while the text keys stay finite."""
    c = case("A")
    for layer in (0, 3):
        mean, token, _ = run(get_model("fp32"), dict(c, strokes=torch.full_like(c["strokes"], float("nan"))), layer, lens=None)
        assert torch.isnan(mean).all() and (token == 0).all(), layer


def test_c_abi_refuses_a_prompt_longer_than_the_kernels_tile():
    """Rule 5's last check: Lt <= 168, the longest prompt whose H x 16 x Lt tile fits the kernel's 64 KiB of LDS.  Only a handle
    with a larger max_Lt can get as far as that check; it is refused before dhw_finalize, so the handle needs no weights."""
    l, h = _lib.lib(), C.c_void_p()
    dims = _lib.DhwDims(num_layers=2, c1=128, c2=192, c3=256, max_B=1, max_L=8, max_Lt=176, S=14, precision=_lib.PREC_BF16)
    _lib.check(l.dhw_create(C.byref(h), C.byref(dims), torch.cuda.current_device()))
    try:
        s, t = torch.zeros((1, 8, 2), device="cuda"), torch.ones((1, 169), dtype=torch.int64, device="cuda")
        sg, sv = torch.ones(1, device="cuda"), torch.zeros((1, 14, 1280), device="cuda")
        eps, pen, token = torch.zeros((1, 8, 2), device="cuda"), torch.zeros((1, 8), device="cuda"), torch.full((1, 1), -7, dtype=torch.int32, device="cuda")
        rc = l.dhw_attention(h, s.data_ptr(), t.data_ptr(), sg.data_ptr(), sv.data_ptr(), 1, 8, 169, None, 3, None, None, token.data_ptr(), eps.data_ptr(),
                             pen.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = l.dhw_last_error(h).decode()
        assert rc == -1 and "Lt = 169" in msg and "168" in msg and "dhw_attention" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert (token == -7).all()
    finally:
        l.dhw_destroy(h)


# ---------------------------------------------------------------- 8. a narrower model: the folded head scale
def test_c2_96_model_against_the_reference():
    """c = (128, 96, 256): heads of 32 channels run zero-padded to 64 with sqrt(64/32) folded into Wq, so the kernel's fixed
    1/8 has to come out as 1/sqrt(32).  fp32, case A, layer 2."""
    sd = _sd(c2=96)
    m = dhg_amd.DiffusionModel(2, 128, 96, 256, precision="fp32", max_B=2, max_L=40, max_Lt=5).eval()
    m.load_state_dict(sd, strict=True)
    c = case("A")
    ref = align_ref.attention(sd, c["strokes"], c["text"], c["sigma"], c["style"], "att_layers.0")
    mean, token, probs = run(m, c, 2)
    ep, em = (probs - ref["probs"]).abs().max().item(), (mean - ref["mean"]).abs().max().item()
    contrast = align_ref.spread(ref["probs"], c["text"])
    print(f"c2=96 fp32 att_layers.0: max |probs - ref| {ep:.3e}, max |mean - ref| {em:.3e}, bound {BOUND['fp32']:.1e}, reference contrast {contrast:.3f}")
    assert ep <= BOUND["fp32"] and em <= BOUND["fp32"] and BOUND["fp32"] < contrast / 100


# ---------------------------------------------------------------- 9. end to end
def test_align_and_rewrite_a_sampled_line():
    m = get_model("bf16")
    tok = dhg_amd.Tokenizer()
    prompts = ["Hi", "Rabbit"]
    sv = torch.from_numpy(spec.synthetic_inputs(1, 8, 1, seed=9)["style"])
    text, lens, svb = dhg_amd.inference._encode_batch("test", prompts, sv)
    Lt, L = text.shape[1], max(lens)
    line = dhg_amd.sample(m, text.cuda(), svb.cuda(), L=L, T=3, seed=4, lengths=lens)
    al = dhg_amd.align(m, line, text.cuda(), svb.cuda(), lengths=lens, T=3)
    token = al.token.cpu()
    assert tuple(token.shape) == (2, L) and tuple(al.mean.shape) == (2, L // 8, Lt) and token.dtype == torch.int32
    assert ((token >= -1) & (token < Lt)).all()
    for b, n in enumerate(lens):
        assert (token[b, :n] >= 0).all() and (token[b, n:] == -1).all()
        assert (token[b, :n] < len(tok.encode(prompts[b]))).all()           # padding tokens never win
        for k, span in enumerate(al.spans[b]):
            rows = (token[b] == k).nonzero().flatten()
            assert (span is None) == (rows.numel() == 0)
            if span is not None:
                assert span == (int(rows[0]), int(rows[-1]) + 1)
    keep = dhg_amd.rewrite_mask(al, 0, 2)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (2, L) and not keep[0, lens[0]:].any()
    again = dhg_amd.sample(m, text.cuda(), svb.cuda(), L=L, T=3, seed=11, lengths=lens, known=line, keep=keep.cuda())
    k = keep.cpu()
    assert torch.equal(again.cpu()[k], line.cpu()[k]) and torch.isfinite(again).all()
    if (~k[1, :lens[1]]).any():
        assert not torch.equal(again.cpu()[1, :lens[1]][~k[1, :lens[1]]], line.cpu()[1, :lens[1]][~k[1, :lens[1]]])
