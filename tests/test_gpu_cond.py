"""Conditioned sampling (include/dhw.h dhw_sample_cond; ``sample(..., known=, keep=, t_start=, cond_noise=)``, ``restyle``):
replacement conditioning of the reverse process.  Runs on the MI355X only (-m gpu).

Contract (include/dhw.h, rules 1-7): kept rows of the output are ``known`` bit for bit; with nothing kept and t_start = T the
call is the plain one bit for bit, whatever ``known`` holds; the conditioning stream is the generator at iteration 2^30 + k;
a ragged row equals its alone run, a shard its rows, a graph replay the eager launches — all bitwise.  Against the CPU
helper (tests/cond_ref.py, proven on the CPU by tests/test_cond_cpu.py) the fp32 loop stays within the bound of
test_gpu_parity.test_short_sampling_matches_oracle_T_generalised for the unconditioned loop: 1e-4.
Measured on the MI355X: 1.2e-6 / 4.8e-7 (new, t_start 9 / 4), 9.5e-7 / 2.4e-7 (standard).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec
from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_ref  # noqa: E402

pytestmark = pytest.mark.gpu

B, L, Lt, T = 3, 72, 7, 3
LENS = [72, 40, 8]
_MODELS = {}


def _sd():
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}


def fresh_model(prec):
    m = dhg_amd.DiffusionModel(2, precision=prec, max_B=8, max_L=488, max_Lt=40).eval()
    m.load_state_dict(_sd(), strict=True)
    return m


def get_model(prec):
    if prec not in _MODELS:
        _MODELS[prec] = fresh_model(prec)
    return _MODELS[prec]


def _cuda(*arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def _known(b, l, seed):
    """known [b,l,3]: dx, dy ~ N(0,1), pen in {0,1}."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn((b, l, 3), generator=g)
    k[..., 2] = (k[..., 2] > 0).float()
    return k


def _mask(b, l, seed, p=0.4):
    return torch.rand((b, l), generator=torch.Generator().manual_seed(seed)) < p


# ---------------------------------------------------------------- 1. nothing conditioned == the plain call, bit for bit
@pytest.mark.parametrize("lengths", [None, LENS])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_identity_nothing_kept_full_schedule(prec, lengths):
    m = get_model(prec)
    inp = spec.synthetic_inputs(B, L, Lt, seed=21, T=T)
    tx, sv, nz = _cuda(inp["text"], inp["style"], inp["noise"])
    nan3 = torch.full((B, L, 3), float("nan"), device="cuda")
    nan_cz = torch.full((T, B, L, 2), float("nan"), device="cuda")
    none = torch.zeros((B, L), dtype=torch.bool, device="cuda")
    for mode in ("new", "standard"):
        for noise in (None, nz):
            kw = dict(L=L, T=T, diffusion_mode=mode, noise=noise, seed=7, first_sample=2, lengths=lengths)
            plain = dhg_amd.sample(m, tx, sv, **kw).cpu()
            got = dhg_amd.sample(m, tx, sv, known=nan3, keep=none, t_start=T, cond_noise=nan_cz if noise is not None else None, **kw).cpu()
            assert torch.isfinite(plain).all() and torch.equal(got, plain), (mode, noise is None)
            got = dhg_amd.sample(m, tx, sv, known=None, t_start=T, **kw).cpu()
            assert torch.equal(got, plain), (mode, noise is None, "known=None")
            got = dhg_amd.sample(m, tx, sv, known=nan3, **kw).cpu()   # known given, nothing seeded: never read
            assert torch.equal(got, plain), (mode, noise is None, "keep=None")


# ---------------------------------------------------------------- 2. everything kept == known, pen included
@pytest.mark.parametrize("t_start", [3, 1])
def test_everything_kept_returns_known(t_start):
    m = get_model("bf16")
    inp = spec.synthetic_inputs(B, L, Lt, seed=22, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    known = _known(B, L, 5)
    allk = torch.ones((B, L), dtype=torch.bool)
    for mode in ("new", "standard"):
        out = dhg_amd.sample(m, tx, sv, L=L, T=T, diffusion_mode=mode, seed=1, known=known.cuda(), keep=allk.cuda(), t_start=t_start).cpu()
        assert torch.equal(out, known), mode
    out = dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1, lengths=LENS, known=known.cuda(), keep=allk.to(torch.uint8).cuda(), t_start=t_start).cpu()
    for b, n in enumerate(LENS):
        assert torch.equal(out[b, :n], known[b, :n]) and not out[b, n:].any(), b


# ---------------------------------------------------------------- 3. the conditioned loop against the CPU helper
_ORACLE = {}


def _oracle_case():
    """Inputs of the oracle test (the shape of test_short_sampling_matches_oracle_T_generalised), built once and shared."""
    if not _ORACLE:
        Bo, Lo, Lto, To = 2, 40, 5, 9
        inp = spec.synthetic_inputs(Bo, Lo, Lto, seed=5, T=To)
        g = torch.Generator().manual_seed(17)
        keep = torch.zeros((Bo, Lo), dtype=torch.bool)
        keep[0, 5:22] = True   # rows 5..21 of sample 0 (not aligned to 8), none of sample 1
        _ORACLE.update(sd=_sd(), text=torch.from_numpy(inp["text"]), style=torch.from_numpy(inp["style"]), noise=torch.from_numpy(inp["noise"]),
                       known=_known(Bo, Lo, 18), keep=keep, cond_noise=torch.randn((To, Bo, Lo, 2), generator=g), L=Lo, T=To)
    return _ORACLE


@pytest.mark.parametrize("t_start", [9, 4])
@pytest.mark.parametrize("mode", ["new", "standard"])
def test_oracle(mode, t_start):
    """fp32, B=2, L=40, Lt=5, T=9: max|out - cond_ref| < 1e-4 (measured on the MI355X: new 1.19e-06 / 4.77e-07 at t_start 9 / 4,
    standard 9.54e-07 / 2.38e-07; max|ref| 4.3-5.0), kept rows bitwise.  Each figure is printed before the assertion."""
    o = _oracle_case()
    ref = cond_ref.cond_sample(ref_cpu.forward, o["sd"], o["text"], o["style"], o["L"], o["noise"], T=o["T"], mode=mode, known=o["known"],
                               keep=o["keep"], t_start=t_start, cond_noise=o["cond_noise"])
    m = get_model("fp32")
    out = dhg_amd.sample(m, o["text"].cuda(), o["style"].cuda(), L=o["L"], T=o["T"], diffusion_mode=mode, noise=o["noise"].cuda(),
                         known=o["known"].cuda(), keep=o["keep"].cuda(), t_start=t_start, cond_noise=o["cond_noise"].cuda()).cpu()
    err = (out - ref).abs().max().item()
    print(f"conditioned loop vs cond_ref [{mode}, t_start={t_start}]: max abs error {err:.3e} (max|ref| {ref.abs().max().item():.3g})")
    assert torch.isfinite(out).all()
    assert err < 1e-4
    assert torch.equal(out[o["keep"]], o["known"][o["keep"]])


# ---------------------------------------------------------------- 4. the conditioning stream is the generator at 2^30 + k
def test_conditioning_stream_is_pinned():
    m = fresh_model("fp32")
    inp = spec.synthetic_inputs(B, L, Lt, seed=23, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    known = _known(B, L, 6)
    seed, first = 11, 4
    cap = m.set_teacher(torch.zeros((T - 1, B, L, 2), device="cuda"), 1)   # capture x after every step (eager launches)
    try:
        out = dhg_amd.sample(m, tx, sv, L=L, T=T, seed=seed, first_sample=first, known=known.cuda(),
                             keep=torch.ones((B, L), dtype=torch.bool, device="cuda")).cpu()
        cap = cap.cpu().numpy()
    finally:
        m.set_teacher(None)
        m._apply_teacher()
    assert torch.equal(out, known)
    _, abar = _lib.schedule(T)
    kxy = known[..., :2].numpy()
    one = np.float32(1.0)
    for k in range(T - 1):
        i = T - 1 - k
        a_next = abar[i - 1] if i > 1 else one
        ka, kb = np.sqrt(a_next), np.sqrt(one - a_next)
        assert ka.dtype == np.float32 and kb.dtype == np.float32

        def expect(it):
            z = m.debug_randn(seed, first, B, L, it).numpy()
            return ka * kxy + kb * z   # fp32: one rounding per operation, no contraction

        want = expect(2 ** 30 + k)
        assert want.dtype == np.float32 and np.array_equal(cap[k], want), k
        if kb > 0:
            assert not np.array_equal(cap[k], expect(k)), k   # not the sampler's own draw of that iteration
    assert abar[1] < 1   # (k = 0 is noised: the comparison above is not vacuous)


# ---------------------------------------------------------------- 5. a ragged row equals its alone run
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_ragged_rows_equal_their_alone_runs(prec):
    m = get_model(prec)
    inp = spec.synthetic_inputs(B, L, Lt, seed=24, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    known, keep = _known(B, L, 7).cuda(), _mask(B, L, 8).cuda()
    for t_start in (3, 2):
        out = dhg_amd.sample(m, tx, sv, L=L, T=T, seed=5, first_sample=1, lengths=LENS, known=known, keep=keep, t_start=t_start).cpu()
        for b, n in enumerate(LENS):
            alone = dhg_amd.sample(m, tx[b:b + 1].contiguous(), sv[b:b + 1].contiguous(), L=n, T=T, seed=5, first_sample=1 + b,
                                   known=known[b:b + 1, :n].contiguous(), keep=keep[b:b + 1, :n].contiguous(), t_start=t_start).cpu()
            assert torch.equal(out[b, :n], alone[0]), (t_start, b)
            assert not out[b, n:].any()
            kb = keep[b, :n].cpu()
            assert kb.any() and torch.equal(out[b, :n][kb], known[b, :n].cpu()[kb])


# ---------------------------------------------------------------- 6. sharding
def _shard_case(m):
    Bs = 4
    inp = spec.synthetic_inputs(Bs, L, Lt, seed=25, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    known, keep = _known(Bs, L, 9).cuda(), _mask(Bs, L, 10).cuda()
    assert keep[:2].any() and keep[2:].any()
    kw = dict(L=L, T=T, seed=6, t_start=2)
    full = dhg_amd.sample(m, tx, sv, first_sample=0, known=known, keep=keep, **kw).cpu()
    halves = [dhg_amd.sample(m, tx[s:s + 2].contiguous(), sv[s:s + 2].contiguous(), first_sample=s, known=known[s:s + 2].contiguous(),
                             keep=keep[s:s + 2].contiguous(), **kw).cpu() for s in (0, 2)]
    return full, torch.cat(halves)


def test_shards_equal_the_whole_batch():
    full, parts = _shard_case(get_model("bf16"))
    assert torch.isfinite(full).all() and torch.equal(full, parts)
    _ORACLE["shard_full"] = full


def test_shards_equal_the_whole_batch_on_two_streams(monkeypatch):
    monkeypatch.setenv("DHW_STREAMS", "2")   # (read at dhw_create: the handle owns two workspaces and a side stream)
    m = fresh_model("bf16")
    inp = spec.synthetic_inputs(1, 8, 1, seed=1, T=1)
    dhg_amd.sample(m, *_cuda(inp["text"], inp["style"]), L=8, T=1)   # creates the handle
    monkeypatch.delenv("DHW_STREAMS")
    assert _lib.lib().dhw_set_streams(m._handle, 2) == 2
    full, parts = _shard_case(m)
    assert torch.equal(full, parts)
    one = _ORACLE.get("shard_full")
    if one is None:
        one, _ = _shard_case(get_model("bf16"))
    assert torch.equal(full, one)   # the sub-batch split changes nothing


# ---------------------------------------------------------------- 7. one graph serves every mask
def test_graph_replay_equals_eager_and_serves_every_mask():
    m = fresh_model("bf16")
    inp = spec.synthetic_inputs(B, L, Lt, seed=26, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    cases = [(_known(B, L, 11).cuda(), _mask(B, L, 12).cuda()), (_known(B, L, 13).cuda(), _mask(B, L, 14, p=0.7).cuda())]
    kw = dict(L=L, T=T, seed=8, lengths=LENS, t_start=2)
    got = [dhg_amd.sample(m, tx, sv, known=k, keep=q, **kw).cpu() for k, q in cases]   # capture, then a replay with another mask
    again = dhg_amd.sample(m, tx, sv, known=cases[0][0], keep=cases[0][1], **kw).cpu()
    _lib.lib().dhw_set_graph(m._handle, 0)
    try:
        eager = [dhg_amd.sample(m, tx, sv, known=k, keep=q, **kw).cpu() for k, q in cases]
    finally:
        _lib.lib().dhw_set_graph(m._handle, 1)
    assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1]) and torch.equal(again, got[0])
    assert not torch.equal(got[0], got[1])
    m2 = fresh_model("bf16")
    assert torch.equal(dhg_amd.sample(m2, tx, sv, known=cases[1][0], keep=cases[1][1], **kw).cpu(), got[1])


# ---------------------------------------------------------------- 8. errors at the C-ABI
def _raw_call(m, tx, sv, out, T_, noise, known, keep, t_start, cond_noise):
    p = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().dhw_sample_cond(m._handle, tx.data_ptr(), sv.data_ptr(), tx.shape[0], out.shape[1], tx.shape[1], None, T_, 0, p(noise), 1, 0,
                                    p(known), p(keep), t_start, p(cond_noise), out.data_ptr(), s)
    return rc, _lib.lib().dhw_last_error(m._handle).decode()


def test_c_abi_rejects_bad_conditioning_and_keeps_the_handle():
    m = get_model("bf16")
    inp = spec.synthetic_inputs(B, L, Lt, seed=27, T=T)
    tx, sv, nz = _cuda(inp["text"], inp["style"], inp["noise"])
    known, keep = _known(B, L, 15).cuda(), _mask(B, L, 16).to(torch.uint8).cuda()
    cz = torch.randn((T, B, L, 2), generator=torch.Generator().manual_seed(1)).cuda()
    ref = dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1, known=known, keep=keep, t_start=2).cpu()
    out = torch.empty((B, L, 3), device="cuda")
    for args, what in (((None, known, keep, 0, None), "t_start = 0"), ((None, known, keep, T + 1, None), "t_start = 4"),
                       ((None, None, keep, T, None), "known is NULL"), ((None, None, None, 2, None), "known is NULL"),
                       ((nz, known, keep, T, None), "cond_noise is NULL"), ((None, known, keep, T, cz), "noise is NULL"),
                       ((nz, known, None, T, cz), "keep is NULL")):
        rc, msg = _raw_call(m, tx, sv, out, T, *args)
        assert rc == -1 and what in msg and "dhw_sample_cond" in msg, (what, rc, msg)
    rc, msg = _raw_call(m, tx, sv, out, T, None, known, keep, 2, None)
    assert rc == 0, msg
    assert torch.equal(out.cpu(), ref)
    rc, msg = _raw_call(m, tx, sv, out, T, nz, known, keep, 2, cz)
    assert rc == 0, msg
    assert torch.equal(out.cpu(), dhg_amd.sample(m, tx, sv, L=L, T=T, noise=nz, known=known, keep=keep, t_start=2, cond_noise=cz).cpu())


def test_persistent_step_handle_refuses_conditioned_sampling(monkeypatch):
    monkeypatch.setenv("DHW_PERSIST", "1")
    m = fresh_model("bf16")
    inp = spec.synthetic_inputs(B, L, Lt, seed=28, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    plain = dhg_amd.sample(m, tx, sv, L=L, T=T, seed=2).cpu()   # handle created under the switch
    monkeypatch.delenv("DHW_PERSIST")
    known, keep = _known(B, L, 19).cuda(), _mask(B, L, 20).cuda()
    with pytest.raises(_lib.DhwError) as e:
        dhg_amd.sample(m, tx, sv, L=L, T=T, seed=2, known=known, keep=keep)
    assert e.value.code == -1 and "DHW_PERSIST" in str(e.value)
    assert torch.equal(dhg_amd.sample(m, tx, sv, L=L, T=T, seed=2).cpu(), plain)   # the handle still works


# ---------------------------------------------------------------- 9. end to end
def test_restyle_then_render_end_to_end():
    m = get_model("bf16")
    lens = [72, 40, 24]
    inp = spec.synthetic_inputs(B, L, Lt, seed=29)
    tx, sv = _cuda(inp["text"], inp["style"])
    sv2 = torch.from_numpy(spec.synthetic_inputs(B, L, Lt, seed=30)["style"]).cuda()
    line = dhg_amd.sample(m, tx, sv, seed=3, lengths=lens)
    new = dhg_amd.restyle(line, tx, sv2, m, lengths=lens, strength=0.5, seed=4)
    assert tuple(new.shape) == (B, L, 3) and new.is_cuda and torch.isfinite(new).all()
    images, widths = dhg_amd.render_strokes(new, lens)
    print("restyled widths:", widths.tolist())
    assert tuple(images.shape) == (B, 1, 96, 1400) and torch.isfinite(images).all()
    assert (widths > 0).all()
    for b, n in enumerate(lens):
        assert not torch.equal(new[b, :n], line[b, :n]) and not new[b, n:].any(), b
