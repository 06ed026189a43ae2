"""Deterministic sampling and inversion (include/dhw.h dhw_ddim_sample, dhw_ddim_invert, dhw_ddim_update; ``sample_ddim``,
``invert``, ``transfer``): runs on the MI355X only (-m gpu).

Shapes: B = 3, L = 72, Lt = 7 with one padded token, lens = [24, 72, 40] (tails inside a 256-thread block and a full row),
T = 9, S in {1, 4, 9}.

What is bit for bit: the update kernel against numpy float32; an S = 1 call against dhw_forward + that update; a ragged row
against its alone run; a handed-back latent; a persistent-step handle; ``sample`` before and after a ddim call.

What has a bound, and where it comes from (tests 3 and 7).  The fp32 denoiser is within TOL["fp32"] of the CPU oracle at
every call (tests/test_gpu_parity.py).  The CPU reference (tests/ddim_ref.py) is run twice on the test's inputs: plain, and
with every eps it gets moved by +-TOL["fp32"]["eps"] and every pen by +-TOL["fp32"]["pen"] (random sign per element, fixed
seed).  The bound is 4x the largest deviation between the two runs: 4x because the GPU's error is within TOL at every call
but correlated from call to call, where the random signs partly cancel.  The round trip's bound is the CPU reference's own
round-trip error plus the sampler's bound at S = 9.  Every figure is printed before it is asserted.

Measured on the CPU reference with these inputs (|x| up to 5.2, |latent| up to 3.4); the GPU's errors are in DESIGN.md §23:
    sample_ddim  S = 4: deviation x 2.4e-05, pen 2.1e-05 -> bounds 9.6e-05, 8.3e-05;  S = 9: 2.3e-05, 2.1e-05 -> 9.1e-05, 8.2e-05
    invert S = 9 iters = 1: deviation 1.4e-05 -> bound 5.8e-05;  iters = 3: 1.4e-05 -> 5.8e-05
    round trip   S = 9 iters = 1: 4.6e-02;  iters = 3: 2.8e-05
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
import ddim_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"fp32": dict(eps=2e-5, pen=2e-5), "bf16": dict(eps=2e-2, pen=5e-3)}   # test_gpu_parity.TOL
B, L, Lt, T = 3, 72, 7, 9
LENS = [24, 72, 40]
_MODELS = {}
_CACHE = {}


def _sd():
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}


def fresh_model(prec, **cap):
    m = dhg_amd.DiffusionModel(2, precision=prec, **{**dict(max_B=8, max_L=488, max_Lt=40), **cap}).eval()
    m.load_state_dict(_sd(), strict=True)
    return m


def get_model(prec):
    if prec not in _MODELS:
        _MODELS[prec] = fresh_model(prec)
    return _MODELS[prec]


def _inputs():
    """text [B,Lt] with one padded token, style, a latent ~ N(0,1) and strokes of a plausible size: built once."""
    if "inputs" not in _CACHE:
        inp = spec.synthetic_inputs(B, L, Lt, seed=61, pad=1, T=1)
        g = torch.Generator().manual_seed(62)
        latent = torch.randn((B, L, 2), generator=g)
        strokes = torch.randn((B, L, 3), generator=g)
        strokes[..., 2] = (strokes[..., 2] > 0.5).float()
        _CACHE["inputs"] = dict(text=torch.from_numpy(inp["text"]), style=torch.from_numpy(inp["style"]), latent=latent, strokes=strokes)
        assert (_CACHE["inputs"]["text"] == 0).sum() >= 1
    return _CACHE["inputs"]


def _gpu(*names):
    i = _inputs()
    return [i[n].cuda() for n in names]


def _coefs(levels):
    """[(A_j, B_j)] j = 0..S from the LIBRARY's schedule, numpy float32: what the host side of the entries computes."""
    return ddim_ref.coefs(levels, T, abar=_lib.schedule(T)[1])


def np_update(base, e, c0, c1, c2, c3):
    """U in numpy float32: five operations, each rounded on its own."""
    base, e = np.asarray(base, np.float32), np.asarray(e, np.float32)
    c0, c1, c2, c3 = (np.float32(c) for c in (c0, c1, c2, c3))
    with np.errstate(all="ignore"):
        out = c2 * ((base - c1 * e) / c0) + c3 * e
    assert out.dtype == np.float32
    return out


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _masked(x, lens):
    """x with the rows at and past lens[b] set to 0 (numpy copy)."""
    x = np.array(x, np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


# ---------------------------------------------------------------- 1. the update kernel alone, against numpy
def _raw_update(base, eps, lens_dev, c, out):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().dhw_ddim_update(base.data_ptr(), eps.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, base.shape[0], base.shape[1],
                                    float(c[0]), float(c[1]), float(c[2]), float(c[3]), out.data_ptr(), s)
    assert rc == 0, _lib.lib().dhw_last_error(None).decode()
    torch.cuda.synchronize()


def test_update_kernel_matches_numpy_bit_for_bit():
    g = torch.Generator().manual_seed(63)
    base, eps = torch.randn((B, L, 2), generator=g) * 3, torch.randn((B, L, 2), generator=g)
    base[0, 0, 0], eps[0, 0, 1], base[1, 5, 1], eps[1, 5, 1] = 0.0, 0.0, 1e-38, 0.0   # zeros, and a subnormal carried through all five operations
    co = _coefs(dhg_amd.ddim_levels(T, 4))
    sets = [(co[j][0], co[j][1], co[j + 1][0], co[j + 1][1]) for j in range(4)]              # the sampler's steps, the last to (1, 0)
    sets += [(co[j + 1][0], co[j + 1][1], co[j][0], co[j][1]) for j in range(3, -1, -1)]     # the inversion's
    sets += [(np.float32(3.0), np.float32(0.1), np.float32(1.0 / 3), np.float32(0.7))]       # a divisor that is no power of two
    lens_dev = torch.tensor(LENS, dtype=torch.int32).cuda()
    for c in sets:
        want = np_update(base.numpy(), eps.numpy(), *c)
        out = torch.full((B, L, 2), float("nan")).cuda()
        _raw_update(base.cuda(), eps.cuda(), None, c, out)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), c
        # ragged, with NaN where nothing may be read: identical valid rows, 0 past the lengths
        bd, ed = base.clone(), eps.clone()
        for b, n in enumerate(LENS):
            bd[b, n:] = float("nan")
            ed[b, n:] = float("nan")
        out = torch.full((B, L, 2), float("nan")).cuda()
        _raw_update(bd.cuda(), ed.cuda(), lens_dev, c, out)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(_masked(want, LENS))), c
    # in place (out = base), as the sampling loop uses it
    x = base.cuda()
    _raw_update(x, eps.cuda(), lens_dev, sets[0], x)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(_masked(np_update(base.numpy(), eps.numpy(), *sets[0]), LENS)))
    # more than one block with a tail: 5 * 104 = 520 rows = two full blocks and 8 rows
    b2, e2 = torch.randn((5, 104, 2), generator=g), torch.randn((5, 104, 2), generator=g)
    out = torch.empty((5, 104, 2)).cuda()
    _raw_update(b2.cuda(), e2.cuda(), None, sets[1], out)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(np_update(b2.numpy(), e2.numpy(), *sets[1])))


@pytest.mark.parametrize("lens", [None, [104, 40, 104, 8, 96]])
def test_update_writes_its_own_rows_and_nothing_behind_them(lens):
    """The unguided instantiation of the shared step kernel has no second half: base and eps hold exactly B * L rows, and the
    B * L rows that follow `out` in the same allocation (where a guided step writes its second copy) keep their pattern."""
    Bq, Lq = 5, 104   # 520 rows: two full blocks and 8 rows
    g = torch.Generator().manual_seed(34)
    base, eps = torch.randn((Bq, Lq, 2), generator=g) * 3, torch.randn((Bq, Lq, 2), generator=g)
    pattern = torch.arange(Bq * Lq * 2, dtype=torch.float32).reshape(Bq, Lq, 2) + 0.5
    buf = torch.cat((torch.full((Bq, Lq, 2), float("nan")), pattern)).cuda()
    c = (np.float32(3.0), np.float32(0.1), np.float32(1.0 / 3), np.float32(0.7))
    _raw_update(base.cuda(), eps.cuda(), None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda(), c, buf[:Bq])
    want = np_update(base.numpy(), eps.numpy(), *c)
    got = buf.cpu().numpy()
    assert np.array_equal(_bits(got[:Bq]), _bits(want if lens is None else _masked(want, lens)))
    assert np.array_equal(_bits(got[Bq:]), _bits(pattern.numpy()))


# ---------------------------------------------------------------- 2. S = 1 is one forward and one update
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_step_is_forward_then_update(prec):
    m = get_model(prec)
    text, style = _gpu("text", "style")
    levels = [5]
    out, lat = dhg_amd.sample_ddim(m, text, style, L=L, T=T, levels=levels, seed=5, first_sample=2, return_latent=True)
    assert torch.equal(lat.cpu(), m.debug_randn(5, 2, B, L, -1))            # the x_T dhw_sample draws
    (A0, B0), (A1, B1) = _coefs(levels)
    assert (A1, B1) == (1.0, 0.0)
    with torch.no_grad():
        eps, pen, _ = m(lat, text, torch.full((B, 1), float(A0), device="cuda"), style)   # dhw_forward
    want = np_update(lat.cpu().numpy(), eps.cpu().numpy(), A0, B0, A1, B1)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got[..., :2]), _bits(want)) and np.array_equal(_bits(got[..., 2]), _bits(pen.cpu().numpy().reshape(B, L)))


# ---------------------------------------------------------------- 3. fp32 against the CPU reference
def _ref():
    """The CPU reference on the shared inputs, plain and perturbed, once: sample at S = 4 and 9 from the given latent, invert at
    S = 9 with iters 1 and 3 of the line the plain S = 9 run wrote, and the round trips of those latents."""
    if "ref" in _CACHE:
        return _CACHE["ref"]
    i, sd = _inputs(), _sd()
    pert = lambda seed: ddim_ref.sign_perturb(TOL["fp32"]["eps"], TOL["fp32"]["pen"], seed)   # noqa: E731
    r = dict(sample={}, sample_p={}, invert={}, invert_p={}, trip={})
    for S in (4, 9):
        lv = dhg_amd.ddim_levels(T, S)
        r["sample"][S] = ddim_ref.sample(ref_cpu.forward, sd, i["text"], i["style"], lv, T, i["latent"], lengths=LENS)
        r["sample_p"][S] = ddim_ref.sample(ref_cpu.forward, sd, i["text"], i["style"], lv, T, i["latent"], lengths=LENS, perturb=pert(70 + S))
    lv = dhg_amd.ddim_levels(T, 9)
    r["x0"] = r["sample"][9].clone()
    for k in (1, 3):
        r["invert"][k] = ddim_ref.invert(ref_cpu.forward, sd, r["x0"], i["text"], i["style"], lv, T, iters=k, lengths=LENS)
        r["invert_p"][k] = ddim_ref.invert(ref_cpu.forward, sd, r["x0"], i["text"], i["style"], lv, T, iters=k, lengths=LENS, perturb=pert(80 + k))
        r["trip"][k] = ddim_ref.sample(ref_cpu.forward, sd, i["text"], i["style"], lv, T, r["invert"][k], lengths=LENS)
    _CACHE["ref"] = r
    return r


def _dev(a, b):
    return (a - b).abs().max().item()


def _sample_bounds(S):
    r = _ref()
    return 4 * _dev(r["sample"][S][..., :2], r["sample_p"][S][..., :2]), 4 * _dev(r["sample"][S][..., 2], r["sample_p"][S][..., 2])


def _invert_bound(k):
    r = _ref()
    return 4 * _dev(r["invert"][k], r["invert_p"][k])


@pytest.mark.parametrize("S", [4, 9])
def test_fp32_sampling_matches_the_cpu_reference(S):
    """Bound = 4x the deviation of the CPU reference under a +-TOL perturbation of every denoiser output (module docstring).
    Measured on the CPU (these inputs): S = 4: x deviation 2.4e-05 (bound 9.6e-05), pen 2.1e-05 (8.3e-05); S = 9: x 2.3e-05
    (9.1e-05), pen 2.1e-05 (8.2e-05).  GPU errors: DESIGN.md §23."""
    r = _ref()
    text, style, latent = _gpu("text", "style", "latent")
    got = dhg_amd.sample_ddim(get_model("fp32"), text, style, T=T, steps=S, latent=latent, lengths=LENS).cpu()
    bx, bp = _sample_bounds(S)
    ex, ep = _dev(got[..., :2], r["sample"][S][..., :2]), _dev(got[..., 2], r["sample"][S][..., 2])
    print(f"sample_ddim fp32 S={S}: CPU deviation x {bx / 4:.3e} pen {bp / 4:.3e}; bound x {bx:.3e} pen {bp:.3e}; GPU error x {ex:.3e} pen {ep:.3e}")
    assert torch.isfinite(got).all() and bx > 0 and bp > 0
    assert ex <= bx and ep <= bp
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, n:], torch.zeros((L - n, 3)))


@pytest.mark.parametrize("iters", [1, 3])
def test_fp32_inversion_matches_the_cpu_reference(iters):
    """As above for ``invert`` at S = 9 of the line the CPU reference sampled.  Measured on the CPU: iters = 1: deviation
    1.4e-05 (bound 5.8e-05); iters = 3: 1.4e-05 (5.8e-05).  GPU errors: DESIGN.md §23."""
    r = _ref()
    text, style = _gpu("text", "style")
    got = dhg_amd.invert(get_model("fp32"), r["x0"].cuda(), text, style, lengths=LENS, T=T, steps=9, iters=iters).cpu()
    bound = _invert_bound(iters)
    err = _dev(got, r["invert"][iters])
    print(f"invert fp32 S=9 iters={iters}: CPU deviation {bound / 4:.3e}; bound {bound:.3e}; GPU error {err:.3e}")
    assert torch.isfinite(got).all() and bound > 0
    assert err <= bound
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, n:], torch.zeros((L - n, 2)))


# ---------------------------------------------------------------- 4. bf16 tracks fp32
def test_bf16_tracks_fp32_at_four_steps():
    """The bf16 criterion of test_sampling_loop_matches_reference_golden, against the fp32 handle: err < 0.02 xmax, pen decisions
    flip only within 0.02 of 0.5 and in at most 2 % of the rows."""
    text, style, latent = _gpu("text", "style", "latent")
    ref = dhg_amd.sample_ddim(get_model("fp32"), text, style, T=T, steps=4, latent=latent, lengths=LENS).cpu().numpy()
    out = dhg_amd.sample_ddim(get_model("bf16"), text, style, T=T, steps=4, latent=latent, lengths=LENS).cpu().numpy()
    xmax = np.abs(ref[..., :2]).max()
    err = np.abs(out[..., :2] - ref[..., :2]).max()
    flipped = np.round(out[..., 2]).astype(np.uint8) != np.round(ref[..., 2]).astype(np.uint8)
    print(f"sample_ddim bf16 vs fp32 S=4: err {err:.3e}, xmax {xmax:.3f}, 0.02 xmax {0.02 * xmax:.3e}; pen flips {int(flipped.sum())} of {flipped.size}")
    assert np.isfinite(out).all()
    assert err < 0.02 * xmax
    assert np.all(np.abs(ref[..., 2][flipped] - 0.5) < 0.02)
    assert flipped.sum() <= 0.02 * flipped.size


# ---------------------------------------------------------------- 5. a ragged row is its alone run
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_ragged_rows_equal_their_alone_runs(prec):
    m = get_model(prec)
    text, style, strokes = _gpu("text", "style", "strokes")
    kw = dict(T=T, steps=4)
    rag, lat = dhg_amd.sample_ddim(m, text, style, L=L, lengths=LENS, seed=9, first_sample=3, return_latent=True, **kw)
    inv = dhg_amd.invert(m, strokes, text, style, lengths=LENS, iters=2, **kw)
    assert torch.isfinite(rag).all() and torch.isfinite(inv).all()
    for b, n in enumerate(LENS):
        alone, lat1 = dhg_amd.sample_ddim(m, text[b:b + 1], style[b:b + 1], L=n, seed=9, first_sample=3 + b, return_latent=True, **kw)
        assert torch.equal(rag[b, :n], alone[0]) and torch.equal(lat[b, :n], lat1[0]), b
        assert torch.equal(rag[b, n:], torch.zeros_like(rag[b, n:])) and torch.equal(lat[b, n:], torch.zeros_like(lat[b, n:]))
        inv1 = dhg_amd.invert(m, strokes[b:b + 1, :n].contiguous(), text[b:b + 1], style[b:b + 1], iters=2, **kw)
        assert torch.equal(inv[b, :n], inv1[0]) and torch.equal(inv[b, n:], torch.zeros_like(inv[b, n:])), b
    # rows past the lengths are never read: NaN there changes nothing
    dirty = strokes.clone()
    for b, n in enumerate(LENS):
        dirty[b, n:] = float("nan")
    assert torch.equal(dhg_amd.invert(m, dirty, text, style, lengths=LENS, iters=2, **kw), inv)
    dl = torch.where(torch.isnan(dirty[..., :2]), dirty[..., :2], lat)
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, latent=dl, lengths=LENS, **kw), rag)
    # every length == L: the call without lengths
    full = dhg_amd.sample_ddim(m, text, style, L=L, seed=9, first_sample=3, **kw)
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, L=L, lengths=[L] * B, seed=9, first_sample=3, **kw), full)
    assert torch.equal(dhg_amd.invert(m, strokes, text, style, lengths=[L] * B, **kw), dhg_amd.invert(m, strokes, text, style, **kw))


# ---------------------------------------------------------------- 6. the latent handed back
def test_latent_hand_back_and_determinism():
    m = get_model("bf16")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=T, steps=4, lengths=LENS)
    out, lat = dhg_amd.sample_ddim(m, text, style, seed=5, return_latent=True, **kw)
    again = dhg_amd.sample_ddim(m, text, style, latent=lat, seed=99, **{k: v for k, v in kw.items() if k != "L"})
    assert torch.isfinite(out).all() and torch.equal(out, again)
    out2, lat2 = dhg_amd.sample_ddim(m, text, style, seed=5, return_latent=True, **kw)
    assert torch.equal(out, out2) and torch.equal(lat, lat2)
    assert not torch.equal(dhg_amd.sample_ddim(m, text, style, seed=6, **kw), out)
    # another style under the same latent is another line; transfer is invert + sample_ddim
    style_to = torch.roll(style, 1, dims=0)
    tr = dhg_amd.transfer(out, text, style, style_to, m, lengths=LENS, T=T, steps=4, iters=2)
    want = dhg_amd.sample_ddim(m, text, style_to, latent=dhg_amd.invert(m, out, text, style, lengths=LENS, T=T, steps=4, iters=2), lengths=LENS, T=T, steps=4)
    assert torch.equal(tr, want) and not torch.equal(tr, out)


# ---------------------------------------------------------------- 7. round trip
def test_round_trip_reproduces_the_line():
    """sample_ddim(latent=invert(x0, iters=k)) against x0 on the fp32 handle at S = 9, k = 1 and 3; x0 is the line the CPU
    reference sampled.  The bound is the CPU reference's own round-trip error plus the sampler's bound of test 3 at S = 9.
    Measured on the CPU: k = 1: 4.6e-02; k = 3: 2.8e-05 (k = 3 is closer on these inputs, so the GPU is asserted to show the
    same order).  GPU figures: DESIGN.md §23."""
    r = _ref()
    m = get_model("fp32")
    text, style = _gpu("text", "style")
    x0 = r["x0"]
    gpu, cpu = {}, {}
    for k in (1, 3):
        lat = dhg_amd.invert(m, x0.cuda(), text, style, lengths=LENS, T=T, steps=9, iters=k)
        back = dhg_amd.sample_ddim(m, text, style, latent=lat, lengths=LENS, T=T, steps=9).cpu()
        gpu[k] = _dev(back[..., :2], x0[..., :2])
        cpu[k] = _dev(r["trip"][k][..., :2], x0[..., :2])
        bound = cpu[k] + _sample_bounds(9)[0]
        print(f"round trip fp32 S=9 iters={k}: CPU reference {cpu[k]:.3e}, bound {bound:.3e}, GPU {gpu[k]:.3e}")
        assert torch.isfinite(back).all()
        assert gpu[k] <= bound, (k, gpu[k], bound)
    if cpu[3] < cpu[1]:
        assert gpu[3] < gpu[1]


# ---------------------------------------------------------------- 8. the sampler is left alone
@pytest.mark.parametrize("lengths", [None, LENS])
def test_ddim_calls_leave_the_sampler_alone(lengths):
    m = fresh_model("bf16")
    text, style, strokes = _gpu("text", "style", "strokes")
    kw = dict(L=L, T=3, seed=7, first_sample=2, lengths=lengths)
    first = dhg_amd.sample(m, text, style, **kw).cpu()                 # captures the graph, sets the generator state
    d = dhg_amd.sample_ddim(m, text, style, L=L, T=T, steps=4, seed=1, lengths=lengths)
    inv = dhg_amd.invert(m, strokes, text, style, lengths=lengths, T=T, steps=2)
    again = dhg_amd.sample(m, text, style, **kw).cpu()                 # replays it
    assert torch.isfinite(first).all() and torch.isfinite(d).all() and torch.isfinite(inv).all() and torch.equal(first, again)


# ---------------------------------------------------------------- 9. errors at the C-ABI
def test_c_abi_rejects_bad_arguments_and_keeps_the_handle():
    m = get_model("bf16")
    text, style, strokes = _gpu("text", "style", "strokes")
    good = dhg_amd.sample_ddim(m, text, style, L=L, T=T, steps=4, seed=1, lengths=LENS)
    l, h = _lib.lib(), m._handle
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((B, L, 3), float("nan"), device="cuda")
    lat = torch.full((B, L, 2), float("nan"), device="cuda")
    pad = torch.zeros((B * L * 2 + 2,), device="cuda")

    def arr(v):
        return (C.c_int32 * max(1, len(v)))(*v)

    def smp(levels, T_=T, lens=LENS, latent=None, latent_out=None):
        rc = l.dhw_ddim_sample(h, text.data_ptr(), style.data_ptr(), B, L, Lt, arr(lens) if lens is not None else None, T_, arr(levels), len(levels),
                               latent, 1, 0, latent_out, out.data_ptr(), s)
        return rc, l.dhw_last_error(h).decode()

    def inv(levels, iters, T_=T, lens=LENS, latent_out=None):
        rc = l.dhw_ddim_invert(h, strokes.data_ptr(), text.data_ptr(), style.data_ptr(), B, L, Lt, arr(lens) if lens is not None else None, T_, arr(levels),
                               len(levels), iters, latent_out if latent_out is not None else lat.data_ptr(), s)
        return rc, l.dhw_last_error(h).decode()

    ok = [8, 5, 2, 0]
    cases = [(smp([5, 5, 2]), "strictly decreasing"), (smp([2, 5]), "levels[1] = 5 is not below levels[0] = 2"), (smp([T, 3]), "levels[0] = 9"),
             (smp([3, -1]), "levels[1] = -1"), (smp(list(range(2, -1, -1)), T_=2), "S = 3 must lie in [1, T = 2]"), (smp([]), "S = 0"),
             (smp(ok, latent=pad.data_ptr() + 4), "latent must be 8-byte aligned"), (smp(ok, latent_out=pad.data_ptr() + 4), "latent_out must be 8-byte aligned"),
             (smp(ok, lens=[24, 44, 40]), "lens[1] = 44"), (smp(ok, T_=0), "T = 0"),
             (inv(ok, 0), "iters = 0"), (inv(ok, 9), "iters = 9"), (inv([5, 5], 1), "strictly decreasing"), (inv(ok, 1, lens=[24, 72, 80]), "lens[2] = 80"),
             (inv(ok, 1, latent_out=pad.data_ptr() + 4), "latent_out must be 8-byte aligned"), (inv(list(range(2, -1, -1)), 1, T_=2), "S = 3")]
    for (rc, msg), what in cases:
        assert rc == -1 and what in msg and "dhw_ddim_" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(lat).all()   # nothing was launched
    rc, msg = smp(ok)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(out, good)   # the handle still works, and computes what it computed before
    rc, msg = inv(ok, 2)
    assert rc == 0, msg
    assert torch.equal(lat, dhg_amd.invert(m, strokes, text, style, lengths=LENS, T=T, steps=4, iters=2))


# ---------------------------------------------------------------- 10. a persistent-step handle
def test_persistent_step_handle_samples_deterministically(monkeypatch):
    monkeypatch.setenv("DHW_PERSIST", "1")
    m = fresh_model("bf16")
    text, style, strokes = _gpu("text", "style", "strokes")
    kw = dict(L=L, T=T, steps=4, seed=3, lengths=LENS)
    got = dhg_amd.sample_ddim(m, text, style, **kw)   # handle created under the switch
    inv = dhg_amd.invert(m, strokes, text, style, lengths=LENS, T=T, steps=4)
    monkeypatch.delenv("DHW_PERSIST")
    assert torch.equal(got, dhg_amd.sample_ddim(get_model("bf16"), text, style, **kw))
    assert torch.equal(inv, dhg_amd.invert(get_model("bf16"), strokes, text, style, lengths=LENS, T=T, steps=4))
