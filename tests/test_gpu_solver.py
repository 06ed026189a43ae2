"""Second-order multistep sampling (include/dhw.h dhw_dpm_coefs, dhw_dpm_update, dhw_dpm_sample, dhw_guided_dpm_sample;
``sample_ddim(order=2)``): runs on the MI355X only (-m gpu).

Shapes, as tests/test_gpu_ddim.py: B = 3, L = 72, Lt = 7 with one padded token, lens = [24, 72, 40], T = 9, S in {1, 2, 4, 9}; the
update kernel alone also at 5 x 104 = 520 rows (two full blocks and 8 rows).

What is bit for bit: the update kernel against numpy float32 with the table dhw_dpm_coefs wrote (both kinds, guided and not,
ragged, in place, hist); its first-order form against dhw_ddim_update and, guided, against dhw_guide_update(kind = 0); order 2 at S <= 2 against order 1; a ragged row against its alone run; a handed-back latent; a second
call on a handle against a fresh handle; ``sample`` and ``sample_ddim(order=1)`` before and after; a persistent-step handle.

What has a bound, and where it comes from.  The fp32 denoiser is within TOL["fp32"] of the CPU oracle at every call
(tests/test_gpu_parity.py).  The CPU reference (tests/solver_ref.py) is run twice on the test's inputs: plain, and with every eps
it gets moved by +-TOL["fp32"]["eps"] and every pen by +-TOL["fp32"]["pen"] (random sign per element, fixed seed).  The bound is
4x the largest deviation between the two runs: 4x because the GPU's error is within TOL at every call but correlated from call
to call, where the random signs partly cancel.  Every figure is printed before it is asserted; DESIGN.md §40 holds them.
bf16 against fp32 is test_gpu_ddim's rule: err < 0.02 xmax, pen decisions flip only within 0.02 of 0.5 and in at most 2 % of rows.
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
import guide_ref  # noqa: E402
import solver_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"fp32": dict(eps=2e-5, pen=2e-5), "bf16": dict(eps=2e-2, pen=5e-3)}   # test_gpu_parity.TOL
B, L, Lt, T = 3, 72, 7, 9
LENS = [24, 72, 40]
SCALE = 2.5
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
    """text [B,Lt] with one padded token, style, a latent ~ N(0,1) and the null condition: built once."""
    if "inputs" not in _CACHE:
        inp = spec.synthetic_inputs(B, L, Lt, seed=61, pad=1, T=1)
        g = torch.Generator().manual_seed(62)
        utext, ustyle = dhg_amd.null_condition(B, Lt)
        _CACHE["inputs"] = dict(text=torch.from_numpy(inp["text"]), style=torch.from_numpy(inp["style"]), latent=torch.randn((B, L, 2), generator=g),
                                utext=utext, ustyle=ustyle)
        assert (_CACHE["inputs"]["text"] == 0).sum() >= 1
    return _CACHE["inputs"]


def _gpu(*names):
    i = _inputs()
    return [i[n].cuda() for n in names]


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _masked(x, lens):
    x = np.array(x, np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


def _dev(a, b):
    return (a - b).abs().max().item()


# ---------------------------------------------------------------- 1. the update kernel alone, against numpy
def _table(levels, order):
    """[S, 9] float32: the table the library uses."""
    S = len(levels)
    out = (C.c_float * (9 * S))()
    rc = _lib.lib().dhw_dpm_coefs(T, (C.c_int32 * S)(*levels), S, order, out)
    assert rc == 0, _lib.lib().dhw_last_error(None).decode()
    return np.array(out, np.float32).reshape(S, 9)


def np_step(base, e, hist, row):
    """-> (x', x0) in numpy float32, each operation rounded on its own: nine for kind 2, U's five (x0: its first three) for kind 1."""
    kind, c0, c1, c2, c3, k0, k1, c4, c5 = (np.float32(v) for v in row)
    with np.errstate(all="ignore"):
        m = c1 * e
        d = base - m
        x0 = d / c0
        if kind == 2:
            p = k0 * x0
            q = k1 * hist
            D = p - q
            s = c4 * base
            n = c5 * D
            out = s + n
        else:
            out = c2 * x0 + c3 * e
    assert out.dtype == np.float32 and x0.dtype == np.float32
    return out, x0


def np_combine(ec, eu, w):
    w = np.asarray(w, np.float32).reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        e = ec + (w - np.float32(1)) * (ec - eu)
    return np.where(w == 0, eu, e)


def _raw(base, eps, hist, row, out, lens_dev=None, scale=None, pen=None, out3=None):
    Bq, Lq = hist.shape[:2]
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = _lib.lib().dhw_dpm_update(base.data_ptr(), eps.data_ptr(), p(pen), p(lens_dev), p(scale), hist.data_ptr(), Bq, Lq, (C.c_float * 9)(*map(float, row)),
                                   p(out), p(out3), _st())
    assert rc == 0, _lib.lib().dhw_last_error(None).decode()
    torch.cuda.synchronize()


CANARY = 12345.5


def _with_canary(x, rows_behind):
    """x on the device with `rows_behind` canary rows behind it in the same allocation -> (the view of x, the canary view)."""
    tail = torch.full((rows_behind,) + tuple(x.shape[1:]), CANARY)
    buf = torch.cat((x, tail)).cuda()
    return buf[:x.shape[0]], buf[x.shape[0]:]


@pytest.mark.parametrize("shape", [(B, L, LENS), (5, 104, [104, 40, 104, 8, 96])])
def test_second_order_update_matches_numpy_bit_for_bit(shape):
    """216 rows (one block, partial) and 520 rows (two full blocks and 8 rows)."""
    Bq, Lq, lens = shape
    g = torch.Generator().manual_seed(163 + Bq)
    base, eps, hist = torch.randn((Bq, Lq, 2), generator=g) * 3, torch.randn((Bq, Lq, 2), generator=g), torch.randn((Bq, Lq, 2), generator=g)
    base[0, 0, 0], eps[0, 0, 1], hist[0, 1, 0] = 0.0, 0.0, 0.0
    base[1, 5, 1], eps[1, 5, 1], hist[1, 5, 1] = 1e-38, 0.0, 0.0           # a subnormal carried through: x0 = 1e-38 / A, s = c4 * 1e-38
    hist[1, 6, 0], eps[1, 6, 0], base[1, 6, 0] = 1e-38, 0.0, 0.0           # ... and through the history term
    tab = np.concatenate((_table(dhg_amd.ddim_levels(T, 4), 2), _table(dhg_amd.ddim_levels(T, 9), 2), _table([8, 7, 3, 1, 0], 2)))
    rows = [r for r in tab if r[0] == 2.0]
    assert len(rows) == 2 + 7 + 3
    rows.append(np.array([2.0, 3.0, 0.1, 0.5, 0.5, 1.0 + 1.0 / 3, 1.0 / 3, 0.7, 0.3], np.float32))   # a divisor that is no power of two, odd factors
    lens_dev = torch.tensor(lens, dtype=torch.int32).cuda()
    bn, en, hn = base.numpy(), eps.numpy(), hist.numpy()
    for row in rows:
        want, want_x0 = np_step(bn, en, hn, row)
        assert np.isfinite(want).all() and want[1, 5, 1] != 0
        out, out_c = _with_canary(torch.full((Bq, Lq, 2), float("nan")), Bq)
        hd, hd_c = _with_canary(hist, Bq)
        _raw(base.cuda(), eps.cuda(), hd, row, out)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), row
        assert np.array_equal(_bits(hd.cpu().numpy()), _bits(want_x0)), row                    # hist afterwards holds x0's bits
        assert bool((out_c == CANARY).all()) and bool((hd_c == CANARY).all())                   # nothing behind out or hist
        # ragged, with NaN where nothing may be read: identical valid rows, 0 past the lengths in out and hist
        bd, ed, hh = base.clone(), eps.clone(), hist.clone()
        for b, n in enumerate(lens):
            bd[b, n:], ed[b, n:], hh[b, n:] = float("nan"), float("nan"), float("nan")
        out, out_c = _with_canary(torch.full((Bq, Lq, 2), float("nan")), Bq)
        hd, hd_c = _with_canary(hh, Bq)
        _raw(bd.cuda(), ed.cuda(), hd, row, out, lens_dev)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(_masked(want, lens))), row
        assert np.array_equal(_bits(hd.cpu().numpy()), _bits(_masked(want_x0, lens))), row
        assert bool((out_c == CANARY).all()) and bool((hd_c == CANARY).all())
    # in place (out = base), as the sampling loop uses it, with the pen row of a last step
    row = rows[0]
    want, want_x0 = np_step(bn, en, hn, row)
    pen = torch.rand((Bq, Lq), generator=g)
    x, hd, out3 = base.cuda(), hist.cuda(), torch.full((Bq, Lq, 3), float("nan")).cuda()
    _raw(x, eps.cuda(), hd, row, x, lens_dev, pen=pen.cuda(), out3=out3)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(_masked(want, lens))) and np.array_equal(_bits(hd.cpu().numpy()), _bits(_masked(want_x0, lens)))
    got3 = out3.cpu().numpy()
    assert np.array_equal(_bits(got3[..., :2]), _bits(_masked(want, lens))) and np.array_equal(_bits(got3[..., 2]), _bits(_masked(pen.numpy(), lens)))


@pytest.mark.parametrize("lens", [None, [104, 40, 104, 8, 96]])
def test_first_order_update_is_the_ddim_update_and_writes_hist(lens):
    """A kind-1 row: out equals dhw_ddim_update on the same inputs bit for bit, hist receives x0, and a hist full of NaN on entry
    changes nothing (a first-order step never reads it)."""
    Bq, Lq = 5, 104
    g = torch.Generator().manual_seed(36)
    base, eps = torch.randn((Bq, Lq, 2), generator=g) * 3, torch.randn((Bq, Lq, 2), generator=g)
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    tab = _table(dhg_amd.ddim_levels(T, 4), 2)
    assert list(tab[:, 0]) == [1.0, 2.0, 2.0, 1.0]
    for row in (tab[0], tab[3], _table(dhg_amd.ddim_levels(T, 4), 1)[1], np.array([1.0, 3.0, 0.1, 1.0 / 3, 0.7, 0, 0, 0, 0], np.float32)):
        bd, ed, plain = base.cuda(), eps.cuda(), torch.full((Bq, Lq, 2), float("nan")).cuda()
        rc = _lib.lib().dhw_ddim_update(bd.data_ptr(), ed.data_ptr(), None if lens is None else lens_dev.data_ptr(), Bq, Lq, float(row[1]), float(row[2]),
                                        float(row[3]), float(row[4]), plain.data_ptr(), _st())
        assert rc == 0, _lib.lib().dhw_last_error(None).decode()
        out, out_c = _with_canary(torch.full((Bq, Lq, 2), float("nan")), Bq)
        hd, hd_c = _with_canary(torch.full((Bq, Lq, 2), float("nan")), Bq)
        _raw(bd, ed, hd, row, out, lens_dev)
        want, want_x0 = np_step(base.numpy(), eps.numpy(), None, row)
        if lens is not None:
            want, want_x0 = _masked(want, lens), _masked(want_x0, lens)
        got = out.cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(plain.cpu().numpy())), row
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(hd.cpu().numpy()), _bits(want_x0)), row
        assert bool((out_c == CANARY).all()) and bool((hd_c == CANARY).all())


@pytest.mark.parametrize("lens", [None, [104, 40, 104, 8, 96]])
@pytest.mark.parametrize("kind", [1, 2])
def test_guided_update_on_equal_halves_is_the_plain_update(kind, lens):
    """The guided form with both eps halves the same array equals the unguided form on that array bit for bit at every scale (the
    difference is exactly +0, the product a zero, e + (a zero) = e for e != 0; scale 0 selects the equal half), both halves of out
    are written, hist is one half.  Then two different halves against numpy's combine."""
    Bq, Lq = 5, 104
    g = torch.Generator().manual_seed(37 + kind)
    base, e, hist = torch.randn((Bq, Lq, 2), generator=g) * 3, torch.randn((Bq, Lq, 2), generator=g), torch.randn((Bq, Lq, 2), generator=g)
    e_u = torch.randn((Bq, Lq, 2), generator=g)
    assert bool((e != 0).all())
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    scales = [0.0, 1.0, SCALE, 0.0, 1.0] if kind == 1 else [SCALE, 0.0, 1.0, 4.0, 0.25]
    scale = torch.tensor(scales).cuda()
    row = _table(dhg_amd.ddim_levels(T, 4), 2)[0 if kind == 1 else 2]
    assert row[0] == kind
    plain, hp = torch.full((Bq, Lq, 2), float("nan")).cuda(), hist.cuda()
    _raw(base.cuda(), e.cuda(), hp, row, plain, lens_dev)
    out, out_c = _with_canary(torch.full((2 * Bq, Lq, 2), float("nan")), Bq)
    hd, hd_c = _with_canary(hist, Bq)
    _raw(base.cuda(), torch.cat((e, e)).cuda(), hd, row, out, lens_dev, scale=scale)
    got, want = out.cpu().numpy(), plain.cpu().numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(got[:Bq]), _bits(want)) and np.array_equal(_bits(got[Bq:]), _bits(want))
    assert np.array_equal(_bits(hd.cpu().numpy()), _bits(hp.cpu().numpy()))
    assert bool((out_c == CANARY).all()) and bool((hd_c == CANARY).all())
    for b, n in enumerate(lens or []):
        assert not _bits(got[b, n:]).any() and not _bits(got[Bq + b, n:]).any(), b
    # two different halves, in place on the doubled state
    comb = np_combine(e.numpy(), e_u.numpy(), scales)
    want, want_x0 = np_step(base.numpy(), comb, hist.numpy(), row)
    if lens is not None:
        want, want_x0 = _masked(want, lens), _masked(want_x0, lens)
    x, hd = torch.cat((base, torch.full((Bq, Lq, 2), float("nan")))).cuda(), hist.cuda()
    _raw(x, torch.cat((e, e_u)).cuda(), hd, row, x, lens_dev, scale=scale)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.concatenate((want, want)))) and np.array_equal(_bits(hd.cpu().numpy()), _bits(want_x0))


@pytest.mark.parametrize("lens", [None, [104, 40, 104, 8, 96]])
def test_guided_first_order_update_is_the_guided_ddim_update(lens):
    """A kind-1 row with a scale, on two DIFFERENT eps halves: out equals dhw_guide_update(kind = 0) on the same inputs bit for bit
    in both halves (the two are one kernel template, apart in a template argument: DESIGN.md §41); hist receives the bits of
    x0 = (base - c1 e) / c0 with e numpy's fp32 combine, 0 past a length.  520 rows: two full blocks and 8 rows; the lengths cut
    inside blocks, with NaN behind them in base, eps and hist; hist is NaN throughout on entry (a first-order step never reads it)."""
    Bq, Lq = 5, 104
    g = torch.Generator().manual_seed(41)
    base, e, e_u = torch.randn((Bq, Lq, 2), generator=g) * 3, torch.randn((Bq, Lq, 2), generator=g), torch.randn((Bq, Lq, 2), generator=g)
    assert bool((e != e_u).all())
    scales = [0.0, 1.0, SCALE, 4.0, 0.25]
    scale = torch.tensor(scales).cuda()
    comb = np_combine(e.numpy(), e_u.numpy(), scales)
    bd, ed, ud = base.clone(), e.clone(), e_u.clone()
    for b, n in enumerate(lens or []):
        bd[b, n:], ed[b, n:], ud[b, n:] = float("nan"), float("nan"), float("nan")
    bd, eps2 = bd.cuda(), torch.cat((ed, ud)).cuda()
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    tab = _table(dhg_amd.ddim_levels(T, 4), 2)
    for row in (tab[0], tab[3], np.array([1.0, 3.0, 0.1, 1.0 / 3, 0.7, 0, 0, 0, 0], np.float32)):
        assert row[0] == 1.0
        plain = torch.full((2 * Bq, Lq, 2), float("nan")).cuda()
        rc = _lib.lib().dhw_guide_update(0, bd.data_ptr(), eps2.data_ptr(), None, None if lens is None else lens_dev.data_ptr(), scale.data_ptr(), None, Bq, Lq,
                                         float(row[1]), float(row[2]), float(row[3]), float(row[4]), plain.data_ptr(), None, _st())
        assert rc == 0, _lib.lib().dhw_last_error(None).decode()
        out, out_c = _with_canary(torch.full((2 * Bq, Lq, 2), float("nan")), Bq)
        hd, hd_c = _with_canary(torch.full((Bq, Lq, 2), float("nan")), Bq)
        _raw(bd, eps2, hd, row, out, lens_dev, scale=scale)
        got, want = out.cpu().numpy(), plain.cpu().numpy()
        want_x0 = np_step(base.numpy(), comb, None, row)[1]
        assert np.isfinite(want).all() and not np.array_equal(_bits(want[:Bq]), _bits(np_step(base.numpy(), e.numpy(), None, row)[0]))   # (the halves differ: the combine acts)
        assert np.array_equal(_bits(got[:Bq]), _bits(want[:Bq])) and np.array_equal(_bits(got[Bq:]), _bits(want[Bq:])), row
        assert np.array_equal(_bits(got[Bq:]), _bits(got[:Bq])), row
        assert np.array_equal(_bits(hd.cpu().numpy()), _bits(want_x0 if lens is None else _masked(want_x0, lens))), row
        for b, n in enumerate(lens or []):
            assert not _bits(got[b, n:]).any() and not _bits(got[Bq + b, n:]).any(), b
        assert bool((out_c == CANARY).all()) and bool((hd_c == CANARY).all())


# ---------------------------------------------------------------- 2. the sampling entries, bit for bit
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("guidance", [None, SCALE])
def test_order_two_at_one_and_two_levels_is_order_one(prec, guidance):
    m = get_model(prec)
    text, style, latent = _gpu("text", "style", "latent")
    g = {} if guidance is None else dict(guidance=guidance)
    for S in (1, 2):
        kw = dict(T=T, steps=S, latent=latent, lengths=LENS, **g)
        one = dhg_amd.sample_ddim(m, text, style, **kw)
        assert torch.isfinite(one).all()
        assert torch.equal(dhg_amd.sample_ddim(m, text, style, order=2, **kw), one), S
        assert torch.equal(dhg_amd.sample_ddim(m, text, style, order=1, **kw), one), S
    # ... and differs from it as soon as there is a second-order step
    kw = dict(T=T, steps=4, latent=latent, lengths=LENS, **g)
    assert not torch.equal(dhg_amd.sample_ddim(m, text, style, order=2, **kw), dhg_amd.sample_ddim(m, text, style, **kw))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("guidance", [None, [0.0, SCALE, 1.0]])
def test_ragged_rows_equal_their_alone_runs(prec, guidance):
    m = get_model(prec)
    text, style = _gpu("text", "style")
    kw = dict(T=T, steps=4, order=2, seed=9)
    gb = (lambda b: {}) if guidance is None else (lambda b: dict(guidance=guidance[b]))
    g = {} if guidance is None else dict(guidance=guidance)
    rag, lat = dhg_amd.sample_ddim(m, text, style, L=L, lengths=LENS, first_sample=3, return_latent=True, **kw, **g)
    assert torch.isfinite(rag).all()
    for b, n in enumerate(LENS):
        alone, lat1 = dhg_amd.sample_ddim(m, text[b:b + 1], style[b:b + 1], L=n, first_sample=3 + b, return_latent=True, **kw, **gb(b))
        assert torch.equal(rag[b, :n], alone[0]) and torch.equal(lat[b, :n], lat1[0]), b
        assert torch.equal(rag[b, n:], torch.zeros_like(rag[b, n:])) and torch.equal(lat[b, n:], torch.zeros_like(lat[b, n:]))
    # rows past the lengths are never read: NaN there changes nothing
    dl = lat.clone()
    for b, n in enumerate(LENS):
        dl[b, n:] = float("nan")
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, latent=dl, lengths=LENS, T=T, steps=4, order=2, **g), rag)
    # every length == L: the call without lengths
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, L=L, lengths=[L] * B, **kw, **g), dhg_amd.sample_ddim(m, text, style, L=L, **kw, **g))


def test_latent_hand_back_and_no_stale_history():
    m = get_model("bf16")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=T, steps=4, lengths=LENS, order=2)
    out, lat = dhg_amd.sample_ddim(m, text, style, seed=5, return_latent=True, **kw)
    again = dhg_amd.sample_ddim(m, text, style, latent=lat, seed=99, **{k: v for k, v in kw.items() if k != "L"})
    assert torch.isfinite(out).all() and torch.equal(out, again)
    assert not torch.equal(dhg_amd.sample_ddim(m, text, style, seed=6, **kw), out)
    # a call behind a call with other inputs (other seed, lengths and scale: hist holds that call's last x0 in every row) equals
    # the same call on a fresh model
    dhg_amd.sample_ddim(m, torch.roll(text, 1, 0), torch.roll(style, 1, 0), seed=77, L=L, T=T, steps=9, order=2, guidance=4.0)
    second = dhg_amd.sample_ddim(m, text, style, seed=5, **kw)
    fresh = dhg_amd.sample_ddim(fresh_model("bf16"), text, style, seed=5, **kw)
    assert torch.equal(second, fresh) and torch.equal(second, out)
    guided = dhg_amd.sample_ddim(m, text, style, seed=5, guidance=SCALE, **kw)
    assert torch.equal(guided, dhg_amd.sample_ddim(fresh_model("bf16"), text, style, seed=5, guidance=SCALE, **kw)) and not torch.equal(guided, out)


@pytest.mark.parametrize("lengths", [None, LENS])
def test_order_two_calls_leave_the_other_samplers_alone(lengths):
    m = fresh_model("bf16")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=3, seed=7, first_sample=2, lengths=lengths)
    dk = dict(L=L, T=T, steps=4, seed=1, lengths=lengths)
    first = dhg_amd.sample(m, text, style, **kw).cpu()                 # captures the graph, sets the generator state
    d1 = dhg_amd.sample_ddim(m, text, style, order=1, **dk)
    d1g = dhg_amd.sample_ddim(m, text, style, guidance=SCALE, **dk)
    d2 = dhg_amd.sample_ddim(m, text, style, order=2, **dk)
    d2g = dhg_amd.sample_ddim(m, text, style, order=2, guidance=SCALE, **dk)
    again = dhg_amd.sample(m, text, style, **kw).cpu()                 # replays it
    assert all(torch.isfinite(t).all() for t in (first, d1, d1g, d2, d2g)) and torch.equal(first, again)
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, order=1, **dk), d1) and torch.equal(dhg_amd.sample_ddim(m, text, style, **dk), d1)
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, guidance=SCALE, **dk), d1g)
    assert torch.equal(d1, dhg_amd.sample_ddim(get_model("bf16"), text, style, **dk))


def test_persistent_step_handle_samples_deterministically(monkeypatch):
    monkeypatch.setenv("DHW_PERSIST", "1")
    m = fresh_model("bf16")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=T, steps=4, seed=3, lengths=LENS, order=2)
    got = dhg_amd.sample_ddim(m, text, style, **kw)   # handle created under the switch
    gotg = dhg_amd.sample_ddim(m, text, style, guidance=SCALE, **kw)
    monkeypatch.delenv("DHW_PERSIST")
    assert torch.isfinite(got).all() and torch.equal(got, dhg_amd.sample_ddim(get_model("bf16"), text, style, **kw))
    assert torch.equal(gotg, dhg_amd.sample_ddim(get_model("bf16"), text, style, guidance=SCALE, **kw))


def test_c_abi_rejects_bad_arguments_and_keeps_the_handle():
    m = get_model("bf16")
    text, style = _gpu("text", "style")
    good = dhg_amd.sample_ddim(m, text, style, L=L, T=T, steps=4, seed=1, lengths=LENS, order=2)
    l, h = _lib.lib(), m._handle
    out = torch.full((B, L, 3), float("nan"), device="cuda")
    pad = torch.zeros((B * L * 2 + 2,), device="cuda")

    def arr(v):
        return (C.c_int32 * max(1, len(v)))(*v)

    def smp(levels, order, T_=T, lens=LENS, latent=None, latent_out=None):
        rc = l.dhw_dpm_sample(h, text.data_ptr(), style.data_ptr(), B, L, Lt, arr(lens) if lens is not None else None, T_, arr(levels), len(levels), order,
                              latent, 1, 0, latent_out, out.data_ptr(), _st())
        return rc, l.dhw_last_error(h).decode()

    ok = [8, 5, 2, 0]
    for (rc, msg), what in (((smp(ok, 0)), "order = 0"), (smp(ok, 3), "order = 3"), (smp(ok, -1), "order = -1"), (smp([5, 5, 2], 2), "strictly decreasing"),
                            (smp([], 2), "S = 0"), (smp(ok, 2, T_=0), "T = 0"), (smp(ok, 2, lens=[24, 44, 40]), "lens[1] = 44"),
                            (smp(ok, 2, latent=pad.data_ptr() + 4), "latent must be 8-byte aligned"),
                            (smp(ok, 2, latent_out=pad.data_ptr() + 4), "latent_out must be 8-byte aligned")):
        assert rc == -1 and what in msg and "dhw_dpm_sample" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()   # nothing was launched
    rc, msg = smp(ok, 2)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(out, good)   # the handle still works, and computes what it computed before


# ---------------------------------------------------------------- 3. fp32 against the CPU reference; bf16 against fp32
def _ref(S, guided, perturbed):
    """tests/solver_ref.py on the shared inputs at order 2, once per configuration."""
    key = ("ref", S, guided, perturbed)
    if key not in _CACHE:
        i, sd = _inputs(), _sd()
        pert = ddim_ref.sign_perturb(TOL["fp32"]["eps"], TOL["fp32"]["pen"], 170 + S + (50 if guided else 0)) if perturbed else None
        lv = dhg_amd.ddim_levels(T, S)
        abar = _lib.schedule(T)[1]
        out = torch.zeros((B, L, 3))
        for b, n in enumerate(LENS):   # each sample alone: the guided forward closes over its own guidance condition
            if guided:
                f = guide_ref.guided_forward(ref_cpu.forward, i["utext"][b:b + 1], i["ustyle"][b:b + 1], torch.tensor([SCALE]), pert)
                out[b, :n] = solver_ref.sample(f, sd, i["text"][b:b + 1], i["style"][b:b + 1], lv, T, i["latent"][b:b + 1, :n], order=2, abar=abar)[0]
            else:
                out[b, :n] = solver_ref.sample(ref_cpu.forward, sd, i["text"][b:b + 1], i["style"][b:b + 1], lv, T, i["latent"][b:b + 1, :n], order=2,
                                               perturb=pert, abar=abar)[0]
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("S", [4, 9])
@pytest.mark.parametrize("guided", [False, True])
def test_fp32_sampling_matches_the_cpu_reference(S, guided):
    """Bound = 4x the deviation of the CPU reference under a +-TOL["fp32"] perturbation of every denoiser output (module
    docstring).  The measured CPU deviations, bounds and GPU errors are the table in DESIGN.md §40."""
    want, pert = _ref(S, guided, False), _ref(S, guided, True)
    text, style, latent = _gpu("text", "style", "latent")
    g = dict(guidance=SCALE) if guided else {}
    got = dhg_amd.sample_ddim(get_model("fp32"), text, style, T=T, steps=S, latent=latent, lengths=LENS, order=2, **g).cpu()
    bx, bp = 4 * _dev(want[..., :2], pert[..., :2]), 4 * _dev(want[..., 2], pert[..., 2])
    ex, ep = _dev(got[..., :2], want[..., :2]), _dev(got[..., 2], want[..., 2])
    print(f"sample_ddim order 2 fp32 S={S} {'guided 2.5' if guided else 'unguided'}: CPU deviation x {bx / 4:.3e} pen {bp / 4:.3e}; "
          f"bound x {bx:.3e} pen {bp:.3e}; GPU error x {ex:.3e} pen {ep:.3e}; max|x| {want[..., :2].abs().max().item():.2f}")
    assert torch.isfinite(got).all() and bx > 0 and bp > 0
    assert ex <= bx and ep <= bp
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, n:], torch.zeros((L - n, 3)))


def test_bf16_tracks_fp32_at_four_steps():
    """The bf16 criterion of tests/test_gpu_ddim.py, against the fp32 handle: err < 0.02 xmax, pen decisions flip only within 0.02
    of 0.5 and in at most 2 % of the rows."""
    text, style, latent = _gpu("text", "style", "latent")
    kw = dict(T=T, steps=4, latent=latent, lengths=LENS, order=2)
    ref = dhg_amd.sample_ddim(get_model("fp32"), text, style, **kw).cpu().numpy()
    out = dhg_amd.sample_ddim(get_model("bf16"), text, style, **kw).cpu().numpy()
    xmax = np.abs(ref[..., :2]).max()
    err = np.abs(out[..., :2] - ref[..., :2]).max()
    flipped = np.round(out[..., 2]).astype(np.uint8) != np.round(ref[..., 2]).astype(np.uint8)
    print(f"sample_ddim order 2 bf16 vs fp32 S=4: err {err:.3e}, xmax {xmax:.3f}, 0.02 xmax {0.02 * xmax:.3e}; pen flips {int(flipped.sum())} of {flipped.size}")
    assert np.isfinite(out).all()
    assert err < 0.02 * xmax
    assert np.all(np.abs(ref[..., 2][flipped] - 0.5) < 0.02)
    assert flipped.sum() <= 0.02 * flipped.size
