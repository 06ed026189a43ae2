"""Classifier-free guidance (include/dhw.h dhw_guided_ddim_sample, dhw_guided_sample, dhw_guide_update; include/dhw_train.h
dhw_train_cond_drop; ``sample(..., guidance=)``, ``sample_ddim(..., guidance=)``, ``GraphedTrainStep(cond_drop=)``): runs on the
MI355X only (-m gpu).

Shapes (test_gpu_ddim.py's): B = 3 (6 forward rows), L = 72, Lt = 7 with one padded token, lens = [24, 72, 40], T = 9,
S in {1, 4, 9}, max_B = 8.

What is bit for bit (value-equal where a -0 may become +0): the step kernel against numpy float32 for its three kinds; scale 1
against plain ``sample_ddim`` (on the 6-row batch and at B = 3); scale 0 against the plain call under the guidance condition;
a ragged row against its alone run; a mixed-scale row against the uniform call; a handed-back latent; ``sample`` before and
after a guided call; a persistent-step handle; the dropout kernel against its numpy statement; a step with cond_drop = 1
against a host-fed step given the null batch (inputs; the losses to the 2e-6 of test_gpu_resident.py).

What has a bound, and where it comes from.  The fp32 denoiser is within TOL["fp32"] of the CPU oracle at every call
(tests/test_gpu_parity.py).  The CPU reference (tests/guide_ref.py) is run twice on the test's inputs: plain, and with every eps
and pen of BOTH branches moved by +-TOL (random sign per element, fixed seed).  The bound is 4x the largest deviation between
the two runs (DESIGN.md §23's method: the GPU's error is within TOL at every call but correlated from call to call, where the
random signs partly cancel).  The bf16 handle is held against the fp32 handle with the same construction at TOL["bf16"].  Every
figure is printed before it is asserted.

Measured on the CPU reference with these inputs, scale 2.5, |x| up to 6.6 (deviation x / pen; the bounds are 4x); the GPU's
errors are in DESIGN.md §33:
    TOL fp32   ddim S = 4: 9.5e-05 / 2.2e-05    ddim S = 9: 7.5e-05 / 2.2e-05    new: 2.1e-04 / 2.4e-05    standard: 1.3e-04 / 2.2e-05
    TOL bf16   ddim S = 4: 9.4e-02 / 7.2e-03    ddim S = 9: 7.5e-02 / 6.8e-03    new: 2.1e-01 / 9.5e-03    standard: 1.3e-01 / 7.4e-03
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec, train, train_model as tm
from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

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
    """text [B,Lt] with one padded token, style, a latent ~ N(0,1), noise [T+1,B,L,2] and the null condition: built once."""
    if "inputs" not in _CACHE:
        inp = spec.synthetic_inputs(B, L, Lt, seed=61, pad=1, T=T)
        g = torch.Generator().manual_seed(62)
        utext, ustyle = dhg_amd.null_condition(B, Lt)
        _CACHE["inputs"] = dict(text=torch.from_numpy(inp["text"]), style=torch.from_numpy(inp["style"]), latent=torch.randn((B, L, 2), generator=g),
                                noise=torch.from_numpy(inp["noise"]), utext=utext, ustyle=ustyle)
        assert (_CACHE["inputs"]["text"] == 0).sum() >= 1
    return _CACHE["inputs"]


def _gpu(*names):
    i = _inputs()
    return [i[n].cuda() for n in names]


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _veq(a, b):
    """Equal as values (numpy.array_equal: -0 == +0), and finite."""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return bool(np.isfinite(a).all()) and np.array_equal(a, b)


def _dev(a, b):
    return (a - b).abs().max().item()


# ---------------------------------------------------------------- 1. the step kernel alone, against numpy
def np_combine(ec, eu, w):
    w = np.asarray(w, np.float32).reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        e = ec + (w - np.float32(1)) * (ec - eu)
    assert e.dtype == np.float32
    return np.where(w == 0, eu, e)


def np_step(kind, base, e, z, c):
    """The three updates in numpy float32, each operation rounded on its own; z None: no noise term."""
    c0, c1, c2, c3 = (np.float32(v) for v in c)
    with np.errstate(all="ignore"):
        if kind == 0:
            out = c2 * ((base - c1 * e) / c0) + c3 * e
        elif kind == 1:
            out = (base - c0 * e) / c1
            if z is not None:
                out = out + z * c2
        else:
            out = c1 * (base - (c3 * e) / c0)
            if z is not None:
                out = out + c2 * z
    assert out.dtype == np.float32
    return out


def _masked(x, lens):
    x = np.array(x, np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


def _raw(kind, base, eps2, pen, lens_dev, scale, z, c, out, out3):
    Bq, Lq = eps2.shape[0] // 2, eps2.shape[1]
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = _lib.lib().dhw_guide_update(kind, base.data_ptr(), eps2.data_ptr(), p(pen), p(lens_dev), scale.data_ptr(), p(z), Bq, Lq, float(c[0]), float(c[1]),
                                     float(c[2]), float(c[3]), p(out), p(out3), _st())
    assert rc == 0, _lib.lib().dhw_last_error(None).decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_step_kernel_matches_numpy_bit_for_bit(kind):
    g = torch.Generator().manual_seed(63 + kind)
    base, eps2 = torch.randn((B, L, 2), generator=g) * 3, torch.randn((2 * B, L, 2), generator=g)
    pen, z = torch.rand((B, L), generator=g), torch.randn((B, L, 2), generator=g)
    base[0, 0, 0], eps2[0, 0, 1], eps2[B, 0, 1] = 0.0, 0.0, 0.0
    base[1, 5, 1], eps2[1, 5, 1], eps2[B + 1, 5, 1] = 1e-38, 0.0, 0.0                     # a subnormal carried through every operation
    eps2[2, 3, 0], eps2[B + 2, 3, 0] = 1e-38, 3e-39                                       # ... and through the combine
    abar = _lib.schedule(T)[1]
    beta = _lib.schedule(T)[0]
    one = np.float32(1)
    sets = [(np.sqrt(abar[5]), np.sqrt(one - abar[5]), np.sqrt(abar[2]), np.sqrt(one - abar[2])), (np.sqrt(abar[0]), np.sqrt(one - abar[0]), one, np.float32(0)),
            (np.sqrt(one - abar[4]), np.sqrt(one - beta[4]), np.sqrt(one - abar[3]), np.float32(0)),
            (np.sqrt(one - abar[4]), one / np.sqrt(one - beta[4]), np.sqrt(beta[4]), beta[4]), (np.float32(3.0), np.float32(0.1), np.float32(1.0 / 3), np.float32(0.7))]
    lens_dev = torch.tensor(LENS, dtype=torch.int32).cuda()
    bn, en, zn = base.numpy(), eps2.numpy(), z.numpy()
    for scale in ([0.0] * B, [1.0] * B, [SCALE] * B, [0.0, 1.0, SCALE], [64.0, 0.5, 7.25]):
        sc = torch.tensor(scale).cuda()
        e = np_combine(en[:B], en[B:], scale)
        if scale[0] == 1.0:
            assert np.array_equal(e[0], en[0])
        if scale[0] == 0.0:
            assert np.array_equal(_bits(e[0]), _bits(en[B]))
        for c in sets:
            for zz in ([None] if kind == 0 else [None, z]):
                want = np_step(kind, bn, e, None if zz is None else zn, c)
                out, out3 = torch.full((2 * B, L, 2), float("nan")).cuda(), torch.full((B, L, 3), float("nan")).cuda()
                _raw(kind, base.cuda(), eps2.cuda(), pen.cuda(), None, sc, None if zz is None else zz.cuda(), c, out, out3)
                got, got3 = out.cpu().numpy(), out3.cpu().numpy()
                assert np.array_equal(_bits(got[:B]), _bits(want)) and np.array_equal(_bits(got[B:]), _bits(want)), (scale, c)
                assert np.array_equal(_bits(got3[..., :2]), _bits(want)) and np.array_equal(_bits(got3[..., 2]), _bits(pen.numpy())), (scale, c)
        # ragged, with NaN where nothing may be read: identical valid rows, 0 past the lengths in both halves and in out3
        c = sets[kind if kind else 0]
        bd, ed, pd, zd = base.clone(), eps2.clone(), pen.clone(), z.clone()
        for b, n in enumerate(LENS):
            bd[b, n:], ed[b, n:], ed[B + b, n:], pd[b, n:], zd[b, n:] = (float("nan"),) * 5
        out, out3 = torch.full((2 * B, L, 2), float("nan")).cuda(), torch.full((B, L, 3), float("nan")).cuda()
        _raw(kind, bd.cuda(), ed.cuda(), pd.cuda(), lens_dev, sc, zd.cuda() if kind else None, c, out, out3)
        want = _masked(np_step(kind, bn, e, zn if kind else None, c), LENS)
        got, got3 = out.cpu().numpy(), out3.cpu().numpy()
        assert np.array_equal(_bits(got[:B]), _bits(want)) and np.array_equal(_bits(got[B:]), _bits(want)), scale
        assert np.array_equal(_bits(got3[..., :2]), _bits(want)) and np.array_equal(_bits(got3[..., 2]), _bits(_masked(pen.numpy(), LENS))), scale
    # in place (out = base, the doubled state), as the sampling loops use it; no out3
    sc = torch.tensor([0.0, 1.0, SCALE]).cuda()
    x = torch.cat((base, torch.full((B, L, 2), float("nan")))).cuda()
    _raw(kind, x, eps2.cuda(), None, lens_dev, sc, z.cuda() if kind else None, sets[0], x, None)
    want = _masked(np_step(kind, bn, np_combine(en[:B], en[B:], [0.0, 1.0, SCALE]), zn if kind else None, sets[0]), LENS)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(np.concatenate((want, want))))
    # more than one block with a tail: 5 * 104 = 520 rows = two full blocks and 8 rows
    b2, e2, z2 = torch.randn((5, 104, 2), generator=g), torch.randn((10, 104, 2), generator=g), torch.randn((5, 104, 2), generator=g)
    s2 = [0.0, 1.0, SCALE, 4.0, 0.25]
    out = torch.empty((10, 104, 2)).cuda()
    _raw(kind, b2.cuda(), e2.cuda(), None, None, torch.tensor(s2).cuda(), z2.cuda() if kind else None, sets[1], out, None)
    want = np_step(kind, b2.numpy(), np_combine(e2.numpy()[:5], e2.numpy()[5:], s2), z2.numpy() if kind else None, sets[1])
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(np.concatenate((want, want))))


@pytest.mark.parametrize("lens", [None, [104, 40, 104, 8, 96]])
def test_guided_and_plain_ddim_updates_compute_one_u(lens):
    """dhw_guide_update(kind = 0) with both eps halves the same array equals dhw_ddim_update on that array bit for bit, at every
    scale: the difference is exactly +0, the product a zero, and e + (a zero) = e for e != 0; at scale 0 the select returns the
    equal half.  So the guided and the unguided instantiation of the step kernel compute the same U.  520 rows: two full
    blocks and 8 rows; the lengths cut inside blocks."""
    Bq, Lq = 5, 104
    g = torch.Generator().manual_seed(35)
    base, e = torch.randn((Bq, Lq, 2), generator=g) * 3, torch.randn((Bq, Lq, 2), generator=g)
    assert bool((e != 0).all())
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    scale = torch.tensor([0.0, 1.0, SCALE, 4.0, 0.25]).cuda()
    abar, one = _lib.schedule(T)[1], np.float32(1)
    for c in ((np.sqrt(abar[5]), np.sqrt(one - abar[5]), np.sqrt(abar[2]), np.sqrt(one - abar[2])),
              (np.float32(3.0), np.float32(0.1), np.float32(1.0 / 3), np.float32(0.7))):
        bd, ed, plain = base.cuda(), e.cuda(), torch.full((Bq, Lq, 2), float("nan")).cuda()
        rc = _lib.lib().dhw_ddim_update(bd.data_ptr(), ed.data_ptr(), None if lens is None else lens_dev.data_ptr(), Bq, Lq, float(c[0]), float(c[1]), float(c[2]),
                                        float(c[3]), plain.data_ptr(), _st())
        assert rc == 0, _lib.lib().dhw_last_error(None).decode()
        out = torch.full((2 * Bq, Lq, 2), float("nan")).cuda()
        _raw(0, bd, torch.cat((ed, ed)), None, lens_dev, scale, None, c, out, None)
        got, want = out.cpu().numpy(), plain.cpu().numpy()
        assert np.isfinite(want).all()
        assert np.array_equal(_bits(got[:Bq]), _bits(want)), c
        assert np.array_equal(_bits(got[Bq:]), _bits(got[:Bq])), c
        for b, n in enumerate(lens or []):
            assert not _bits(got[b, n:]).any() and not _bits(got[Bq + b, n:]).any(), (c, b)


# ---------------------------------------------------------------- 2. / 3. scale 1 and scale 0 are the plain calls
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_scale_one_and_zero_are_the_plain_calls(prec):
    m = get_model(prec)
    text, style, latent, utext, ustyle = _gpu("text", "style", "latent", "utext", "ustyle")
    kw = dict(T=T, steps=4)
    g1 = dhg_amd.sample_ddim(m, text, style, latent=latent, lengths=LENS, guidance=1.0, **kw)
    six = dhg_amd.sample_ddim(m, torch.cat((text, utext)), torch.cat((style, ustyle)), latent=torch.cat((latent, latent)), lengths=LENS + LENS, **kw)
    three = dhg_amd.sample_ddim(m, text, style, latent=latent, lengths=LENS, **kw)
    assert _veq(g1, six[:B]), "scale 1 differs from rows 0-2 of the plain 6-row batch"
    assert _veq(g1, three), "scale 1 differs from the plain call at B = 3 (the 6-row comparison holds: a finding about the forward)"
    g0 = dhg_amd.sample_ddim(m, text, style, latent=latent, lengths=LENS, guidance=0.0, **kw)
    null = dhg_amd.sample_ddim(m, utext, ustyle, latent=latent, lengths=LENS, **kw)
    assert _veq(g0[..., :2], null[..., :2]) and _veq(g0[..., :2], six[B:, :, :2])     # (the pen column is the conditional row's at every scale)
    assert not torch.equal(g1, g0)
    # guiding against the condition itself is that condition's sample at any scale, pen included
    same = dhg_amd.sample_ddim(m, text, style, latent=latent, lengths=LENS, guidance=SCALE, uncond_text=text, uncond_style=style, **kw)
    assert _veq(same, three)
    # the ancestral loop, external noise
    (noise,) = _gpu("noise")
    for mode in ("new", "standard"):
        a1 = dhg_amd.sample(m, text, style, L=L, T=T, diffusion_mode=mode, noise=noise, lengths=LENS, guidance=1.0)
        a0 = dhg_amd.sample(m, text, style, L=L, T=T, diffusion_mode=mode, noise=noise, lengths=LENS, guidance=0.0)
        assert torch.isfinite(a1).all() and torch.isfinite(a0).all() and not torch.equal(a1, a0), mode
        for b, n in enumerate(LENS):
            assert torch.equal(a1[b, n:], torch.zeros_like(a1[b, n:])), (mode, b)


# ---------------------------------------------------------------- 4. rows are independent: lengths and scales
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_ragged_and_mixed_scale_rows_equal_their_own_runs(prec):
    m = get_model(prec)
    text, style, noise = _gpu("text", "style", "noise")
    scales = [0.0, SCALE, 1.0]
    kw = dict(T=T, steps=4, seed=9)
    rag, lat = dhg_amd.sample_ddim(m, text, style, L=L, lengths=LENS, first_sample=3, return_latent=True, guidance=scales, **kw)
    anc = dhg_amd.sample(m, text, style, L=L, T=T, lengths=LENS, seed=9, first_sample=3, guidance=scales)
    assert torch.isfinite(rag).all() and torch.isfinite(anc).all()
    for b, n in enumerate(LENS):
        alone, lat1 = dhg_amd.sample_ddim(m, text[b:b + 1], style[b:b + 1], L=n, first_sample=3 + b, return_latent=True, guidance=scales[b], **kw)
        assert torch.equal(rag[b, :n], alone[0]) and torch.equal(lat[b, :n], lat1[0]), b
        assert torch.equal(rag[b, n:], torch.zeros_like(rag[b, n:])) and torch.equal(lat[b, n:], torch.zeros_like(lat[b, n:]))
        uni = dhg_amd.sample_ddim(m, text, style, L=L, lengths=LENS, first_sample=3, guidance=scales[b], **kw)
        assert torch.equal(rag[b], uni[b]), b
        a1 = dhg_amd.sample(m, text[b:b + 1], style[b:b + 1], L=n, T=T, seed=9, first_sample=3 + b, guidance=scales[b])
        assert torch.equal(anc[b, :n], a1[0]) and torch.equal(anc[b, n:], torch.zeros_like(anc[b, n:])), b
    # every length == L: the call without lengths
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, L=L, lengths=[L] * B, guidance=scales, **kw), dhg_amd.sample_ddim(m, text, style, L=L, guidance=scales, **kw))
    # rows past the lengths are never read: NaN there changes nothing
    dl = lat.clone()
    for b, n in enumerate(LENS):
        dl[b, n:] = float("nan")
    assert torch.equal(dhg_amd.sample_ddim(m, text, style, latent=dl, lengths=LENS, guidance=scales, T=T, steps=4), rag)
    dn = noise.clone()
    for b, n in enumerate(LENS):
        dn[:, b, n:] = float("nan")
    assert torch.equal(dhg_amd.sample(m, text, style, L=L, T=T, noise=dn, lengths=LENS, guidance=scales),
                       dhg_amd.sample(m, text, style, L=L, T=T, noise=noise, lengths=LENS, guidance=scales))


# ---------------------------------------------------------------- 5. the latent handed back; the sampler is left alone; DHW_PERSIST
def test_latent_hand_back_and_the_sampler_is_left_alone():
    m = fresh_model("bf16")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=3, seed=7, first_sample=2, lengths=LENS)
    first = dhg_amd.sample(m, text, style, **kw).cpu()                 # captures the graph, sets the generator state
    g = dict(L=L, T=T, steps=4, lengths=LENS, guidance=SCALE)
    out, lat = dhg_amd.sample_ddim(m, text, style, seed=5, return_latent=True, **g)
    anc = dhg_amd.sample(m, text, style, L=L, T=T, seed=1, lengths=LENS, guidance=SCALE)
    again = dhg_amd.sample(m, text, style, **kw).cpu()                 # replays it
    assert torch.isfinite(first).all() and torch.isfinite(out).all() and torch.isfinite(anc).all() and torch.equal(first, again)
    back = dhg_amd.sample_ddim(m, text, style, latent=lat, seed=99, **{k: v for k, v in g.items() if k != "L"})
    assert torch.equal(out, back)
    assert torch.equal(lat.cpu(), torch.from_numpy(_masked(m.debug_randn(5, 0, B, L, -1).numpy(), LENS)))       # the x_T dhw_sample draws
    assert not torch.equal(dhg_amd.sample_ddim(m, text, style, seed=6, **g), out)
    assert torch.equal(out, dhg_amd.sample_ddim(get_model("bf16"), text, style, seed=5, **g))


def test_persistent_step_handle_samples_the_same(monkeypatch):
    monkeypatch.setenv("DHW_PERSIST", "1")
    m = fresh_model("bf16")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=T, steps=4, seed=3, lengths=LENS, guidance=SCALE)
    got = dhg_amd.sample_ddim(m, text, style, **kw)   # handle created under the switch
    monkeypatch.delenv("DHW_PERSIST")
    assert torch.isfinite(got).all() and torch.equal(got, dhg_amd.sample_ddim(get_model("bf16"), text, style, **kw))


# ---------------------------------------------------------------- 6. capacity, and the C entry's refusals
def test_capacity_the_c_entry_refuses_python_grows():
    m = get_model("bf16")
    text, style, utext, ustyle = _gpu("text", "style", "utext", "ustyle")
    text2, style2 = torch.cat((text, utext)), torch.cat((style, ustyle))
    good = dhg_amd.sample_ddim(m, text, style, L=L, T=T, steps=4, seed=1, lengths=LENS, guidance=SCALE)
    l, h = _lib.lib(), m._handle
    out = torch.full((B, L, 3), float("nan"), device="cuda")
    pad = torch.zeros((B * L * 2 + 2,), device="cuda")

    def arr(v, ty=C.c_int32):
        return (ty * max(1, len(v)))(*v)

    def ddim(levels=(8, 5, 2, 0), B_=B, lens=LENS, scale=(SCALE,) * B, latent=None, latent_out=None, t2=text2):
        rc = l.dhw_guided_ddim_sample(h, t2.data_ptr() if t2 is not None else None, style2.data_ptr(), B_, L, Lt, arr(lens) if lens is not None else None, T,
                                      arr(levels), len(levels), arr(scale, C.c_float) if scale is not None else None, latent, 1, 0, out.data_ptr(), latent_out, _st())
        return rc, l.dhw_last_error(h).decode()

    def anc(T_=T, mode=0, B_=B, lens=LENS, scale=(SCALE,) * B, noise=None):
        rc = l.dhw_guided_sample(h, text2.data_ptr(), style2.data_ptr(), B_, L, Lt, arr(lens) if lens is not None else None, T_, mode,
                                 arr(scale, C.c_float), noise, 1, 0, out.data_ptr(), _st())
        return rc, l.dhw_last_error(h).decode()

    five = (SCALE,) * 5
    cases = [(ddim(B_=5, lens=None, scale=five), "2B = 10"), (ddim(B_=5, lens=None, scale=five), "max_B = 8"), (anc(B_=5, lens=None, scale=five), "2B = 10"),
             (ddim(scale=(1.0, -0.5, 1.0)), "scale[1] = -0.5"), (ddim(scale=(1.0, 1.0, 64.5)), "scale[2] = 64.5"), (ddim(scale=(float("nan"), 1.0, 1.0)), "scale[0] = nan"),
             (anc(scale=(1.0, float("inf"), 1.0)), "scale[1] = inf"), (ddim(scale=None), "(scale)"), (ddim(t2=None), "(text2)"),
             (ddim(levels=(5, 5, 2)), "strictly decreasing"), (ddim(levels=()), "S = 0"), (ddim(lens=[24, 44, 40]), "lens[1] = 44"),
             (ddim(latent=pad.data_ptr() + 4), "latent must be 8-byte aligned"), (ddim(latent_out=pad.data_ptr() + 4), "latent_out must be 8-byte aligned"),
             (anc(T_=0), "T = 0"), (anc(mode=2), "mode = 2"), (anc(noise=pad.data_ptr() + 4), "noise must be 8-byte aligned"), (anc(B_=9, lens=None, scale=(1.0,) * 9), "B=9")]
    for (rc, msg), what in cases:
        assert rc == -1 and what in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()   # nothing was launched
    rc, msg = ddim()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(out, good)   # the handle still works, and computes what it computed before
    # the Python call grows a handle that is too small for 2B rows, and computes the same
    small = fresh_model("bf16", max_B=4)
    got = dhg_amd.sample_ddim(small, text, style, L=L, T=T, steps=4, seed=1, lengths=LENS, guidance=SCALE)
    assert small._cap["max_B"] == 2 * B and torch.equal(got, good)


# ---------------------------------------------------------------- against the CPU reference, with measured bounds
CONFIGS = ("ddim4", "ddim9", "new", "standard")


def _ref_run(cfg, perturb=None):
    i, sd = _inputs(), _sd()
    if cfg.startswith("ddim"):
        return guide_ref.sample_ddim(ref_cpu.forward, sd, i["text"], i["style"], i["utext"], i["ustyle"], SCALE, dhg_amd.ddim_levels(T, int(cfg[4:])), T, i["latent"],
                                     lengths=LENS, perturb=perturb)
    return guide_ref.sample(ref_cpu.forward, sd, i["text"], i["style"], i["utext"], i["ustyle"], SCALE, L, i["noise"], T, cfg, lengths=LENS, perturb=perturb)


def _ref(cfg, tol=None):
    """The CPU reference on the shared inputs, plain (tol None) or perturbed by +-TOL[tol], once per configuration."""
    key = ("ref", cfg, tol)
    if key not in _CACHE:
        pert = None if tol is None else guide_ref.ddim_ref.sign_perturb(TOL[tol]["eps"], TOL[tol]["pen"], 90 + CONFIGS.index(cfg))
        _CACHE[key] = _ref_run(cfg, pert)
    return _CACHE[key]


def _bounds(cfg, tol):
    a, p = _ref(cfg), _ref(cfg, tol)
    return 4 * _dev(a[..., :2], p[..., :2]), 4 * _dev(a[..., 2], p[..., 2])


def _gpu_run(prec, cfg):
    key = ("gpu", prec, cfg)
    if key not in _CACHE:
        m = get_model(prec)
        text, style, latent, noise = _gpu("text", "style", "latent", "noise")
        if cfg.startswith("ddim"):
            out = dhg_amd.sample_ddim(m, text, style, T=T, steps=int(cfg[4:]), latent=latent, lengths=LENS, guidance=SCALE)
        else:
            out = dhg_amd.sample(m, text, style, L=L, T=T, diffusion_mode=cfg, noise=noise, lengths=LENS, guidance=SCALE)
        _CACHE[key] = out.cpu()
    return _CACHE[key]


@pytest.mark.parametrize("cfg", CONFIGS)
def test_fp32_guided_sampling_matches_the_cpu_reference(cfg):
    """Bound = 4x the deviation of the CPU reference under a +-TOL["fp32"] perturbation of every denoiser output of both branches
    (module docstring, with the CPU figures).  GPU errors: DESIGN.md §33."""
    want, got = _ref(cfg), _gpu_run("fp32", cfg)
    bx, bp = _bounds(cfg, "fp32")
    ex, ep = _dev(got[..., :2], want[..., :2]), _dev(got[..., 2], want[..., 2])
    print(f"guided {cfg} fp32 scale {SCALE}: CPU deviation x {bx / 4:.3e} pen {bp / 4:.3e}; bound x {bx:.3e} pen {bp:.3e}; GPU error x {ex:.3e} pen {ep:.3e}")
    assert torch.isfinite(got).all() and bx > 0 and bp > 0
    assert ex <= bx and ep <= bp
    for b, n in enumerate(LENS):
        assert torch.equal(got[b, n:], torch.zeros((L - n, 3)))


@pytest.mark.parametrize("cfg", CONFIGS)
def test_bf16_guided_sampling_tracks_the_fp32_handle(cfg):
    """The same construction at TOL["bf16"]: the bf16 handle against the fp32 handle, bound = 4x the deviation of the CPU
    reference under a +-TOL["bf16"] perturbation (module docstring).  GPU figures: DESIGN.md §33."""
    ref, got = _gpu_run("fp32", cfg), _gpu_run("bf16", cfg)
    bx, bp = _bounds(cfg, "bf16")
    ex, ep = _dev(got[..., :2], ref[..., :2]), _dev(got[..., 2], ref[..., 2])
    print(f"guided {cfg} bf16 vs fp32 scale {SCALE}: CPU deviation x {bx / 4:.3e} pen {bp / 4:.3e}; bound x {bx:.3e} pen {bp:.3e}; GPU difference x {ex:.3e} pen {ep:.3e}")
    assert torch.isfinite(got).all() and bx > 0 and bp > 0
    assert ex <= bx and ep <= bp


def test_scale_one_with_the_device_generator_tracks_sample():
    """Guided ancestral sampling at scale 1 draws what ``sample(seed=...)`` draws and moves along e_c: the two differ only in how
    the forward is issued (eager entries and the per-call sigma FFN against the fused graph with its all-steps tables).  Held to
    the fp32 bound of the "new" configuration above; whether it happens to be bitwise is printed."""
    m = get_model("fp32")
    text, style = _gpu("text", "style")
    kw = dict(L=L, T=T, seed=11, first_sample=4, lengths=LENS)
    plain = dhg_amd.sample(m, text, style, **kw).cpu()
    guided = dhg_amd.sample(m, text, style, guidance=1.0, **kw).cpu()
    bx, bp = _bounds("new", "fp32")
    ex, ep = _dev(guided[..., :2], plain[..., :2]), _dev(guided[..., 2], plain[..., 2])
    print(f"guided scale 1, device generator, vs sample(seed=): x {ex:.3e} pen {ep:.3e}; bound x {bx:.3e} pen {bp:.3e}; bitwise: {torch.equal(guided, plain)}")
    assert torch.isfinite(guided).all() and ex <= bx and ep <= bp


# ---------------------------------------------------------------- 7. the dropout kernel against its statement
def _drop_call(rng, Bq, Ltq, S, p, ids, mask, style, dropped):
    rc = _lib.lib().dhw_train_cond_drop(rng.data_ptr(), Bq, Ltq, S, p, ids.data_ptr(), mask.data_ptr(), style.data_ptr(), dropped.data_ptr(), _st())
    assert rc == 0, _lib.lib().dhw_train_last_error()


@pytest.mark.parametrize("S,captured", [(14, False), (1, False), (14, True)])
def test_cond_drop_equals_the_numpy_statement_bit_for_bit(S, captured):
    Bq, Ltq, seed, GUARD = 13, 7, 0x1234567_89ABCDEF, 64
    g = torch.Generator().manual_seed(4)
    ids0 = torch.randint(1, spec.VOCAB, (Bq, Ltq), generator=g)
    ids0[:, Ltq - 2:] = 0
    mask0, style0 = (ids0 == 0).float(), torch.randn((Bq, S, 1280), generator=g)
    n_ids, n_sty = Bq * Ltq, Bq * S * 1280
    rng = torch.zeros(2, dtype=torch.int64, device=DEV)
    bufs = dict(ids=torch.empty(n_ids + GUARD, dtype=torch.int64, device=DEV), mask=torch.empty(n_ids + GUARD, device=DEV),
                style=torch.empty(n_sty + GUARD, device=DEV), dropped=torch.empty(Bq + GUARD, dtype=torch.int32, device=DEV))

    def fill():
        for k, (src, n) in dict(ids=(ids0, n_ids), mask=(mask0, n_ids), style=(style0, n_sty)).items():
            bufs[k].fill_(-7)
            bufs[k][:n].copy_(src.reshape(-1))
        bufs["dropped"].fill_(-7)

    graph = None
    seen = set()
    for index, p in ((0, 0.3), (1, 0.3), (7, 0.5), (2 ** 33, 0.3), (1, 0.0), (1, 1.0)):
        fill()
        rng.copy_(torch.tensor([seed, index], dtype=torch.int64))
        torch.cuda.synchronize()
        if not captured:
            _drop_call(rng, Bq, Ltq, S, p, bufs["ids"], bufs["mask"], bufs["style"], bufs["dropped"])
        elif p == 0.3:          # one capture serves every draw index: rng is read at replay
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    _drop_call(rng, Bq, Ltq, S, p, bufs["ids"], bufs["mask"], bufs["style"], bufs["dropped"])
                fill()
            graph.replay()
        else:
            continue
        torch.cuda.synchronize()
        want_d = guide_ref.cond_drop(seed, index, Bq, p)
        wi, wm, ws = guide_ref.apply_drop(want_d, ids0.numpy(), mask0.numpy(), style0.numpy())
        assert np.array_equal(bufs["dropped"][:Bq].cpu().numpy(), want_d), (index, p)
        assert np.array_equal(bufs["ids"][:n_ids].cpu().numpy().reshape(Bq, Ltq), wi) and np.array_equal(_bits(bufs["mask"][:n_ids].cpu().numpy().reshape(Bq, Ltq)), _bits(wm))
        assert np.array_equal(_bits(bufs["style"][:n_sty].cpu().numpy().reshape(Bq, S, 1280)), _bits(ws)), (index, p)
        for k, n in dict(ids=n_ids, mask=n_ids, style=n_sty, dropped=Bq).items():
            assert bool((bufs[k][n:] == -7).all()), f"{k}: written past its end"
        if p == 0.0:
            assert not want_d.any()
        if p == 1.0:
            assert want_d.all()
        seen.add(tuple(want_d.tolist()))
    assert len(seen) >= (3 if captured else 5)   # the draws differ from index to index: both kinds of sample were exercised


# ---------------------------------------------------------------- 8. - 10. the training step
SHAPE = dict(B=2, L=64, Lt=10, N=9, S=14)
BUFFERS = ("x", "pen", "alphas", "sigma", "ids", "mask", "style")


def _dataset(N, Lq, Ltq, S, seed=5):
    g = torch.Generator().manual_seed(seed)
    strokes = torch.cat([torch.randn(N, Lq, 2, generator=g), (torch.rand(N, Lq, 1, generator=g) < 0.2).float()], dim=-1)
    text = torch.randint(1, spec.VOCAB, (N, Ltq), generator=g)
    text[:, Ltq - 2:] = 0
    return {"strokes": strokes, "text": text, "style": torch.randn(N, S, 1280, generator=g).abs()}


def _setup():
    if "train" not in _CACHE:
        d = _dataset(SHAPE["N"], SHAPE["L"], SHAPE["Lt"], SHAPE["S"])
        d["writer"] = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2])
        _CACHE["train"] = (d, spec.synthetic_state_dict(2, 128, 192, 256, seed=0), dhg_amd.get_alpha_set(60).float())
    return _CACHE["train"]


def _step(sd, data=None, alpha_set=None, **kw):
    model = tm.TrainModel(sd, num_layers=2, device=DEV, drop_rate=0.1)
    return tm.GraphedTrainStep(model, train.Adam(model.parameters()), SHAPE["B"], SHAPE["L"], SHAPE["Lt"], seed=7, data=data, alpha_set=alpha_set, **kw)


def _run_pair(graph, resident, kw_a, kw_b, null_b):
    """Step A (built with kw_a) on update 3 of the resident data or of a host batch; step B (kw_b), host-fed, on the rows A trained
    on — with the null condition in place of their prompts and styles when null_b.  -> (A, B, loss A, loss B)."""
    d, sd, abar = _setup()
    k, Bq = 3, SHAPE["B"]
    if resident:
        a = _step(sd, tm.ResidentData(d, DEV), abar, **kw_a)
        loss_a = a(step=k, graph=graph).cpu()
        idx, src, alphas = (t.cpu().long() if t.dtype == torch.int32 else t.cpu() for t in a.last_draw())
    else:
        idx, src, alphas = torch.tensor([4, 1]), torch.tensor([3, 2]), torch.tensor([0.31, 0.77])
        a = _step(sd, **kw_a)
        loss_a = a({"strokes": d["strokes"][idx], "text": d["text"][idx], "style": d["style"][src]}, None, k, alphas=alphas.reshape(-1, 1), graph=graph).cpu()
    text, style = dhg_amd.null_condition(Bq, SHAPE["Lt"], SHAPE["S"]) if null_b else (d["text"][idx], d["style"][src])
    b = _step(sd, **kw_b)
    loss_b = b({"strokes": d["strokes"][idx], "text": text, "style": style}, None, k, alphas=alphas.reshape(-1, 1), graph=graph).cpu()
    return a, b, loss_a, loss_b


def _same_inputs(a, b):
    for name in BUFFERS + ("eps", "keep"):
        x, y = getattr(a, name).cpu(), getattr(b, name).cpu()
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), name


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("resident", [True, False])
def test_step_that_drops_every_condition_equals_the_step_fed_the_null_batch(graph, resident):
    a, b, loss_a, loss_b = _run_pair(graph, resident, dict(cond_drop=1.0), {}, True)
    assert torch.equal(a.last_dropped().cpu(), torch.ones(SHAPE["B"], dtype=torch.int32))
    assert a.ids.cpu().tolist() == [[1] + [0] * (SHAPE["Lt"] - 1)] * SHAPE["B"] and not a.style.any()
    _same_inputs(a, b)
    print("losses dropped / null-fed:", loss_a.tolist(), loss_b.tolist())
    # (the loss sums are fp32 atomics over blocks: the same inputs give the same loss up to summation order — test_gpu_resident.py's 2e-6)
    assert bool(torch.isfinite(loss_a).all()) and bool(((loss_a - loss_b).abs() <= 2e-6 * loss_b.abs()).all()), (loss_a, loss_b)
    with pytest.raises(ValueError, match="cond_drop = 0"):
        b.last_dropped()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("resident", [True, False])
def test_step_built_with_cond_drop_zero_is_the_step_built_without_it(graph, resident):
    a, b, loss_a, loss_b = _run_pair(graph, resident, dict(cond_drop=0.0), {}, False)
    assert a.dropped is None and b.dropped is None       # nothing allocated, nothing launched
    _same_inputs(a, b)
    assert bool(torch.isfinite(loss_a).all()) and bool(((loss_a - loss_b).abs() <= 2e-6 * loss_b.abs()).all()), (loss_a, loss_b)


def test_step_drops_what_the_statement_says_under_replay():
    """p = 0.5 under graph replay: the flags of update n are guide_ref.cond_drop(seed, n, B, p) — one capture, the draw index is
    read at replay — and a kept sample keeps its rows."""
    d, sd, abar = _setup()
    a = _step(sd, tm.ResidentData(d, DEV), abar, cond_drop=0.5, warmup=10 ** 9)
    seen = set()
    for n in (1, 2, 5, 6, 1):
        a(step=n)
        want = guide_ref.cond_drop(7, n, SHAPE["B"], 0.5)
        got = a.last_dropped().cpu().numpy()
        assert np.array_equal(got, want), (n, got, want)
        idx, src, _ = (t.cpu().long() for t in a.last_draw())
        wi, wm, ws = guide_ref.apply_drop(want, d["text"][idx].numpy(), (d["text"][idx] == 0).float().numpy(), d["style"][src].numpy())
        assert np.array_equal(a.ids.cpu().numpy(), wi) and np.array_equal(a.mask.cpu().numpy(), wm) and np.array_equal(a.style.cpu().numpy(), ws), n
        seen.add(tuple(want.tolist()))
    assert a.graph is not None and len(seen) > 1


# ---------------------------------------------------------------- 11. fit(cond_drop=0.5)
def test_fit_with_cond_drop_trains_from_the_twelve_sample_file(tmp_path):
    cfg = tmp_path / "cfg.yml"
    cfg.write_text("""
experiment: {seed: 1}
dataset_args: {max_seq_len: 64, max_text_len: 8}
training_args: {steps: 4, batch_size: 2, warmup_steps: 100, clip_grad: 100.0, dropout: 0.1, att_layers_num: 2, channels: 128, log_freq: 2, save_freq: 3}
optimizer: {type: torch.optim.Adam, params: {lr: 0.0003, weight_decay: 0.00001, betas: [0.9, 0.98]}}
""")
    d = _dataset(12, 64, 8, 14, seed=8)
    d["writer"] = torch.arange(12) // 3
    torch.save(d, tmp_path / "batches.pt")
    lines = []
    tm.fit(cfg, tmp_path / "batches.pt", tmp_path / "run", log=lines.append, resident=True, cond_drop=0.5)
    assert len(lines) == 2 and lines[0].startswith("Step 2 | Loss: ")
    sd = torch.load(tmp_path / "run" / "model_final.pth", weights_only=True)
    ref = spec.synthetic_state_dict(2, seed=0)
    assert list(sd) == list(ref) and all(bool(torch.isfinite(v).all()) for v in sd.values())
    assert max(float((sd[k] - torch.from_numpy(ref[k])).abs().max()) for k in ref) > 0
    with pytest.raises(ValueError, match="cond_drop = 1.5"):
        tm.fit(cfg, tmp_path / "batches.pt", tmp_path / "bad", log=lines.append, cond_drop=1.5)
