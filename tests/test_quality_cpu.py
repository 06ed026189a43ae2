"""Host side of the sample-quality metric (include/dhw.h dhw_moments_update; dhg_amd.FeatureStats, frechet_distance,
sample_quality) that needs no GPU: the two symbols declared, exported and bound, every argument rule of the C entry through the
handle-less error path, frechet_distance against closed forms, the rank-deficient case, and FeatureStats on a host state."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, quality

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moments_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


# ---------------------------------------------------------------- the C-ABI
def test_moments_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bsize_t\s+dhw_moments_workspace_bytes\s*\(", header) and re.search(r"\bint\s+dhw_moments_update\s*\(", header)
    l = _lib.lib()
    for name in ("dhw_moments_workspace_bytes", "dhw_moments_update"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_moments_update.restype is C.c_int and l.dhw_moments_workspace_bytes.restype is C.c_size_t
    assert len(_lib.SIGNATURES["dhw_moments_update"][1]) == 9 and len(_lib.SIGNATURES["dhw_moments_workspace_bytes"][1]) == 3
    for name in ("FeatureStats", "frechet_distance", "line_features", "sample_quality"):
        assert getattr(dhg_amd, name) is getattr(quality, name)


def test_moments_workspace_bytes():
    f = _lib.lib().dhw_moments_workspace_bytes
    assert f(67, 14, 1280) == 67 * 1280 * 8 and f(1, 1, 16) == 128 and f(16384, 64, 2048) == 0   # (the last: N S D >= 2^31)
    for N, S, D in ((0, 1, 16), (16385, 1, 16), (1, 0, 16), (1, 65, 16), (1, 1, 8), (1, 1, 24), (1, 1, 2064), (1, 1, 0), (-1, -1, -16)):
        assert f(N, S, D) == 0, (N, S, D)


def _call(**kw):
    a = dict(feat=FAKE, N=5, S=2, D=48, sum=FAKE, gram=FAKE, ws=FAKE, ws_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["ws_bytes"] is None:
        a["ws_bytes"] = l.dhw_moments_workspace_bytes(a["N"], a["S"], a["D"])
    rc = l.dhw_moments_update(a["feat"], a["N"], a["S"], a["D"], a["sum"], a["gram"], a["ws"], a["ws_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


BAD_C = [
    (dict(N=0), r"\bN must be"), (dict(N=16385), r"\bN must be"), (dict(S=0), r"\bS must be"), (dict(S=65), r"\bS must be"),
    (dict(D=8), r"\bD must be"), (dict(D=24), r"\bD must be"), (dict(D=2064), r"\bD must be"),
    (dict(N=16384, S=64, D=2048, ws_bytes=1 << 40), r"N S D"),
    (dict(feat=None), "feat is NULL"), (dict(sum=None), "sum is NULL"), (dict(gram=None), "gram is NULL"), (dict(ws=None), "ws is NULL"),
    (dict(feat=FAKE + 4), "feat must be 16-byte aligned"), (dict(sum=FAKE + 8), "sum must be 16-byte aligned"),
    (dict(gram=FAKE + 8), "gram must be 16-byte aligned"), (dict(ws=FAKE + 8), "ws must be 16-byte aligned"),
    (dict(ws_bytes=5 * 48 * 8 - 1), "ws_bytes"),
]


@pytest.mark.parametrize("bad,name", BAD_C)
def test_each_argument_rule_of_dhw_moments_update_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_moments_update:"), (bad, msg)


def test_kernel_constants_match_the_wrapper():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "moments", "moments.h")).read()
    for name in ("MOMENTS_MAX_N", "MOMENTS_MAX_S", "MOMENTS_MIN_D", "MOMENTS_MAX_D"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(quality, name)
    assert quality.FeatureStats.chunk == quality.MOMENTS_MAX_N


# ---------------------------------------------------------------- frechet_distance against closed forms
D, N = 48, 200


def _set(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.standard_normal((N, D)) * g.uniform(0.5, 1.2, D) + g.uniform(-1, 1, D)


def _stats(x):
    x = np.asarray(x, np.float64)
    return quality.FeatureStats.from_state(len(x), x.sum(0), x.T @ x)


XA, XB = _set(1), _set(2)


@pytest.mark.parametrize("via", ["pairs", "stats"])
def test_frechet_distance_closed_forms(via):
    """D = 48, 200 samples per set (full rank).  Bound: 1e-10 (tr Ca + tr Cb); the eigen-solver's own rounding is around 1e-13 at
    tr = 36 and is not what is tested."""
    def fd(x, y):
        if via == "pairs":
            return dhg_amd.frechet_distance(moments_ref.mean_cov(x), moments_ref.mean_cov(y))
        return dhg_amd.frechet_distance(_stats(x), _stats(y))

    ma, ca = moments_ref.mean_cov(XA)
    tra, trb = np.trace(ca), np.trace(moments_ref.mean_cov(XB)[1])
    errs = {"identical": abs(fd(XA, XA)) / (2e-10 * tra)}
    c = 0.75
    errs["shift"] = abs(fd(XA, XA + c) - 48 * c * c) / (2e-10 * tra)
    errs["scaled"] = abs(fd(XA, 2 * (XA - ma) + ma) - tra) / (1e-10 * 5 * tra)
    errs["symmetric"] = abs(fd(XA, XB) - fd(XB, XA)) / (1e-10 * (tra + trb))
    q, _ = np.linalg.qr(np.random.Generator(np.random.PCG64(3)).standard_normal((D, D)))
    errs["rotated"] = abs(fd(XA @ q, XB @ q) - fd(XA, XB)) / (1e-10 * (tra + trb))
    errs["reference"] = abs(fd(XA, XB) - moments_ref.frechet_distance(ma, ca, *moments_ref.mean_cov(XB))) / (1e-10 * (tra + trb))
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert fd(XA, XB) > 0.1 * tra and all(v <= 1 for v in errs.values()), errs


def test_frechet_distance_of_a_rank_deficient_set_with_itself():
    """D = 48, N = 7: the covariance has rank 6, the square roots of clipped eigenvalues leave about 1e-7 tr.  Measured with
    tests/moments_ref.py for this construction: FD(a, a) = -4.13e-06 at tr = 42.22 (9.8e-08 tr) from np.cov, and -3.68e-06
    (8.7e-08 tr) from dhg_amd.frechet_distance on the (count, sum, gram) state; at D = 1280, N = 64 the same statement gives
    -1.45e-04 at tr = 991 (1.5e-07 tr).  Asserted: |FD(a, a)| <= 1e-5 tr, and the warning about count <= D."""
    x = _set(4)[:7]
    m, c = moments_ref.mean_cov(x)
    tr = np.trace(c)
    ref = moments_ref.frechet_distance(m, c, m, c)
    with pytest.warns(UserWarning, match="rank-deficient"):
        got = dhg_amd.frechet_distance(_stats(x), _stats(x))
    print(f"rank-deficient self-distance: ref {ref:.3e}, got {got:.3e}, tr {tr:.4g}, ratio {abs(got) / tr:.2e}")
    assert abs(got) <= 1e-5 * tr and abs(ref) <= 1e-5 * tr
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dhg_amd.frechet_distance(_stats(XA), _stats(XB))            # 200 > 48: silent
        dhg_amd.frechet_distance((m, c), (m, c))                    # pairs carry no count: silent
    with pytest.raises(ValueError, match="dimensions"):
        dhg_amd.frechet_distance((m, c), (m[:16], c[:16, :16]))


# ---------------------------------------------------------------- FeatureStats without a device
def test_feature_stats_mean_and_cov_from_a_host_state():
    st = _stats(XA)
    m, c = moments_ref.mean_cov(XA)
    assert st.count == N and st.D == D
    assert np.abs(st.mean() - m).max() <= 1e-12 * np.abs(m).max()
    assert np.abs(st.cov() - c).max() <= 1e-12 * np.abs(c).max() and np.array_equal(st.cov(), st.cov().T)


def test_feature_stats_save_and_load_round_trip_bit_exactly(tmp_path):
    st = _stats(XA)
    path = tmp_path / "real.npz"
    st.save(path)
    assert sorted(np.load(path).files) == ["count", "gram", "sum"]
    back = dhg_amd.FeatureStats.load(path)
    assert back.count == st.count and back.D == st.D
    for a, b in zip(back._state(), st._state()):
        assert a.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))
    assert dhg_amd.frechet_distance(st, back) == dhg_amd.frechet_distance(st, st)


def test_feature_stats_refusals():
    for bad in (8, 24, 2064, 0, 48.0, True):
        with pytest.raises(ValueError, match="D = "):
            dhg_amd.FeatureStats(bad)
    empty = dhg_amd.FeatureStats(48)
    assert empty.count == 0
    with pytest.raises(ValueError, match="fewer than 1"):
        empty.mean()
    one = quality.FeatureStats.from_state(1, XA[0], np.outer(XA[0], XA[0]))
    assert np.array_equal(one.mean(), XA[0])
    with pytest.raises(ValueError, match="fewer than 2"):
        one.cov()
    for v in (np.nan, np.inf):
        s, g = XA.sum(0), XA.T @ XA
        g[3, 5] = v
        with pytest.raises(ValueError, match="non-finite"):
            quality.FeatureStats.from_state(N, s, g).cov()
        s[7] = v
        with pytest.raises(ValueError, match="non-finite"):
            quality.FeatureStats.from_state(N, s, XA.T @ XA).mean()
    with pytest.raises(ValueError, match="gram"):
        quality.FeatureStats.from_state(3, np.zeros(48), np.zeros((48, 32)))
    with pytest.raises(ValueError, match=r"features must be floating-point \[N, S, 48\]"):
        empty.update(np.zeros((3, 2, 32), np.float32))
    with pytest.raises(ValueError, match="S = 65"):
        empty.update(np.zeros((3, 65, 48), np.float32))


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


def test_sample_quality_rejects_unknown_keywords_before_any_device_access(monkeypatch):
    _no_device(monkeypatch)
    data = {"strokes": torch.zeros(4, 16, 3), "text": torch.ones(4, 3, dtype=torch.int64), "style": torch.zeros(4, 14, 1280)}
    with pytest.raises(TypeError, match="unknown sampler keyword.*temperature.*for sample "):
        dhg_amd.sample_quality(None, data, None, temperature=2.0)
    with pytest.raises(TypeError, match="diffusion_mode.*for sample_ddim"):
        dhg_amd.sample_quality(None, data, None, steps=4, diffusion_mode="new")
    with pytest.raises(TypeError, match="steps"):
        dhg_amd.sample_quality(None, data, None, levels=[3, 1], step=4)
    with pytest.raises(ValueError, match="missing 'style'"):
        dhg_amd.sample_quality(None, {"strokes": data["strokes"], "text": data["text"]}, None)
    for bad in (1, 5, 2.0):
        with pytest.raises(ValueError, match="n = "):
            dhg_amd.sample_quality(None, data, None, n=bad)
    with pytest.raises(ValueError, match="batch"):
        dhg_amd.sample_quality(None, data, None, batch=0)
    with pytest.raises(ValueError, match="real must be"):
        dhg_amd.sample_quality(None, data, None, real=(np.zeros(1280), np.eye(1280)))
