"""Host side of the dynamic time warping between stroke lines (include/dhw.h dhw_dtw_workspace_bytes / dhw_dtw; dhg_amd.stroke_features,
dtw_distance, nearest_strokes) that needs no GPU: the two symbols declared, exported and bound, every argument rule of the C entry
through the handle-less error path, the workspace size, the Python refusals before any device access, the --dtw flag of
tools/eval_samples.py, and the numpy reference's own checks (tests/dtw_ref.py): its two forms agree bit for bit and obey the
closed forms of the metric.

dhw_dtw takes the 18 arguments of its declaration in include/dhw.h (a, lens_a, M, La, b, lens_b, N, Lb, F, normalize, skip_diag,
dist_out, steps_out, nearest_out, nearest_idx, ws, ws_bytes, hip_stream)."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib
from dhg_amd import dtw as dtw_mod

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it
ARGS = {"dhw_dtw_workspace_bytes": 5, "dhw_dtw": 18}
TIE_LENS_A, TIE_LENS_B = [3, 3, 16, 10, 12], [12, 14, 1, 10, 3, 8, 18]


def tie_data():
    """Binary features, F = 3, from PCG64(11): many cells where two or three predecessors tie."""
    g = np.random.Generator(np.random.PCG64(11))
    a = g.integers(0, 2, size=(len(TIE_LENS_A), max(TIE_LENS_A), 3)).astype(np.float32)
    b = g.integers(0, 2, size=(len(TIE_LENS_B), max(TIE_LENS_B), 3)).astype(np.float32)
    return a, b


# ---------------------------------------------------------------- the C-ABI
def test_dtw_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    l = _lib.lib()
    for name, nargs in ARGS.items():
        ret = "size_t" if name.endswith("_bytes") else "int"
        decl = re.search(rf"\b{ret}\s+{name}\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(params.split(",")) == nargs, name
        assert name in _lib.SIGNATURES and hasattr(l, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(l, name).restype is (C.c_size_t if ret == "size_t" else C.c_int)
    for name in ("stroke_features", "dtw_distance", "nearest_strokes"):
        assert getattr(dhg_amd, name) is getattr(dtw_mod, name)


def test_dtw_workspace_bytes():
    f = _lib.lib().dhw_dtw_workspace_bytes
    assert f(1, 1, 1, 1, 1) == 16                        # the [M,N] fp32 matrix, rounded up to 16 bytes
    assert f(5, 7, 64, 65, 3) == 144 and f(5, 7, 1, 1024, 4) == 144
    assert f(1024, 1024, 488, 488, 3) == 4 << 20
    assert f(16384, 4096, 1024, 1024, 4) == 1 << 28
    for dims in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (16385, 1, 1, 1, 1), (1, 16385, 1, 1, 1), (16384, 4097, 8, 8, 3), (8192, 8193, 8, 8, 3),
                 (1, 1, 0, 1, 1), (1, 1, 1025, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1025, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 5), (-1, -1, -1, -1, -1)):
        assert f(*dims) == 0, dims
    for dims in ((3, 5, 17, 33, 2), (16384, 4096, 1024, 1024, 4), (2, 2, 1024, 1024, 3)):
        assert f(*dims) > 0 and f(*dims) % 16 == 0


def call(**kw):
    a = dict(a=FAKE, lens_a=FAKE, M=3, La=40, b=FAKE, lens_b=FAKE, N=5, Lb=50, F=3, normalize=1, skip_diag=0, dist_out=FAKE, steps_out=FAKE,
             nearest_out=FAKE, nearest_idx=FAKE, ws=FAKE, ws_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["ws_bytes"] is None:
        a["ws_bytes"] = l.dhw_dtw_workspace_bytes(a["M"], a["N"], a["La"], a["Lb"], a["F"])
    rc = l.dhw_dtw(a["a"], a["lens_a"], a["M"], a["La"], a["b"], a["lens_b"], a["N"], a["Lb"], a["F"], a["normalize"], a["skip_diag"], a["dist_out"],
                   a["steps_out"], a["nearest_out"], a["nearest_idx"], a["ws"], a["ws_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


POINTERS = ("a", "lens_a", "b", "lens_b", "dist_out", "steps_out", "nearest_out", "nearest_idx", "ws")
BAD = [
    (dict(M=0), r"\bM must be"), (dict(M=16385), r"\bM must be"), (dict(N=0), r"\bN must be"), (dict(N=16385), r"\bN must be"),
    (dict(M=16384, N=4097), "M N must be at most 2\\^26"), (dict(M=8193, N=8192), "M N must be at most 2\\^26"),
    (dict(La=0), r"\bLa must be"), (dict(La=1025), r"\bLa must be"), (dict(Lb=0), r"\bLb must be"), (dict(Lb=1025), r"\bLb must be"),
    (dict(F=0), r"\bF must be"), (dict(F=5), r"\bF must be"),
    (dict(skip_diag=1), "skip_diag needs M == N"),
    (dict(dist_out=None, steps_out=None, nearest_out=None, nearest_idx=None), "dist_out, steps_out and nearest_out are all NULL"),
    (dict(nearest_out=None), "nearest_idx needs nearest_out"),
    (dict(a=None), r"\ba is NULL"), (dict(b=None), r"\bb is NULL"), (dict(ws=None), "ws is NULL"),
    (dict(ws_bytes=59), "ws_bytes 59 < dhw_dtw_workspace_bytes"),
] + [({n: FAKE + 4}, rf"\b{n} must be 16-byte aligned") for n in POINTERS]


@pytest.mark.parametrize("bad,name", BAD, ids=["-".join(f"{k}={v}" for k, v in b.items()) for b, _ in BAD])
def test_each_argument_rule_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_dtw: "), (bad, msg)


def test_kernel_constants_match_the_wrapper():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "dtw", "dtw.h")).read()
    for name in ("DTW_MAX_N", "DTW_MAX_L", "DTW_MAX_F"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(dtw_mod, name)
    assert re.search(r"DTW_MAX_PAIRS = 1ll << 26;", src) and dtw_mod.DTW_MAX_PAIRS == 1 << 26


# ---------------------------------------------------------------- Python refusals, before any device access
def test_python_refusals_before_any_device_access(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    good = np.zeros((4, 16, 3), np.float32)
    for f, lengths in ((dhg_amd.stroke_features, "lengths"), (dhg_amd.dtw_distance, "lengths_a"), (dhg_amd.nearest_strokes, "lengths_q")):
        def fn(x, lens=None, f=f, lengths=lengths, **kw):
            return f(x, **{lengths: lens}, **kw)
        for v in (np.nan, np.inf, -np.inf):
            x = good.copy()
            x[2, 5, 1] = v
            with pytest.raises(ValueError, match="non-finite"):
                fn(x)
            with pytest.raises(ValueError, match="non-finite"):
                fn(torch.from_numpy(x), np.array([16, 16, 6, 16]))
        for lens in ([0, 16, 16, 16], [1, 2, 17, 3], [-1, 1, 1, 1]):
            with pytest.raises(ValueError, match=r"lengths must lie in \[1, 16\]"):
                fn(good, np.array(lens))
        with pytest.raises(ValueError, match="lengths must hold 4 integers"):
            fn(good, np.array([1, 2, 3]))
        with pytest.raises(ValueError, match="lengths must hold 4 integers"):
            fn(good, np.array([1.0, 2.0, 3.0, 4.0]))
        with pytest.raises(ValueError, match="kind = 'velocity' must be one of positions, offsets"):
            fn(good, kind="velocity")
        for w in (-1.0, float("nan"), float("inf"), "1", True):
            with pytest.raises(ValueError, match="pen_weight"):
                fn(good, pen_weight=w)
        for shape in ((4, 16, 2), (4, 16), (0, 16, 3), (4, 0, 3)):
            with pytest.raises(ValueError, match=r"strokes must be floating-point \[B, L, 3\]"):
                fn(np.zeros(shape, np.float32))
        with pytest.raises(ValueError, match=r"strokes must be floating-point \[B, L, 3\]"):
            fn(np.zeros((4, 16, 3), np.int32))
        with pytest.raises(ValueError, match="at most 1024"):
            fn(np.zeros((1, 1025, 3), np.float32))
    with pytest.raises(ValueError, match="non-finite"):
        dhg_amd.dtw_distance(good, np.full((2, 8, 3), np.nan, np.float32))
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 8\]"):
        dhg_amd.nearest_strokes(good, np.zeros((2, 8, 3), np.float32), None, np.array([9, 1]))
    with pytest.raises(ValueError, match="without the set"):
        dhg_amd.dtw_distance(good, None, None, np.array([1, 1, 1, 1]))
    with pytest.raises(ValueError, match="_chunk"):
        dhg_amd.dtw_distance(good, _chunk=0)
    # a NaN behind a line's length is not a refusal: the checks pass and the call stops at the missing device
    x = good.copy()
    x[2, 9:] = np.nan
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        dhg_amd.stroke_features(x, np.array([16, 16, 9, 16]))
    data = {"strokes": torch.zeros(4, 16, 3), "text": torch.ones(4, 3, dtype=torch.int64), "style": torch.zeros(4, 14, 1280)}
    with pytest.raises(ValueError, match="k = 9"):
        dhg_amd.sample_metrics(None, data, None, k=9, dtw=True)


def test_eval_samples_dtw_flag_parses():
    spec_ = importlib.util.spec_from_file_location("eval_samples_mod", os.path.join(ROOT, "tools", "eval_samples.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    a = mod.parser().parse_args(["--data", "x.pt", "--dtw", "--guidance", "1.5"])
    assert a.dtw is True and a.metrics is False
    a = mod.parser().parse_args(["--data", "x.pt", "--metrics"])
    assert a.dtw is False and a.metrics is True
    with pytest.raises(SystemExit):
        mod.main(["--data", "x.pt", "--dtw", "--real-stats", "r.npz"])


# ---------------------------------------------------------------- the reference's own checks
def test_the_two_forms_of_the_reference_agree_bit_for_bit():
    g = np.random.Generator(np.random.PCG64(5))
    lens = (1, 2, 3, 17, 40)
    for F in (1, 3, 4):
        for n in lens:
            for m in lens:
                a, b = g.normal(size=(n, F)).astype(np.float32), g.normal(size=(m, F)).astype(np.float32)
                d0, k0 = dtw_ref.dtw_loop(a, b)
                d1, k1 = dtw_ref.dtw_diag(a, b)
                assert np.float32(d0).tobytes() == np.float32(d1).tobytes() and k0 == k1, (F, n, m)
                ai, bi = g.integers(-7, 8, size=(n, F)), g.integers(-7, 8, size=(m, F))
                assert dtw_ref.dtw_loop(ai, bi) == dtw_ref.dtw_diag(ai, bi)
    a, b = tie_data()
    other = 0
    for p, n in enumerate(TIE_LENS_A):
        for q, m in enumerate(TIE_LENS_B):
            want = dtw_ref.dtw_loop(a[p, :n], b[q, :m])
            assert dtw_ref.dtw_diag(a[p, :n], b[q, :m]) == want
            swapped = dtw_ref.dtw_loop(a[p, :n], b[q, :m], order=("left", "up", "diag"))
            assert swapped[0] == want[0]                       # the distance does not depend on the tie order, the path length does
            other += swapped[1] != want[1]
    assert 4 * other >= len(TIE_LENS_A) * len(TIE_LENS_B), other


def test_reference_closed_forms():
    g = np.random.Generator(np.random.PCG64(6))
    for n in (1, 2, 17, 40):
        x = g.normal(size=(n, 3)).astype(np.float32)
        y = g.normal(size=(n + 5, 3)).astype(np.float32)
        for f in (dtw_ref.dtw_loop, dtw_ref.dtw_diag):
            assert f(x, x) == (0, n)                                       # the diagonal path: n cells of cost 0
            assert f(x, np.repeat(x, 2, axis=0)) == (0, 2 * n)             # every row matched twice, all at cost 0
            assert f(x, y)[0] == f(y, x)[0]                                # the distance is symmetric
    batch = g.normal(size=(3, 9, 2)).astype(np.float32)
    dist, steps = dtw_ref.dtw_batch(batch, [9, 0, 4], batch, [10, 9, 1], normalize=True)
    assert np.isinf(dist[1]).all() and np.isinf(dist[:, 0]).all() and (steps[1] == 0).all() and (steps[:, 0] == 0).all()
    d, k = dtw_ref.dtw_loop(batch[2, :4], batch[1])
    assert dist[2, 1] == np.float32(d) / np.float32(k) and steps[2, 1] == k
    best, idx = dtw_ref.nearest(dist)
    assert np.isinf(best[1]) and idx[1] == -1 and idx[0] in (1, 2) and best[0] == dist[0, 1:].min()
    feat = dtw_ref.features(np.array([[[1, 2, 0.4], [0.5, -1, 0.6], [2, 2, 1]]], np.float32), "positions", 4.0)
    assert np.array_equal(feat, np.array([[[0, 0, 0], [0.5, -1, 2], [2.5, 1, 2]]], np.float32))
