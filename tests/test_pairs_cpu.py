"""Host side of the pairwise metrics (include/dhw.h dhw_pairs_*; dhg_amd.FeatureSet, knn_radius, nearest, precision_recall,
kernel_distance, sample_metrics) that needs no GPU: the five symbols declared, exported and bound, every argument rule of the C
entries through the handle-less error path, the workspace size, the Python refusals before any device access, closed forms of the
numpy reference (tests/pairs_ref.py) and the --metrics flag of tools/eval_samples.py."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, quality

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it
ARGS = {"dhw_pairs_pool": 6, "dhw_pairs_workspace_bytes": 3, "dhw_pairs_knn": 8, "dhw_pairs_cover": 12, "dhw_pairs_polysum": 10}


# ---------------------------------------------------------------- the C-ABI
def test_pairs_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    l = _lib.lib()
    for name, nargs in ARGS.items():
        ret = "size_t" if name.endswith("_bytes") else "int"
        assert re.search(rf"\b{ret}\s+{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(l, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(l, name).restype is (C.c_size_t if ret == "size_t" else C.c_int)
    for name in ("FeatureSet", "knn_radius", "nearest", "precision_recall", "kernel_distance", "sample_metrics"):
        assert getattr(dhg_amd, name) is getattr(quality, name)


def test_pairs_workspace_bytes():
    f = _lib.lib().dhw_pairs_workspace_bytes
    # k-major copies of both sets padded to 64 rows, their squared norms, and 8 candidates per row and split (1 split per 64 columns)
    assert f(1, 1, 16) == 8 * (16 * 64 * 2 + 64 * 2 + 64 * 1 * 8)
    assert f(67, 37, 48) == 8 * (48 * 128 + 48 * 64 + 128 + 64 + 128 * 1 * 8)
    assert f(37, 67, 48) == 8 * (48 * 64 + 48 * 128 + 64 + 128 + 64 * 2 * 8)
    assert f(16384, 16384, 2048) == 8 * (2 * 2048 * 16384 + 2 * 16384 + 16384 * 32 * 8)
    for M, N, D in ((0, 1, 16), (1, 0, 16), (16385, 1, 16), (1, 16385, 16), (1, 1, 8), (1, 1, 24), (1, 1, 2064), (1, 1, 0), (-1, -1, -16)):
        assert f(M, N, D) == 0, (M, N, D)


def _err():
    return _lib.lib().dhw_last_error(None).decode()


def _ws(a, M, N):
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib.lib().dhw_pairs_workspace_bytes(M, N, a["D"])


def call_pool(**kw):
    a = dict(feat=FAKE, N=5, S=2, D=48, out=FAKE)
    a.update(kw)
    return _lib.lib().dhw_pairs_pool(a["feat"], a["N"], a["S"], a["D"], a["out"], None), _err()


def call_knn(**kw):
    a = dict(x=FAKE, N=5, D=48, k=3, radius2=FAKE, ws=FAKE, ws_bytes=None)
    a.update(kw)
    _ws(a, a["N"], a["N"])
    return _lib.lib().dhw_pairs_knn(a["x"], a["N"], a["D"], a["k"], a["radius2"], a["ws"], a["ws_bytes"], None), _err()


def call_cover(**kw):
    a = dict(q=FAKE, M=3, ref=FAKE, N=5, D=48, radius2=FAKE, count=FAKE, nearest2=FAKE, nearest_idx=FAKE, ws=FAKE, ws_bytes=None)
    a.update(kw)
    _ws(a, a["M"], a["N"])
    return _lib.lib().dhw_pairs_cover(a["q"], a["M"], a["ref"], a["N"], a["D"], a["radius2"], a["count"], a["nearest2"], a["nearest_idx"], a["ws"],
                                      a["ws_bytes"], None), _err()


def call_polysum(**kw):
    a = dict(x=FAKE, M=3, y=FAKE, N=5, D=48, skip_diag=0, out=FAKE, ws=FAKE, ws_bytes=None)
    a.update(kw)
    _ws(a, a["M"], a["N"])
    return _lib.lib().dhw_pairs_polysum(a["x"], a["M"], a["y"], a["N"], a["D"], a["skip_diag"], a["out"], a["ws"], a["ws_bytes"], None), _err()


BAD_D = [(dict(D=8), r"\bD must be"), (dict(D=24), r"\bD must be"), (dict(D=2064), r"\bD must be")]
BAD_WS = [(dict(ws=None), "ws is NULL"), (dict(ws=FAKE + 8), "ws must be 16-byte aligned"), (dict(ws_bytes=1023), "ws_bytes")]
BAD = (
    [(call_pool, b, n) for b, n in BAD_D + [
        (dict(N=0), r"\bN must be"), (dict(N=16385), r"\bN must be"), (dict(S=0), r"\bS must be"), (dict(S=65), r"\bS must be"),
        (dict(N=16384, S=64, D=2048), "N S D"), (dict(feat=None), "feat is NULL"), (dict(out=None), "out is NULL"),
        (dict(feat=FAKE + 4), "feat must be 16-byte aligned"), (dict(out=FAKE + 8), "out must be 16-byte aligned")]] +
    [(call_knn, b, n) for b, n in BAD_D + BAD_WS + [
        (dict(N=0), r"\bN must be"), (dict(N=16385), r"\bN must be"), (dict(k=0), r"\bk must be"), (dict(k=9, N=20), r"\bk must be"),
        (dict(k=5), r"\bk must be.*below N"), (dict(k=1, N=1), r"\bk must be.*below N"),
        (dict(x=None), "x is NULL"), (dict(radius2=None), "radius2 is NULL"), (dict(x=FAKE + 8), "x must be 16-byte aligned"),
        (dict(radius2=FAKE + 8), "radius2 must be 16-byte aligned")]] +
    [(call_cover, b, n) for b, n in BAD_D + BAD_WS + [
        (dict(M=0), r"\bM must be"), (dict(M=16385), r"\bM must be"), (dict(N=0), r"\bN must be"), (dict(N=16385), r"\bN must be"),
        (dict(radius2=None), "radius2 and count must both.*radius2 is NULL"), (dict(count=None), "radius2 and count must both.*count is NULL"),
        (dict(q=None), "q is NULL"), (dict(ref=None), "ref is NULL"), (dict(nearest2=None), "nearest2 is NULL"),
        (dict(q=FAKE + 8), "q must be 16-byte aligned"), (dict(ref=FAKE + 8), "ref must be 16-byte aligned"),
        (dict(radius2=FAKE + 8), "radius2 must be 16-byte aligned"), (dict(count=FAKE + 4), "count must be 16-byte aligned"),
        (dict(nearest2=FAKE + 8), "nearest2 must be 16-byte aligned"), (dict(nearest_idx=FAKE + 4), "nearest_idx must be 16-byte aligned")]] +
    [(call_polysum, b, n) for b, n in BAD_D + BAD_WS + [
        (dict(M=0), r"\bM must be"), (dict(M=16385), r"\bM must be"), (dict(N=0), r"\bN must be"), (dict(N=16385), r"\bN must be"),
        (dict(skip_diag=1), "skip_diag needs M == N"), (dict(x=None), "x is NULL"), (dict(y=None), "y is NULL"), (dict(out=None), "out is NULL"),
        (dict(x=FAKE + 8), "x must be 16-byte aligned"), (dict(y=FAKE + 8), "y must be 16-byte aligned"),
        (dict(out=FAKE + 8), "out must be 16-byte aligned")]])


@pytest.mark.parametrize("fn,bad,name", BAD, ids=[f"{f.__name__[5:]}-{'-'.join(f'{k}={v}' for k, v in b.items())}" for f, b, _ in BAD])
def test_each_argument_rule_answers_without_a_gpu(fn, bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = fn(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith(f"dhw_pairs_{fn.__name__[5:]}:"), (bad, msg)


def test_kernel_constants_match_the_wrapper():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "pairs", "pairs.h")).read()
    for name in ("PAIRS_MAX_N", "PAIRS_MAX_K"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(quality, name)


# ---------------------------------------------------------------- Python refusals, before any device access
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


def test_feature_set_refusals_before_any_device_access(monkeypatch):
    _no_device(monkeypatch)
    for bad in (8, 24, 2064, 0, 48.0, True):
        with pytest.raises(ValueError, match="D = "):
            dhg_amd.FeatureSet(bad)
    s = dhg_amd.FeatureSet(48)
    assert s.count == 0 and tuple(s.data.shape) == (0, 48) and s.data.dtype == torch.float64
    with pytest.raises(ValueError, match=r"features must be floating-point \[N, S, 48\]"):
        s.update(np.zeros((3, 2, 32), np.float32))
    with pytest.raises(ValueError, match="S = 65"):
        s.update(np.zeros((3, 65, 48), np.float32))
    for v in (np.nan, np.inf, -np.inf):
        x = np.zeros((3, 48), np.float32)
        x[1, 7] = v
        with pytest.raises(ValueError, match="non-finite"):
            s.update(x)
    with pytest.raises(ValueError, match="at most 16384 rows"):
        s.update(torch.zeros(16385, 48))
    full = dhg_amd.FeatureSet.from_rows(np.zeros((16380, 48)))
    with pytest.raises(ValueError, match="at most 16384 rows"):
        full.update(torch.zeros(5, 48))
    with pytest.raises(ValueError, match="at most 16384 rows"):
        dhg_amd.FeatureSet.from_rows(np.zeros((16385, 16)))
    with pytest.raises(ValueError, match="non-finite"):
        dhg_amd.FeatureSet.from_rows(np.full((2, 16), np.nan))
    assert s.count == 0 and s.update(np.zeros((0, 48), np.float32)) is s


def test_metric_refusals_before_any_device_access(monkeypatch):
    _no_device(monkeypatch)
    g = np.random.Generator(np.random.PCG64(1))
    a, b, one = (dhg_amd.FeatureSet.from_rows(g.normal(size=(n, 48))) for n in (5, 4, 1))
    other = dhg_amd.FeatureSet.from_rows(g.normal(size=(5, 32)))
    for k in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="k = "):
            dhg_amd.knn_radius(a, k)
    with pytest.raises(ValueError, match="k = 5 needs more than 5 rows"):
        dhg_amd.knn_radius(a, 5)
    with pytest.raises(ValueError, match="k = 4 needs more than 4 rows"):
        dhg_amd.precision_recall(a, b, 4)
    with pytest.raises(ValueError, match="expected a FeatureSet"):
        dhg_amd.nearest(np.zeros((3, 48)), a)
    with pytest.raises(ValueError, match="different dimensions"):
        dhg_amd.nearest(a, other)
    with pytest.raises(ValueError, match="fewer than 1"):
        dhg_amd.nearest(dhg_amd.FeatureSet(48), a)
    with pytest.raises(ValueError, match="fewer than 2"):
        dhg_amd.kernel_distance(a, one)
    data = {"strokes": torch.zeros(4, 16, 3), "text": torch.ones(4, 3, dtype=torch.int64), "style": torch.zeros(4, 14, 1280)}
    with pytest.raises(TypeError, match="sample_metrics: unknown sampler keyword.*temperature.*for sample "):
        dhg_amd.sample_metrics(None, data, None, temperature=2.0)
    with pytest.raises(ValueError, match="k = 9"):
        dhg_amd.sample_metrics(None, data, None, k=9)
    with pytest.raises(ValueError, match="n = "):
        dhg_amd.sample_metrics(None, data, None, n=5)
    with pytest.raises(ValueError, match="real must be a FeatureSet"):
        dhg_amd.sample_metrics(None, data, None, real=dhg_amd.FeatureStats(1280))
    with pytest.raises(ValueError, match="real must be a FeatureStats"):
        dhg_amd.sample_metrics(None, data, None, real=(a, a))


def test_feature_set_without_a_device(tmp_path):
    rows = np.random.Generator(np.random.PCG64(2)).normal(size=(7, 48))
    s = dhg_amd.FeatureSet.from_rows(rows)
    assert s.count == 7 and s.D == 48 and np.array_equal(s.data.numpy(), rows) and np.array_equal(s.rows(), rows)
    s.save(tmp_path / "set.npz")
    assert sorted(np.load(tmp_path / "set.npz").files) == ["rows"]
    back = dhg_amd.FeatureSet.load(tmp_path / "set.npz")
    assert back.count == 7 and np.array_equal(back.rows().view(np.int64), rows.view(np.int64))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs an MI355X"):
            s.update(np.zeros((2, 48), np.float32))
        with pytest.raises(RuntimeError, match="needs an MI355X"):
            dhg_amd.knn_radius(s, 3)


# ---------------------------------------------------------------- closed forms of the reference
def test_reference_closed_forms():
    g = np.random.Generator(np.random.PCG64(3))
    x = g.normal(size=(40, 16))
    m = pairs_ref.metrics(x, x, 3)                      # every row lies in its own ball (d2 = 0 <= radius)
    assert m["precision"] == m["recall"] == m["coverage"] == 1.0 and m["density"] >= 1.0 / 3
    far = x + 1e3                                        # farther apart than every radius
    assert max(pairs_ref.radius(x, 3).max(), pairs_ref.radius(far, 3).max()) < pairs_ref.d2(x, far).min()
    assert pairs_ref.metrics(x, far, 3) == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    # every generated row equals real row 5: it lies in that row's ball (precision 1); the generated balls have radius 0, so a real
    # row is recalled only if it equals row 5: recall = 1 / N (rows within that ball)
    gen = np.repeat(x[5:6], 9, axis=0)
    m = pairs_ref.metrics(x, gen, 3)
    assert (pairs_ref.radius(gen, 3) == 0).all()
    assert m["precision"] == 1.0 and m["recall"] == 1.0 / 40 and 0 < m["coverage"] <= 1
    # radius by index: a duplicated row has radius 0 at k = 1 and the plain nearest-neighbour distance otherwise
    y = np.vstack([x[:5], x[2:3]])
    r = pairs_ref.radius(y, 1)
    assert r[2] == 0 and r[5] == 0 and (r[[0, 1, 3, 4]] > 0).all()
    count, near, idx = pairs_ref.cover(y, x[:5], pairs_ref.radius(x[:5], 1))
    assert near[5] == 0 and idx[5] == 2 and list(idx[:5]) == [0, 1, 2, 3, 4]
    # the cubic sum and KID
    a, b = g.normal(size=(6, 16)), g.normal(size=(4, 16))
    want = sum((a[i] @ b[j] + 16) ** 3 for i in range(6) for j in range(4))
    assert abs(pairs_ref.polysum(a, b) - want) <= 1e-12 * abs(want)
    want = sum((a[i] @ a[j] + 16) ** 3 for i in range(6) for j in range(6) if i != j)
    assert abs(pairs_ref.polysum(a, a, True) - want) <= 1e-12 * abs(want)
    kxx = pairs_ref.polysum(a, a, True) / 30
    kyy = pairs_ref.polysum(b, b, True) / 12
    kxy = pairs_ref.polysum(a, b) / 24
    assert abs(pairs_ref.kid(a, b) - (kxx + kyy - 2 * kxy) / 16 ** 3) <= 1e-12 * kxx / 16 ** 3
    two = g.normal(size=(400, 16))
    assert abs(pairs_ref.kid(two[:200], two[200:])) < 0.05 * pairs_ref.kid(two[:200], two[200:] + 1.0)   # same law: near 0


def test_reference_pooling_is_the_moments_rule():
    import moments_ref
    feat = np.random.Generator(np.random.PCG64(4)).normal(size=(5, 3, 16)).astype(np.float32)
    assert np.array_equal(pairs_ref.pool(feat), moments_ref.pool(feat))


# ---------------------------------------------------------------- tools/eval_samples.py --metrics
def test_eval_samples_metrics_flag_parses():
    spec_ = importlib.util.spec_from_file_location("eval_samples_mod", os.path.join(ROOT, "tools", "eval_samples.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    a = mod.parser().parse_args(["--data", "x.pt", "--metrics", "--k", "5", "--guidance", "1.5", "2.5"])
    assert a.metrics is True and a.k == 5 and a.guidance == [1.5, 2.5]
    a = mod.parser().parse_args(["--data", "x.pt"])
    assert a.metrics is False and a.k == 3
    for argv in (["--data", "x.pt", "--metrics", "--real-stats", "r.npz"], ["--data", "x.pt", "--metrics", "--k", "9"]):
        with pytest.raises(SystemExit):
            mod.main(argv)
