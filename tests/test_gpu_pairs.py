"""Pairwise metrics on the GPU (include/dhw.h dhw_pairs_*, dhg_amd.FeatureSet / knn_radius / nearest / precision_recall /
kernel_distance) against tests/pairs_ref.py.

Harness: every output and the workspace lie between canaries, every input has NaN rows behind its last row, and every call runs
twice in fresh buffers with the same bits required.

Exact data: the integer features of test_gpu_moments.py (column d drawn from its own range) pooled with S in {1, 2}: every pooled
value is a multiple of 1/2, every product a multiple of 1/4 and every d2 far below 2^53, so radius2, count, nearest2 and
nearest_idx must equal the reference bit for bit in any order of summation.  Every cube is a multiple of 1 / S^6, so the cube sum is
exact in any order while S^6 sum |x.y + D|^3 < 2^53.  The test computes that sum: at most 2.6e10 at the D = 48 shapes and 9.5e14 at
(130, 67, 1280), so the condition holds everywhere but at D = 1280 with S = 2 (64 x 8.0e14 > 2^53); polysum must equal the reference
bit for bit where it holds and stay within the derived bound below in that one case.  The query set and the reference set differ in
size in every case, so a swapped row / column map cannot pass.

Ties: binary features, X 67 x 16 and Y 37 x 16 from PCG64(7), X[66] = X[0] (two rows of radius 0 at k = 1: exclusion is by index) and
Y[5] = X[3] (a query equal to a reference row).  Computed with the reference: 41 pairs with d2 == radius2; precision 0.865 with <=
and 0.459 with <, recall 0.776 against 0.403: the comparison operator is pinned.

Real-valued data: clipped normals of test_gpu_moments.real_features, S = 14, N = 67 real rows and M = 53 generated rows whose features
are shifted by 0.15 (D = 48) / 0.05 (D = 1280).  Reference values: precision 0.47 / 0.49, recall 0.43 / 0.60, coverage 0.55 / 0.55.
Per pair b_ij = (D + 8) 2^-53 . 2 (sq_i + sq_j) bounds the expanded form against the direct one; an order statistic is 1-Lipschitz in
the sup norm, so |radius2 - ref| <= max_j b_ij and likewise nearest2.  The test asserts on the reference that no pair lies within b of
its threshold (smallest gap: 1.4e9 b at D = 48, 3.4e7 b at D = 1280) and that the two nearest neighbours of a query differ by more
than their bounds (4.5e8 and 1.9e6 times), and then demands count and nearest_idx to be equal.
polysum: |got - ref| <= (3 D + M N + 16) 2^-53 sum_ij (sum_d |x_id y_jd| + D)^3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_ref  # noqa: E402
from test_gpu_moments import int_features, real_features  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 32            # canary elements on each side of every output and of the workspace
CANARY = -1234.5
EXTRA_ROWS = 3        # NaN rows behind the last row of every input: never read


class Guarded:
    """A device buffer of n elements between GUARD canaries on each side."""

    def __init__(self, n, dtype=torch.float64):
        self.n = n
        self.t = torch.full((n + 2 * GUARD,), CANARY if dtype.is_floating_point else -12345, dtype=dtype, device="cuda")
        self.canary = self.t[0].item()

    @property
    def ptr(self):
        return self.t[GUARD:].data_ptr()

    def read(self):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.canary).all() and (a[GUARD + self.n:] == self.canary).all(), "a canary was overwritten"
        return a[GUARD:GUARD + self.n].copy()


def padded(x, dtype):
    """x on the device with EXTRA_ROWS NaN rows behind it."""
    x = np.asarray(x)
    p = np.full((x.shape[0] + EXTRA_ROWS,) + x.shape[1:], np.nan, dtype)
    p[:x.shape[0]] = x
    return torch.from_numpy(p).cuda()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def twice(fn):
    """fn() twice in fresh buffers: the same bits both times."""
    first, second = fn(), fn()
    for a, b in zip(first, second):
        assert (a is None and b is None) or same_bits(a, b), "the same call gave other bits"
    return first


def workspace(M, N, D):
    need = int(_lib.lib().dhw_pairs_workspace_bytes(M, N, D))
    assert need > 0 and need % 8 == 0
    return Guarded(need // 8), need


def gpu_pool(feat):
    def run():
        N, S, D = feat.shape
        out = Guarded(N * D)
        x = padded(feat, np.float32)
        _lib.check(_lib.lib().dhw_pairs_pool(x.data_ptr(), N, S, D, out.ptr, stream()))
        torch.cuda.synchronize()
        return (out.read().reshape(N, D),)
    return twice(run)[0]


def gpu_knn(x, k):
    def run():
        N, D = x.shape
        out, (ws, need) = Guarded(N), workspace(N, N, D)
        xd = padded(x, np.float64)
        _lib.check(_lib.lib().dhw_pairs_knn(xd.data_ptr(), N, D, k, out.ptr, ws.ptr, need, stream()))
        torch.cuda.synchronize()
        ws.read()
        return (out.read(),)
    return twice(run)[0]


def gpu_cover(q, ref, radius2=None, want_idx=True):
    def run():
        (M, D), N = q.shape, ref.shape[0]
        near, idx, (ws, need) = Guarded(M), Guarded(M, torch.int32), workspace(M, N, D)
        count = Guarded(M, torch.int32) if radius2 is not None else None
        rad = padded(radius2, np.float64) if radius2 is not None else None
        qd, refd = padded(q, np.float64), padded(ref, np.float64)      # (named: both stay allocated through the call)
        _lib.check(_lib.lib().dhw_pairs_cover(qd.data_ptr(), M, refd.data_ptr(), N, D,
                                              None if rad is None else rad.data_ptr(), None if count is None else count.ptr, near.ptr,
                                              idx.ptr if want_idx else None, ws.ptr, need, stream()))
        torch.cuda.synchronize()
        ws.read()
        got_idx = idx.read()
        if not want_idx:
            assert (got_idx == idx.canary).all()
        return None if count is None else count.read(), near.read(), got_idx if want_idx else None
    return twice(run)


def gpu_polysum(x, y, skip_diag=False):
    def run():
        (M, D), N = x.shape, y.shape[0]
        out, (ws, need) = Guarded(1), workspace(M, N, D)
        xd, yd = padded(x, np.float64), padded(y, np.float64)
        _lib.check(_lib.lib().dhw_pairs_polysum(xd.data_ptr(), M, yd.data_ptr(), N, D, int(skip_diag), out.ptr, ws.ptr, need, stream()))
        torch.cuda.synchronize()
        ws.read()
        return (out.read(),)
    return float(twice(run)[0][0])


# ---------------------------------------------------------------- exact data
REF = {}


def exact_case(N, M, D, S):
    """Pooled integer sets and their reference results: computed once, shared, never changed."""
    key = (N, M, D, S)
    if key not in REF:
        fx, fy = int_features(N, S, D, 1), int_features(M, S, D, 2)
        X, Y = pairs_ref.pool(fx), pairs_ref.pool(fy)
        for a in (fx, fy, X, Y):
            a.setflags(write=False)
        REF[key] = (fx, fy, X, Y)
    return REF[key]


def cube_sum_is_exact(x, y, S):
    """S^6 sum |x.y + D|^3 < 2^53: every cube is a multiple of 1 / S^6, so every partial sum in any order is exactly representable."""
    t = np.abs(x @ y.T + x.shape[1])
    return float(S) ** 6 * float((t * t * t).sum()) < 2.0 ** 53


EXACT_SHAPES = [(2, 1, 16, (1,)), (5, 3, 48, (1, 3)), (65, 64, 48, (3,)), (67, 37, 48, (1, 3, 8)), (130, 67, 1280, (3,))]


def check_exact(N, M, D, ks, S):
    fx, fy, X, Y = exact_case(N, M, D, S)
    assert same_bits(gpu_pool(fx), X) and same_bits(gpu_pool(fy), Y)
    for k in ks:
        want_r = pairs_ref.radius(X, k)
        got_r = gpu_knn(X, k)
        assert same_bits(got_r, want_r), (k, np.argwhere(got_r != want_r)[:8])
        want = pairs_ref.cover(Y, X, want_r)
        got = gpu_cover(Y, X, want_r)
        for name, g, w in zip(("count", "nearest2", "nearest_idx"), got, want):
            assert same_bits(g, w), (name, k, np.argwhere(g != w)[:8])
    none, near, no_idx = gpu_cover(Y, X, None, want_idx=False)
    assert none is None and no_idx is None and same_bits(near, pairs_ref.cover(Y, X)[1])
    for a, b, skip in ((Y, X, False), (X, X, True), (X, Y, False)):
        got, want = gpu_polysum(a, b, skip), pairs_ref.polysum(a, b, skip)
        if cube_sum_is_exact(a, b, S):
            assert got == want, (a.shape, b.shape, skip, got, want)
        else:
            assert (D, S) == (1280, 2) and abs(got - want) <= pairs_ref.polysum_bound(a, b), (got, want)


def test_the_cube_sum_is_exact_where_the_test_says():
    for N, M, D, _ in EXACT_SHAPES + [(37, 67, 48, None)]:
        for S in (1, 2):
            _, _, X, Y = exact_case(N, M, D, S)
            for a, b in ((Y, X), (X, X), (X, Y)):
                assert cube_sum_is_exact(a, b, S) == ((D, S) != (1280, 2))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("N,M,D,ks", EXACT_SHAPES)
def test_exact_data_bit_for_bit(N, M, D, ks, S):
    check_exact(N, M, D, ks, S)


@pytest.mark.parametrize("split", ["1", "3"])
def test_exact_data_with_forced_splits(monkeypatch, split):
    """67 reference rows are two 64-column chunks: 1 split walks both in one workgroup, 3 is clipped to one chunk per split."""
    monkeypatch.setenv("DHW_PAIRS_SPLIT", split)
    check_exact(67, 37, 48, (1, 3, 8), 2)
    check_exact(37, 67, 48, (3,), 1)


# ---------------------------------------------------------------- ties
def test_ties_pin_the_comparison_and_exclusion_by_index():
    g = np.random.Generator(np.random.PCG64(7))
    X = g.integers(0, 2, size=(67, 16)).astype(np.float64)
    Y = g.integers(0, 2, size=(37, 16)).astype(np.float64)
    X[66], Y[5] = X[0], X[3]
    r = pairs_ref.radius(X, 1)
    d = pairs_ref.d2(Y, X)
    strict = float(((d < r[None]).sum(1) > 0).mean())
    assert r[0] == r[66] == 0 and int((d == r[None]).sum()) == 41 and d[5, 3] == 0
    got_r = gpu_knn(X, 1)
    assert same_bits(got_r, r)
    count, near, idx = gpu_cover(Y, X, r)
    want = pairs_ref.cover(Y, X, r)
    assert same_bits(count, want[0]) and same_bits(near, want[1]) and same_bits(idx, want[2])
    assert near[5] == 0 and idx[5] == 3
    precision = float((count > 0).mean())
    print(f"precision with <= {precision:.3f}, with < {strict:.3f}")
    assert abs(precision - 0.865) < 1e-3 and abs(strict - 0.459) < 1e-3
    c0, n0, i0 = gpu_cover(X, X, r)                       # a set against itself: every row is its own nearest at distance 0 <= radius
    assert (n0 == 0).all() and (c0 >= 1).all() and i0[66] == 0 and (i0[:66] == np.arange(66)).all()
    for k in (2, 8):
        assert same_bits(gpu_knn(X, k), pairs_ref.radius(X, k))


# ---------------------------------------------------------------- real-valued data
REAL = {}


def real_case(D):
    if D not in REAL:
        shift = np.float32(0.15 if D == 48 else 0.05)
        X = pairs_ref.pool(real_features(67, 14, D, 3))
        Y = pairs_ref.pool(real_features(53, 14, D, 4) + shift)
        for a in (X, Y):
            a.setflags(write=False)
        REAL[D] = (X, Y)
    return REAL[D]


@pytest.mark.parametrize("D", [48, 1280])
def test_real_valued_data_within_the_derived_bounds(D):
    X, Y = real_case(D)
    k = 3
    m = pairs_ref.metrics(X, Y, k)
    assert all(0.2 < m[n] < 0.8 for n in ("precision", "recall", "coverage")), m
    bxx, byx = pairs_ref.pair_bound(X, X), pairs_ref.pair_bound(Y, X)
    r = pairs_ref.radius(X, k)
    got_r = gpu_knn(X, k)
    e_r = float((np.abs(got_r - r) / bxx.max(1)).max())
    d = pairs_ref.d2(Y, X)
    gap_cover = float((np.abs(d - r[None]) / byx).min())
    order = np.argsort(d, axis=1)[:, :2]
    two = np.take_along_axis(d, order, 1)
    gap_near = float(((two[:, 1] - two[:, 0]) / np.take_along_axis(byx, order, 1).sum(1)).min())
    assert gap_cover > 1 and gap_near > 1, "a pair of the reference lies within the bound of its threshold"
    want = pairs_ref.cover(Y, X, r)
    count, near, idx = gpu_cover(Y, X, r)
    e_n = float((np.abs(near - want[1]) / byx.max(1)).max())
    errs = {}
    for name, a, b, skip in (("yx", Y, X, False), ("xx", X, X, True), ("yy", Y, Y, True)):
        errs[name] = abs(gpu_polysum(a, b, skip) - pairs_ref.polysum(a, b, skip)) / pairs_ref.polysum_bound(a, b)
    print(f"D = {D}: largest error / bound: radius2 {e_r:.3e}, nearest2 {e_n:.3e}, polysum " + ", ".join(f"{n} {v:.3e}" for n, v in errs.items()) +
          f"; smallest gap / bound: cover {gap_cover:.3e}, two nearest {gap_near:.3e}")
    assert e_r <= 1 and e_n <= 1 and all(v <= 1 for v in errs.values())
    assert same_bits(count, want[0]) and same_bits(idx, want[2])


# ---------------------------------------------------------------- the Python layer
def test_feature_set_takes_pooled_and_unpooled_inputs_and_pools_as_the_moments_do():
    feat = real_features(21, 1, 48, 4)
    a = dhg_amd.FeatureSet(48).update(torch.from_numpy(feat[:, 0]))          # [N,D], from the host
    b = dhg_amd.FeatureSet(48).update(torch.from_numpy(feat).cuda())         # [N,1,D], on the device
    assert a.count == b.count == 21 and a.device.type == "cuda" and a.data.is_cuda and a.data.dtype == torch.float64
    assert same_bits(a.rows(), b.rows()) and same_bits(a.rows(), feat[:, 0].astype(np.float64))
    # the pooled matrix dhw_moments_update leaves in its workspace
    feat = real_features(21, 14, 48, 5)
    l = _lib.lib()
    need = int(l.dhw_moments_workspace_bytes(21, 14, 48))
    state, ws = torch.zeros(48 + 48 * 48, dtype=torch.float64, device="cuda"), torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    _lib.check(l.dhw_moments_update(torch.from_numpy(feat).cuda().data_ptr(), 21, 14, 48, state.data_ptr(), state[48:].data_ptr(), ws.data_ptr(), need,
                                    stream()))
    torch.cuda.synchronize()
    s = dhg_amd.FeatureSet(48).update(feat[:8]).update(feat[8:])
    assert s.count == 21 and same_bits(s.rows(), ws.cpu().numpy().reshape(21, 48)) and same_bits(s.rows(), pairs_ref.pool(feat))
    with pytest.raises(ValueError, match="non-finite"):
        s.update(torch.full((2, 48), float("nan"), device="cuda"))
    assert s.count == 21
    grown = dhg_amd.FeatureSet(48)
    big = int_features(300, 1, 48, 6)
    grown.update(big[:250]).update(big[250:])                              # past the first capacity of 256 rows
    assert grown.count == 300 and same_bits(grown.rows(), pairs_ref.pool(big))


def test_metrics_against_the_reference(tmp_path):
    _, _, X, Y = exact_case(67, 37, 48, 2)
    real, gen = dhg_amd.FeatureSet.from_rows(X), dhg_amd.FeatureSet.from_rows(Y)
    for k in (1, 3):
        assert same_bits(dhg_amd.knn_radius(real, k).cpu().numpy(), pairs_ref.radius(X, k))
        assert dhg_amd.precision_recall(real, gen, k) == pairs_ref.metrics(X, Y, k)
    d2, idx = dhg_amd.nearest(gen, real)
    want = pairs_ref.cover(Y, X)
    assert idx.dtype == torch.int32 and same_bits(d2.cpu().numpy(), want[1]) and same_bits(idx.cpu().numpy(), want[2])
    kid, ref = dhg_amd.kernel_distance(real, gen), pairs_ref.kid(X, Y)
    assert abs(kid - ref) <= 1e-12 * abs(ref)
    ones = dhg_amd.precision_recall(real, real, 3)
    assert ones["precision"] == ones["recall"] == ones["coverage"] == 1.0 and ones["density"] >= 1.0 / 3
    for D in (48, 1280):
        X, Y = real_case(D)
        real, gen = dhg_amd.FeatureSet.from_rows(X), dhg_amd.FeatureSet.from_rows(Y)
        kid, ref = dhg_amd.kernel_distance(real, gen), pairs_ref.kid(X, Y)
        print(f"D = {D}: KID {kid:.6g}, relative error {abs(kid - ref) / abs(ref):.2e}")
        assert abs(kid - ref) <= 1e-12 * abs(ref)
        assert dhg_amd.precision_recall(real, gen, 3) == pairs_ref.metrics(X, Y, 3)
    real.save(tmp_path / "real.npz")
    assert same_bits(dhg_amd.FeatureSet.load(tmp_path / "real.npz").rows(), X)


def test_the_entries_can_be_captured_into_a_graph():
    """No allocation and no synchronisation inside the entries: knn -> cover -> polysum on one stream, captured and replayed."""
    _, _, X, Y = exact_case(67, 37, 48, 2)
    l = _lib.lib()
    xd, yd = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(Y.copy()).cuda()
    need = max(int(l.dhw_pairs_workspace_bytes(67, 67, 48)), int(l.dhw_pairs_workspace_bytes(37, 67, 48)))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    r, near, acc = (torch.zeros(n, dtype=torch.float64, device="cuda") for n in (67, 37, 2))
    count, idx = (torch.zeros(37, dtype=torch.int32, device="cuda") for _ in range(2))

    def calls():
        s = stream()
        _lib.check(l.dhw_pairs_knn(xd.data_ptr(), 67, 48, 3, r.data_ptr(), ws.data_ptr(), need, s))
        _lib.check(l.dhw_pairs_cover(yd.data_ptr(), 37, xd.data_ptr(), 67, 48, r.data_ptr(), count.data_ptr(), near.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                     need, s))
        _lib.check(l.dhw_pairs_polysum(yd.data_ptr(), 37, xd.data_ptr(), 67, 48, 0, acc.data_ptr(), ws.data_ptr(), need, s))

    calls()                                                             # (the kernels are loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    for t in (r, near, acc, count, idx):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want_r = pairs_ref.radius(X, 3)
    want = pairs_ref.cover(Y, X, want_r)
    assert same_bits(r.cpu().numpy(), want_r) and same_bits(count.cpu().numpy(), want[0]) and same_bits(near.cpu().numpy(), want[1])
    assert same_bits(idx.cpu().numpy(), want[2]) and float(acc[0]) == pairs_ref.polysum(Y, X)
