"""Dynamic time warping on the GPU (include/dhw.h dhw_dtw; dhg_amd.stroke_features / dtw_distance / nearest_strokes /
sample_metrics(dtw=True)) against tests/dtw_ref.py, the numpy float32 statement of the pair rules.

Harness (that of test_gpu_pairs.py): every output and the workspace lie between canaries, every line has NaN rows behind its
length and every set NaN lines behind its last line, and every call runs twice in fresh buffers with the same bits required.

Everything is compared bit for bit: every cell is a fixed sequence of float32 operations (difference, product, sum over f
ascending, three-way minimum, one addition) in a fixed dependence order, so there is nothing for a tolerance to absorb but a
fused multiply-add or another tie order.
  Exact integers: features in [-7, 7], so a cell costs at most 196 F and every D is an integer of at most 196 F (La + Lb - 1)
    (a path has at most La + Lb - 1 cells): the test computes that bound and checks it against 2^24.
  Ties: binary features (tests/test_dtw_cpu.tie_data): the path length depends on the predecessor order of rule 5 in at least a
    quarter of the pairs (asserted on the reference), the distance does not.
  Real-valued: normals; dist, steps and the normalised dist.
A duplicated line in a set against itself: without skip_diag every distance is 0 and a row's index is its own, except the later
copy's, which is the earlier copy (rule 8: the smallest index attaining the minimum); with skip_diag the copies find each other."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_ref  # noqa: E402
from test_dtw_cpu import TIE_LENS_A, TIE_LENS_B, tie_data  # noqa: E402
from test_gpu_pairs import Guarded, same_bits, stream, twice  # noqa: E402

pytestmark = pytest.mark.gpu

EXTRA = 2   # NaN lines behind the last line of every set, garbage entries behind the last length


def padded_lines(x, lens):
    """x [M,L,F] on the device: NaN in every row at or past its line's length and EXTRA NaN lines behind the last line."""
    x = np.asarray(x, np.float32)
    p = np.full((x.shape[0] + EXTRA,) + x.shape[1:], np.nan, np.float32)
    p[:x.shape[0]] = x
    if lens is not None:
        for i, n in enumerate(lens):
            p[i, max(int(n), 0):] = np.nan
    return torch.from_numpy(p).cuda()


def device_lens(lens):
    return None if lens is None else torch.from_numpy(np.concatenate([np.asarray(lens, np.int32), np.full(EXTRA, 7777, np.int32)])).cuda()


def gpu_dtw(a, lens_a, b, lens_b, normalize=False, skip_diag=False, want=("dist", "steps", "near", "idx")):
    """dhw_dtw twice in fresh guarded buffers -> {name: array or None}."""
    (M, La, F), (N, Lb, _) = np.shape(a), np.shape(b)
    l = _lib.lib()

    def run():
        need = int(l.dhw_dtw_workspace_bytes(M, N, La, Lb, F))
        assert need >= 4 * M * N and need % 16 == 0
        ws = Guarded(need // 4, torch.float32)
        out = {"dist": Guarded(M * N, torch.float32), "steps": Guarded(M * N, torch.int32), "near": Guarded(M, torch.float32), "idx": Guarded(M, torch.int32)}
        ad, bd, la, lb = padded_lines(a, lens_a), padded_lines(b, lens_b), device_lens(lens_a), device_lens(lens_b)
        ptr = lambda name: out[name].ptr if name in want else None   # noqa: E731
        _lib.check(l.dhw_dtw(ad.data_ptr(), None if la is None else la.data_ptr(), M, La, bd.data_ptr(), None if lb is None else lb.data_ptr(), N, Lb, F,
                             int(normalize), int(skip_diag), ptr("dist"), ptr("steps"), ptr("near"), ptr("idx"), ws.ptr, need, stream()))
        torch.cuda.synchronize()
        ws.read()
        res = []
        for name in ("dist", "steps", "near", "idx"):
            got = out[name].read()
            if name not in want:
                assert (got == out[name].canary).all(), f"{name} was written without being asked for"
            res.append(got.reshape(M, N) if name in ("dist", "steps") and name in want else got if name in want else None)
        return res
    return dict(zip(("dist", "steps", "near", "idx"), twice(run)))


def check_against_reference(a, lens_a, b, lens_b, normalize=False, skip_diag=False):
    want_d, want_k = dtw_ref.dtw_batch(a, lens_a, b, lens_b, normalize)
    want_n, want_i = dtw_ref.nearest(want_d, skip_diag)
    got = gpu_dtw(a, lens_a, b, lens_b, normalize, skip_diag)
    assert same_bits(got["steps"], want_k), np.argwhere(got["steps"] != want_k)[:8]
    assert same_bits(got["dist"], want_d), np.argwhere(got["dist"] != want_d)[:8]
    assert same_bits(got["near"], want_n) and same_bits(got["idx"], want_i), (got["near"], want_n, got["idx"], want_i)
    return got


def int_lines(M, L, F, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(-7, 8, size=(M, L, F)).astype(np.float32)


def mixed_lengths(count, L, first, seed):
    """Lengths in which 1, 2 and the full L stand next to one another (the chained-query reset), then random ones."""
    g = np.random.Generator(np.random.PCG64(seed))
    base = [L, 1, min(2, L)]
    base = base[first:] + base[:first]
    return [base[i] if i < 3 else int(g.integers(1, L + 1)) for i in range(count)]


# ---------------------------------------------------------------- exact integers
EXACT = [(1, 1, 1, 1, 1), (3, 5, 17, 33, 2), (5, 7, 64, 65, 3), (4, 3, 130, 67, 4), (2, 2, 1024, 1024, 3), (3, 2, 1000, 129, 3)]


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("M,N,La,Lb,F", EXACT)
def test_exact_integers_bit_for_bit(M, N, La, Lb, F, ragged):
    a, b = int_lines(M, La, F, 1), int_lines(N, Lb, F, 2)
    largest = float(np.max(np.abs(a)) + np.max(np.abs(b))) ** 2 * F * (La + Lb - 1)
    assert largest < 2.0 ** 24, "a D of this case may not be an exactly representable integer"
    lens_a = mixed_lengths(M, La, 0, 3) if ragged else None
    lens_b = mixed_lengths(N, Lb, 2, 4) if ragged else None      # a: L, 1, 2, ..; b: 2, L, 1, ..
    got = check_against_reference(a, lens_a, b, lens_b)
    assert (got["dist"] == np.rint(got["dist"])).all() and got["dist"].max() <= largest
    if ragged:
        check_against_reference(a, lens_a, b, lens_b, normalize=True)


# ---------------------------------------------------------------- ties
def test_ties_pin_the_predecessor_order():
    a, b = tie_data()
    want_d, want_k = dtw_ref.dtw_batch(a, TIE_LENS_A, b, TIE_LENS_B)
    other = sum(dtw_ref.dtw_loop(a[p, :n], b[q, :m], order=("left", "up", "diag"))[1] != want_k[p, q]
                for p, n in enumerate(TIE_LENS_A) for q, m in enumerate(TIE_LENS_B))
    assert 4 * other >= want_k.size, "the tie data no longer distinguishes the predecessor orders"
    loop_d, loop_k = dtw_ref.dtw_batch(a, TIE_LENS_A, b, TIE_LENS_B, pair=dtw_ref.dtw_loop)
    assert same_bits(loop_d, want_d) and same_bits(loop_k, want_k)
    got = check_against_reference(a, TIE_LENS_A, b, TIE_LENS_B)
    assert same_bits(got["steps"], want_k)
    check_against_reference(a, TIE_LENS_A, b, TIE_LENS_B, normalize=True)


# ---------------------------------------------------------------- real-valued data
REAL = {}


def real_case():
    """Normals, F = 3, M = 6 lines against N = 9 of ragged lengths up to 200, and the reference results: computed once, shared."""
    if not REAL:
        g = np.random.Generator(np.random.PCG64(21))
        a, b = g.normal(size=(6, 200, 3)).astype(np.float32), g.normal(size=(9, 200, 3)).astype(np.float32)
        la, lb = [200, 1, 2, 57, 130, 199], [2, 200, 1, 64, 65, 3, 128, 129, 77]
        REAL.update(a=a, b=b, la=la, lb=lb, plain=dtw_ref.dtw_batch(a, la, b, lb), norm=dtw_ref.dtw_batch(a, la, b, lb, normalize=True))
        for v in (a, b) + REAL["plain"] + REAL["norm"]:
            v.setflags(write=False)
    return REAL


def test_real_valued_data_bit_for_bit():
    c = real_case()
    for normalize, (want_d, want_k) in ((False, c["plain"]), (True, c["norm"])):
        got = gpu_dtw(c["a"], c["la"], c["b"], c["lb"], normalize)
        assert same_bits(got["steps"], want_k), np.argwhere(got["steps"] != want_k)[:8]
        assert same_bits(got["dist"], want_d), np.argwhere(got["dist"] != want_d)[:8]
        want_n, want_i = dtw_ref.nearest(want_d)
        assert same_bits(got["near"], want_n) and same_bits(got["idx"], want_i)
    assert np.isfinite(c["plain"][0]).all() and (c["plain"][0] > 0).all()


def test_a_pair_alone_has_the_bits_it_has_in_the_batch():
    """The batch holds lines of up to 200 rows (4 columns per lane); alone, a pair runs at its own lengths (other column counts)."""
    c = real_case()
    want_d, want_k = c["norm"]
    for p in (0, 1, 3):
        for q in (0, 2, 3, 5, 8):
            n, m = c["la"][p], c["lb"][q]
            got = gpu_dtw(c["a"][p:p + 1, :n], None, c["b"][q:q + 1, :m], None, True, want=("dist", "steps"))
            assert same_bits(got["dist"], want_d[p:p + 1, q:q + 1]) and same_bits(got["steps"], want_k[p:p + 1, q:q + 1]), (p, q)


# ---------------------------------------------------------------- lengths outside the range
def test_lengths_outside_the_range_give_inf_and_are_skipped_by_nearest():
    a, b = int_lines(5, 20, 3, 5), int_lines(6, 70, 3, 6)
    lens_a, lens_b = [20, 0, 21, 7, -3], [71, 70, 0, 1, 33, 70]
    got = check_against_reference(a, lens_a, b, lens_b, normalize=True)
    assert np.isinf(got["dist"][[1, 2, 4]]).all() and (got["steps"][[1, 2, 4]] == 0).all()
    assert np.isinf(got["dist"][:, [0, 2]]).all() and (got["steps"][:, [0, 2]] == 0).all()
    assert np.isfinite(got["dist"][[0, 3]][:, [1, 3, 4, 5]]).all()
    assert np.isinf(got["near"][[1, 2, 4]]).all() and (got["idx"][[1, 2, 4]] == -1).all() and np.isin(got["idx"][[0, 3]], [1, 3, 4, 5]).all()
    none = check_against_reference(a, lens_a, b[:1], lens_b[:1])          # every reference invalid
    assert np.isinf(none["near"]).all() and (none["idx"] == -1).all()


# ---------------------------------------------------------------- nearest
def test_nearest_prefers_the_smaller_index_and_needs_no_matrix_output():
    b = int_lines(9, 40, 3, 7)
    b[6] = b[2]                                                            # a duplicated reference line
    a = int_lines(4, 33, 3, 8)
    a[1, :] = 0
    a[1, :33] = b[2, :33]                                                  # a query that is a prefix of both copies
    lens_b = [40, 39, 33, 40, 1, 2, 33, 40, 17]
    got = check_against_reference(a, None, b, lens_b)
    assert got["near"][1] == 0 and got["idx"][1] == 2
    alone = gpu_dtw(a, None, b, lens_b, want=("near", "idx"))              # the matrix lies in the workspace
    assert alone["dist"] is None and alone["steps"] is None
    assert same_bits(alone["near"], got["dist"].min(1)) and same_bits(alone["idx"], got["idx"])
    only = gpu_dtw(a, None, b, lens_b, want=("near",))
    assert only["idx"] is None and same_bits(only["near"], got["near"])
    norm = gpu_dtw(a, None, b, lens_b, normalize=True, want=("near", "idx"))
    want_n, want_i = dtw_ref.nearest(dtw_ref.dtw_batch(a, None, b, lens_b, normalize=True)[0])
    assert same_bits(norm["near"], want_n) and same_bits(norm["idx"], want_i)


def test_skip_diag_finds_the_planted_duplicate():
    x = int_lines(7, 30, 3, 9)
    x[5] = x[1]
    lens = [30, 30, 12, 1, 29, 30, 2]
    plain = check_against_reference(x, lens, x, lens)
    assert (plain["near"] == 0).all() and plain["idx"].tolist() == [0, 1, 2, 3, 4, 1, 6]
    skip = check_against_reference(x, lens, x, lens, skip_diag=True)
    assert skip["idx"][1] == 5 and skip["idx"][5] == 1 and skip["near"][1] == skip["near"][5] == 0
    assert (skip["idx"] != np.arange(7)).all() and (np.delete(skip["near"], [1, 5]) > 0).all()


# ---------------------------------------------------------------- graph capture
def test_the_entry_can_be_captured_into_a_graph():
    c = real_case()
    l = _lib.lib()
    a, b = torch.from_numpy(c["a"].copy()).cuda(), torch.from_numpy(c["b"].copy()).cuda()
    la, lb = torch.tensor(c["la"], dtype=torch.int32).cuda(), torch.tensor(c["lb"], dtype=torch.int32).cuda()
    need = int(l.dhw_dtw_workspace_bytes(6, 9, 200, 200, 3))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dist, near = torch.zeros(54, dtype=torch.float32, device="cuda"), torch.zeros(6, dtype=torch.float32, device="cuda")
    steps, idx = torch.zeros(54, dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda")

    def calls():
        _lib.check(l.dhw_dtw(a.data_ptr(), la.data_ptr(), 6, 200, b.data_ptr(), lb.data_ptr(), 9, 200, 3, 1, 0, dist.data_ptr(), steps.data_ptr(),
                             near.data_ptr(), idx.data_ptr(), ws.data_ptr(), need, stream()))

    calls()                                                                # (the kernels are loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    for t in (dist, near, steps, idx):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want_d, want_k = c["norm"]
    want_n, want_i = dtw_ref.nearest(want_d)
    assert same_bits(dist.cpu().numpy().reshape(6, 9), want_d) and same_bits(steps.cpu().numpy().reshape(6, 9), want_k)
    assert same_bits(near.cpu().numpy(), want_n) and same_bits(idx.cpu().numpy(), want_i)


# ---------------------------------------------------------------- the Python layer
def sixteenth_strokes(B, L, seed):
    """Strokes whose dx, dy are multiples of 1/16 in [-4, 4] (every prefix sum is exact in any order) and whose pen is 0 or 1."""
    g = np.random.Generator(np.random.PCG64(seed))
    s = np.empty((B, L, 3), np.float32)
    s[..., :2] = g.integers(-64, 65, size=(B, L, 2)) / 16.0
    s[..., 2] = g.random((B, L)) < 0.1
    return s


def test_stroke_features_against_numpy():
    s = sixteenth_strokes(5, 50, 31)
    s[0, :, 2] = np.array([0.5, 1.5, 2.5, -0.5, 0.49, 0.51, -1.0, 0.0, 1.0, 0.0] * 5)   # rint: half to even
    for kind in ("positions", "offsets"):
        for w in (1.0, 4.0, 0.3):
            got = dhg_amd.stroke_features(s, kind=kind, pen_weight=w)
            assert got.is_cuda and got.dtype == torch.float32 and same_bits(got.cpu().numpy(), dtw_ref.features(s, kind, w)), (kind, w)
    lens = np.array([50, 1, 2, 17, 49])
    dirty = s.copy()
    for i, n in enumerate(lens):
        dirty[i, n:] = np.nan                                              # rows behind a length may hold anything
    got = dhg_amd.stroke_features(torch.from_numpy(dirty).cuda(), lens).cpu().numpy()
    want = dtw_ref.features(s)
    assert all(same_bits(got[i, :n], want[i, :n]) for i, n in enumerate(lens))


def test_pen_weight_is_the_cost_of_a_lift_mismatch_and_positions_see_a_scaling():
    L = 24
    a = np.zeros((1, L, 3), np.float32)
    a[0, :, 0], a[0, :, 1] = 4.0, np.tile([1.0, -1.0], L // 2)          # 4 to the right per row: leaving the diagonal costs >= 16 a cell
    b = a.copy()
    a[0, [3, 9, 20], 2] = 1
    b[0, [9, 14], 2] = 1                                                   # lifts at rows 3, 20 and 14 have no partner: 3 mismatched cells
    for w in (1.0, 4.0):
        dist, steps = dhg_amd.dtw_distance(a, b, pen_weight=w, normalize=False)
        want = dtw_ref.dtw_batch(dtw_ref.features(a, "positions", w), None, dtw_ref.features(b, "positions", w), None)
        assert same_bits(dist.cpu().numpy(), want[0]) and same_bits(steps.cpu().numpy(), want[1])
        assert float(dist[0, 0]) == 3 * w and int(steps[0, 0]) == L
    # a uniform doubling of dx, dy: the rendered picture of a line fills its image at any scale, the positions do not
    s = sixteenth_strokes(3, 40, 32)
    twice_s = s.copy()
    twice_s[..., :2] *= 2
    dist, steps = dhg_amd.dtw_distance(s, twice_s)
    want = dtw_ref.dtw_batch(dtw_ref.features(s), None, dtw_ref.features(twice_s), None, normalize=True)
    assert same_bits(dist.cpu().numpy(), want[0]) and same_bits(steps.cpu().numpy(), want[1])
    assert (dist.diagonal() > 0).all()
    same, _ = dhg_amd.dtw_distance(s, s.copy())
    assert (same.diagonal() == 0).all()


def test_blocks_give_the_bits_of_one_call():
    x, y = sixteenth_strokes(7, 40, 33), sixteenth_strokes(5, 56, 34)
    lx, ly = np.array([40, 1, 2, 33, 40, 17, 5]), np.array([56, 2, 1, 56, 30])
    one = dhg_amd.dtw_distance(x, y, lx, ly)
    want = dtw_ref.dtw_batch(dtw_ref.features(x), lx, dtw_ref.features(y), ly, normalize=True)
    assert one[0].shape == (7, 5) and one[1].dtype == torch.int32
    assert same_bits(one[0].cpu().numpy(), want[0]) and same_bits(one[1].cpu().numpy(), want[1])
    for chunk in (1, 3, 4):
        blocks = dhg_amd.dtw_distance(x, y, lx, ly, _chunk=chunk)
        assert all(same_bits(g.cpu().numpy(), w.cpu().numpy()) for g, w in zip(blocks, one)), chunk
    me = dhg_amd.dtw_distance(x, lengths_a=lx)
    assert same_bits(me[0].cpu().numpy(), dhg_amd.dtw_distance(x, x, lx, lx)[0].cpu().numpy()) and (me[0].diagonal() == 0).all()
    # nearest: against another set, against the set itself (refs given: every line finds itself) and against the other lines
    near, idx = dhg_amd.nearest_strokes(x, y, lx, ly)
    want_n, want_i = dtw_ref.nearest(want[0])
    assert idx.dtype == torch.int32 and same_bits(near.cpu().numpy(), want_n) and same_bits(idx.cpu().numpy(), want_i)
    near, idx = dhg_amd.nearest_strokes(x, x, lx, lx)
    assert (near == 0).all() and idx.tolist() == list(range(7))
    xx = dtw_ref.dtw_batch(dtw_ref.features(x), lx, dtw_ref.features(x), lx, normalize=True)[0]
    want_n, want_i = dtw_ref.nearest(xx, skip_diag=True)
    for chunk in (None, 2, 3):
        near, idx = dhg_amd.nearest_strokes(x, lengths_q=lx, _chunk=chunk)
        assert same_bits(near.cpu().numpy(), want_n) and same_bits(idx.cpu().numpy(), want_i), chunk
        near, idx = dhg_amd.nearest_strokes(x, y, lx, ly, _chunk=chunk)
        assert same_bits(idx.cpu().numpy(), dtw_ref.nearest(want[0])[1]), chunk
    dup = np.concatenate([y, y[3:4]])                                      # a duplicate in another block: the smaller index stays
    near, idx = dhg_amd.nearest_strokes(y[3:4], dup, _chunk=2)
    assert float(near[0]) == 0 and int(idx[0]) == 3


# ---------------------------------------------------------------- sample_metrics(dtw=True)
def test_sample_metrics_with_dtw():
    from test_gpu_quality import LT, L, T, pen_lines
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        extractor = dhg_amd.StyleExtractor()
    model = dhg_amd.DiffusionModel(2, precision="bf16", max_B=8, max_L=L, max_Lt=LT).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}, strict=True)
    inp = spec.synthetic_inputs(6, L, LT, seed=5)
    data = {"strokes": pen_lines(6), "text": torch.from_numpy(inp["text"]), "style": torch.from_numpy(inp["style"])}

    def metrics(**k):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return dhg_amd.sample_metrics(model, data, extractor, n=6, batch=4, k=3, T=T, **k)

    plain = metrics(seed=3)
    m, m2, m3 = metrics(seed=3, dtw=True), metrics(seed=3, dtw=True), metrics(seed=4, dtw=True)
    names = ("dtw_paired", "dtw_nearest", "dtw_self")
    assert set(m) - set(plain) == set(names) | {"dtw_nearest_idx"} and not set(plain) & set(names)
    assert all(np.isfinite(m[n]) and m[n] > 0 for n in names)
    assert all(m[n] == m2[n] for n in names) and torch.equal(m["dtw_nearest_idx"], m2["dtw_nearest_idx"])
    assert any(m[n] != m3[n] for n in names)
    # every other key has the bits of the call without dtw
    for n in ("fd", "precision", "recall", "density", "coverage", "kid", "k", "n"):
        assert m[n] == plain[n], n
    assert m["gen_set"].rows().tobytes() == plain["gen_set"].rows().tobytes() and m["real_set"].rows().tobytes() == plain["real_set"].rows().tobytes()
    # the three numbers are those of dtw_distance on the lines the loop drew
    gen = torch.cat([dhg_amd.sample(model, data["text"][lo:lo + 4].cuda(), data["style"][lo:lo + 4].cuda(), L=L, seed=3, first_sample=lo, T=T)
                     for lo in (0, 4)])
    cross = dhg_amd.dtw_distance(gen, data["strokes"])[0].cpu().numpy()
    own = dhg_amd.dtw_distance(gen)[0].cpu().numpy()
    np.fill_diagonal(own, np.inf)
    mean = lambda v: float(np.ascontiguousarray(v).astype(np.float64).mean())   # noqa: E731
    assert m["dtw_paired"] == mean(cross.diagonal()) and m["dtw_nearest"] == mean(cross.min(1)) and m["dtw_self"] == mean(own.min(1))
    assert m["dtw_nearest_idx"].cpu().numpy().tolist() == cross.argmin(1).tolist()
