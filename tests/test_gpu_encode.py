"""The stroke encoder on the GPU (include/dhw.h dhw_encode, dhg_amd.encode_strokes) against the reference's recorded outputs
(tests/golden/encode_lines.npz) and against the float64 statement of the rules (tests/encode_ref.py).

Tolerance, derived and not measured: both sides compute in fp64; the merged sets are equal because the gap between the last
merged and the first unmerged key is >= 1e-9 (asserted for every line used here), about 1e6 times the fp64 noise of the keys;
what is left is the fp64 noise of the values themselves (summation order of the std, about 1e-13 relative after four
normalisations), which can move an f32 rounding by one step at most.  So lengths, status and the pen column are exact and
dx, dy are at most 1 f32 ulp apart, compared as ordered int32 bit patterns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, vis

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "encode_lines.npz"))
CASES = sorted(int(k.split("_")[1]) for k in GOLDEN.files if k.startswith("points_"))
GOLDEN_L = int(GOLDEN["max_seq_len"])
PAD = np.array([0, 0, 1], np.float32)


def encode_raw(points, counts, L, rounds=3, max_abs=15.0):
    """dhw_encode on device tensors, on the current stream: points f32 [B,N,3], counts int32 [B] or None."""
    B, N = int(points.shape[0]), int(points.shape[1])
    l = _lib.lib()
    strokes = torch.empty((B, L, 3), device="cuda", dtype=torch.float32)
    lens = torch.empty((B,), device="cuda", dtype=torch.int32)
    status = torch.empty((B,), device="cuda", dtype=torch.int32)
    need = int(l.dhw_encode_workspace_bytes(B, N))
    ws = torch.empty(max(need, 16), device="cuda", dtype=torch.uint8)
    _lib.check(l.dhw_encode(points.data_ptr(), counts.data_ptr() if counts is not None else None, B, N, L, rounds, max_abs, strokes.data_ptr(),
                            lens.data_ptr(), status.data_ptr(), ws.data_ptr(), need, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return strokes, lens, status


def batch_of(lines, N=None, fill=np.nan):
    """Lines of different lengths in one [B,N,3] array; what lies past a line's count is NaN: it must never be read."""
    N = max(len(p) for p in lines) if N is None else N
    host = np.full((len(lines), N, 3), fill, np.float32)
    for b, p in enumerate(lines):
        host[b, :len(p)] = p
    return torch.from_numpy(host).cuda(), torch.tensor([len(p) for p in lines], dtype=torch.int32).cuda()


def run(lines, L, rounds=3, max_abs=15.0, N=None, counts=True):
    pts, cnt = batch_of(lines, N)
    out = encode_raw(pts, cnt if counts else None, L, rounds, max_abs)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def ulps(a, b):
    """|a - b| in f32 steps, through ordered integer images of the bit patterns (so -0.0 and 0.0 are 0 apart)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def check(got, want, label):
    (gs, gl, gst), (ws, wl, wst) = got, want
    assert gst.tolist() == list(wst), (label, gst.tolist(), list(wst))
    assert gl.tolist() == list(wl), (label, gl.tolist(), list(wl))
    for b in range(len(gs)):
        assert np.array_equal(gs[b, :, 2], ws[b][:, 2]), (label, b, "pen")
        d = ulps(gs[b, :, :2], ws[b][:, :2])
        print(f"{label}[{b}]: len {gl[b]} status {gst[b]} max ulp {d.max()} rows off by one {(d.max(axis=1) > 0).sum()}")
        assert d.max() <= 1, (label, b, int(d.max()))
        if gst[b]:
            assert (gs[b] == PAD).all(), (label, b)
        else:
            assert (gs[b, gl[b]:] == PAD).all(), (label, b)


# ---------------------------------------------------------------- against the reference's recorded outputs
def test_golden_lines_match_the_reference():
    lines = [GOLDEN[f"points_{c}"] for c in CASES]
    want_s = []
    for c in CASES:
        w = np.tile(PAD, (GOLDEN_L, 1))
        if not GOLDEN[f"dropped_{c}"]:
            w = GOLDEN[f"padded_{c}"]                       # the reference's own float32 rows and padding
            rows = GOLDEN[f"rows_{c}"]
            assert np.array_equal(w[:len(rows)], rows.astype(np.float32))
        want_s.append(w)
    want_l = [len(GOLDEN[f"rows_{c}"]) for c in CASES]
    want_st = [{9: 4, 10: 8}.get(c, 0) for c in CASES]     # the two lines the reference drops: too long, an offset above 15
    assert [bool(GOLDEN[f"dropped_{c}"]) for c in CASES] == [s != 0 for s in want_st]
    check(run(lines, GOLDEN_L), (want_s, want_l, want_st), "golden")


# ---------------------------------------------------------------- against the rules, on the smallest shapes that can go wrong
def pen_line(n, seed):
    """n integer tablet points in pen-down strokes of 3 to 30 points."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) * g.uniform(0.25, 0.45)
    x = np.cumsum(g.uniform(3, 13, n)) + 50 * np.sin(t) + g.normal(0, 1.5, n)
    y = 80 * np.cos(1.07 * t) + 25 * np.sin(0.31 * t) + g.normal(0, 1.5, n)
    end = np.zeros(n)
    i = 0
    while i < n:
        i += int(g.integers(3, 31))
        end[min(i, n) - 1] = 1
        if i < n:
            x[i:] += g.uniform(20, 100)
    return np.stack([np.rint(x), np.rint(y), end], axis=1).astype(np.float32)


def tied_line():
    """41 points: every step is (3, -1) but four, so 16 of the 20 pairs have a key of exactly 0 and k = 8: the cut falls
    inside the tie, and (v, j) says the lowest j merge."""
    steps = np.tile(np.array([[3.0, -1.0]]), (40, 1))
    steps[6], steps[17], steps[30], steps[39] = (1, 4), (-2, 5), (5, 3), (0, 6)
    p = np.zeros((41, 3), np.float32)
    p[1:, :2] = np.cumsum(steps, axis=0)
    p[[12, 25, 40], 2] = 1
    return p


SMALL = [
    np.array([[10, 20, 0], [13, 24, 1]], np.float32),          # n = 2: one row, k = 0, dx != dy
    np.array([[10, 20, 0], [13, 17, 1]], np.float32),          # n = 2: dx == dy, std 0 -> bit 2
    pen_line(3, 31), pen_line(6, 32), pen_line(7, 33),          # one pair, k = 0; 5 rows, k = 1, odd tail; even
    pen_line(65, 34), pen_line(66, 35), pen_line(257, 36), pen_line(258, 37), pen_line(1026, 38),   # 64, 65, 256, 257, 1025 rows
    pen_line(4096, 39),                                         # n = N
    tied_line(),
    np.concatenate([pen_line(20, 40)[:7], [[np.nan, 5, 0]], pen_line(20, 40)[8:]]).astype(np.float32),   # a NaN point -> bit 2
]


@pytest.mark.parametrize("rounds", [3, 1, 0])
def test_small_shapes_match_the_rules(rounds):
    for b, p in enumerate(SMALL):                              # the derivation of the tolerance needs a decided cut
        gaps = []
        encode_ref.encode_rows(p, rounds, gaps)
        assert b == 11 or all(g >= 1e-9 for g, _, _ in gaps), (b, gaps)
    rounds_tied = [b for b in range(len(SMALL)) if b != 11 or rounds == 1]   # the tie is exact in the first round only: later
    lines = [SMALL[b] for b in rounds_tied]                                   # rounds see rounded quotients
    want = encode_ref.encode_batch_ref(lines, 4096, rounds)
    assert want[2][1] == 2 and want[2][len(lines) - 1] == 2 and want[1][0] == 1 and sum(want[2]) == 4
    check(run(lines, 4096, rounds), want, f"small/rounds={rounds}")


def test_tied_keys_follow_the_v_j_order():
    p = tied_line()
    gaps = []
    rows, ok = encode_ref.encode_rows(p, 1, gaps)
    assert ok and gaps[0][1] == 16 and gaps[0][2] == 8 and gaps[0][0] == 0.0     # 16 exact zeros, k = 8, no gap at the cut
    assert len(rows) == 32 and np.allclose(rows[:3, 0] / rows[12, 0], 2) and not np.isclose(rows[3, 0] / rows[12, 0], 2)
    check(run([p], 32, 1), encode_ref.encode_batch_ref([p], 32, 1), "tied")


def test_whole_line_at_N_without_counts():
    p = SMALL[10]
    check(run([p, p[::-1].copy()], 2104, 3, counts=False), encode_ref.encode_batch_ref([p, p[::-1]], 2104, 3), "n=N=4096")


def test_status_bits():
    a, b = pen_line(100, 50), pen_line(30, 51)
    # M > L: 99 rows -> 52 after three rounds
    s, l, st = run([a, b], 48)
    assert st.tolist() == [4, 0] and l.tolist() == [52, 16] and (s[0] == PAD).all() and not (s[1, :16, :2] == 0).all()
    # counts[b] = 1, 0, N + 1: bit 1 and length 0; the neighbours are untouched by it
    pts, cnt = batch_of([a, b, a, b])
    cnt[:] = torch.tensor([1, 30, 101, 0], dtype=torch.int32)
    s, l, st = (t.cpu().numpy() for t in encode_raw(pts, cnt.cuda(), 56))
    assert st.tolist() == [1, 0, 1, 1] and l.tolist() == [0, 16, 0, 0] and (s[[0, 2, 3]] == PAD).all()
    check((s[1:2], l[1:2], st[1:2]), encode_ref.encode_batch_ref([b], 56), "beside bad counts")
    # max_abs: the largest offset of line a decides
    big = float(np.abs(encode_ref.encode_rows(a, 3)[0][:, :2]).max())
    assert run([a], 56, max_abs=big * 1.001)[2].tolist() == [0] and run([a], 56, max_abs=big * 0.999)[2].tolist() == [8]
    # an infinite coordinate and a NaN end flag are non-finite inputs too; a NaN past the count is never read
    c, d = a.copy(), a.copy()
    c[40, 1], d[0, 2] = np.inf, np.nan
    assert run([c, d, a], 56, N=128)[2].tolist() == [2, 2, 0]


# ---------------------------------------------------------------- batch independence and determinism
def test_a_row_of_a_batch_equals_the_line_alone_bit_for_bit():
    lines = [GOLDEN[f"points_{c}"] for c in CASES]
    first = run(lines, GOLDEN_L, N=1500)
    again = run(lines, GOLDEN_L, N=1500)
    for x, y in zip(first, again):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    for b, p in enumerate(lines):                                 # alone at N = counts[b]: lines of <= 1024 points run in the small
        alone = run([p], GOLDEN_L, N=len(p), counts=(b % 2 == 0))  # instance of the kernel, the batch in the large one
        for x, y in zip(first, alone):
            assert np.array_equal(x[b:b + 1].view(np.int32), y.view(np.int32)), b
    other_L = run(lines[:9], 360, N=700)                          # another L and N that admit the lines
    assert np.array_equal(other_L[0].view(np.int32), first[0][:9, :360].view(np.int32)) and np.array_equal(other_L[1], first[1][:9])


# ---------------------------------------------------------------- graph capture
def test_encode_then_render_in_one_graph_replays_identically():
    lines = [GOLDEN[f"points_{c}"] for c in (3, 6, 10, 7)]         # line 10 is dropped (bit 8): all padding, a white image
    pts, cnt = batch_of(lines, fill=0.0)
    H, W = 32, 256
    strokes, lens, status = encode_raw(pts, cnt, 208)               # warm-up: the renderer's workspace is allocated outside
    dhg_amd.render_strokes(strokes, lens.clamp(min=1), height=H, width=W)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        strokes, lens, status = encode_raw(pts, cnt, 208)
        img, wd = dhg_amd.render_strokes(strokes, lens.clamp(min=1), height=H, width=W)
    shots = []
    for _ in range(2):
        img.fill_(7.0)
        strokes.zero_()
        g.replay()
        torch.cuda.synchronize()
        shots.append((img.clone(), wd.clone(), strokes.clone(), status.clone()))
    for x, y in zip(*shots):
        assert torch.equal(x, y)
    img, wd, strokes, status = shots[0]
    assert status.tolist() == [0, 0, 8, 0]
    for b in (0, 1, 3):
        assert img[b].min().item() < 128 and wd[b].item() > 0, b
    assert (img[2] == 255).all() and wd[2].item() == 0
    eager = encode_raw(pts, cnt, 208)[0]
    assert torch.equal(strokes, eager)


# ---------------------------------------------------------------- the wrapper
def test_round_trip_through_polylines_keeps_the_pen_down_stretches():
    """strokes_to_polylines of an encoded line, encoded again without merging, gives the same stretches.  Positions are
    relative to the line's first point and strokes_to_polylines emits nothing after the last lift, so the origin and the
    final stretch are put back; y is negated because the encoder takes tablet coordinates (y downward)."""
    rows = GOLDEN["rows_7"]
    M = len(rows)
    polys = [q for q in vis.strokes_to_polylines(rows) if len(q)]
    pos = np.cumsum(rows[:, :2], axis=0)
    last = int(np.flatnonzero(rows[:, 2])[-1])
    full = [np.concatenate([[[0.0, 0.0]], polys[0]])] + polys[1:] + [pos[last:]]
    assert sum(len(q) for q in full) == M + 1
    strokes, lens, status = dhg_amd.encode_strokes([[q * [1, -1] for q in full]], rounds=0)
    assert strokes.shape == (1, (M + 7) // 8 * 8, 3) and lens.tolist() == [M] and status.tolist() == [0]
    assert dhg_amd.padded_lengths(lens) == [strokes.shape[1]]
    got = strokes[0, :M].cpu().numpy()
    assert np.array_equal(got[:, 2], rows[:, 2])
    again = vis.strokes_to_polylines(got)
    before = vis.strokes_to_polylines(rows)
    assert len(again) == len(before) and [len(q) for q in again] == [len(q) for q in before]
    s = np.std(rows[:, :2])                                          # (the rows are normalised once more: a factor close to 1)
    assert abs(s - 1) < 1e-9 and np.allclose(got[:, :2], rows[:, :2], rtol=0, atol=1e-5)


def test_encode_strokes_mixed_items_and_default_L():
    a, b = GOLDEN["points_3"], GOLDEN["points_6"]
    cut = np.flatnonzero(a[:, 2]) + 1
    as_polys = [q[:, :2] for q in np.split(a, cut[:-1])]
    strokes, lens, status = dhg_amd.encode_strokes([as_polys, b])
    assert strokes.shape == (2, 136, 3) and lens.tolist() == [21, 132] and status.tolist() == [0, 0]     # 132 rows -> L = 136
    want = encode_ref.encode_batch_ref([a, b], 136)
    check(tuple(t.cpu().numpy() for t in (strokes, lens, status)), want, "wrapper")
    unmarked = b.copy()
    unmarked[-1, 2] = 0                                               # the wrapper marks the line's last point itself
    assert torch.equal(dhg_amd.encode_strokes([unmarked])[0], strokes[1:2, :136])
