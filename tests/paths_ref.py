"""The numpy float32 statement of dhw_paths' rules 3-9 (include/dhw.h), for the tests of the entry and of
dhg_amd.stroke_paths.  The drawn set comes from vis.strokes_to_polylines (pinned to the reference's show_strokes by
golden/vis.npz), the scale from the two np.float32 divisions of tests/page_ref.py; every further operation is one np.float32
operation in the rules' order.  Positions and boxes are float64 prefix sums cast to float32: exact on inputs whose offsets
are multiples of 1/16 (page_ref.make_strokes), in any summation order, so all five outputs can be compared bit for bit."""
import numpy as np

from dhg_amd import vis

F32 = np.float32


def line_polylines(strokes, n):
    """[(first stroke row, float32 [m,2] positions)] of the polylines of the first n strokes that hold at least 2 points.
    The polylines of strokes_to_polylines are pos[0:e0], pos[e0:e1], ...: consecutive rows, so each starts where the ones
    before it end."""
    out, i0 = [], 0
    for line in vis.strokes_to_polylines(np.asarray(strokes, np.float64)[:n]):
        if len(line) >= 2:
            out.append((i0, line.astype(F32)))
        i0 += len(line)
    return out


def smooth_pass(v):
    """One pass of rule 5 over one coordinate of one polyline."""
    out = v.copy()
    out[1:-1] = (v[:-2] + v[2:]) * F32(0.25) + v[1:-1] * F32(0.5)
    return out


def round_removals(x, y, kept, tol2, stats=None):
    """One round of rule 6 on one polyline: kept = the ascending indices into x, y of its kept points -> those that stay."""
    c = np.arange(1, len(kept) - 1, 2)                       # odd rank, not the end
    if len(c) == 0:
        return kept
    P, A, B = kept[c], kept[c - 1], kept[c + 1]
    abx, aby = x[B] - x[A], y[B] - y[A]
    apx, apy = x[P] - x[A], y[P] - y[A]
    len2 = abx * abx + aby * aby
    zero = len2 == 0
    if stats is not None:
        stats["len2_zero"] = stats.get("len2_zero", 0) + int(zero.sum())
        stats["evaluated"] = stats.get("evaluated", 0) + len(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.minimum(np.maximum((apx * abx + apy * aby) / len2, F32(0)), F32(1))
        ex, ey = apx - t * abx, apy - t * aby
        d2 = np.where(zero, apx * apx + apy * apy, ex * ex + ey * ey)
    assert d2.dtype == F32
    return np.delete(kept, c[d2 <= tol2])


def paths_ref(strokes, lens=None, slots=None, *, pages, height, width, lines_per_page, margin_left, margin_top, pitch, scale=None,
              smooth=1, tol=0.25, rounds=4, stats=None):
    """-> dict(points f32 [N,L,4], index i32 [N,L,2], counts i32 [N,2], scale f32 [1], boxes f32 [N,4]).  ``stats`` (a dict)
    receives how many candidates were evaluated and how many of them in the len2 == 0 branch."""
    strokes = np.asarray(strokes)
    N, L = strokes.shape[:2]
    P, W, lpp = pages, width, lines_per_page
    ml, mt, pitch = F32(margin_left), F32(margin_top), F32(pitch)
    availw = F32(W) - F32(2) * ml
    lines = []
    for n in range(N):
        slot = n if slots is None else int(slots[n])
        polys = line_polylines(strokes[n], L if lens is None else int(lens[n]))
        if not polys or not 0 <= slot < P * lpp:
            lines.append(None)
            continue
        pts = np.concatenate([p for _, p in polys])
        xmin, xmax, ymin, ymax = pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
        ex, ey = xmax - xmin, ymax - ymin
        sn = F32(np.inf)
        if ey > 0:
            sn = pitch / ey
        if ex > 0:
            sn = min(sn, availw / ex)
        lines.append(dict(polys=polys, xmin=xmin, ymax=ymax, ex=ex, ey=ey, sn=F32(sn), slot=slot))
    if scale is None:
        finite = [ln["sn"] for ln in lines if ln is not None and np.isfinite(ln["sn"])]
        s = F32(min(finite)) if finite else F32(1)
    else:
        s = F32(scale)

    tol2 = F32(tol) * F32(tol)
    points, index = np.zeros((N, L, 4), F32), np.full((N, L, 2), -1, np.int32)
    counts, boxes = np.zeros((N, 2), np.int32), np.zeros((N, 4), F32)
    for n, ln in enumerate(lines):
        if ln is None:
            continue
        top = mt + F32(ln["slot"] % lpp) * pitch
        oy = top + (pitch - ln["ey"] * s) * F32(0.5)
        boxes[n] = (ml, oy, ml + ln["ex"] * s, oy + ln["ey"] * s)
        k = 0
        for num, (i0, pos) in enumerate(ln["polys"]):
            x = ml + (pos[:, 0] - ln["xmin"]) * s
            y = oy + (ln["ymax"] - pos[:, 1]) * s
            for _ in range(smooth):
                x, y = smooth_pass(x), smooth_pass(y)
            kept = np.arange(len(x))
            for _ in range(rounds):
                kept = round_removals(x, y, kept, tol2, stats)
            xk, yk = x[kept], y[kept]
            tx = (np.concatenate([xk[1:], xk[-1:]]) - np.concatenate([xk[:1], xk[:-1]])) / F32(6)
            ty = (np.concatenate([yk[1:], yk[-1:]]) - np.concatenate([yk[:1], yk[:-1]])) / F32(6)
            assert x.dtype == y.dtype == tx.dtype == F32
            m = len(kept)
            points[n, k:k + m] = np.stack([xk, yk, tx, ty], -1)
            index[n, k:k + m, 0] = i0 + kept
            index[n, k:k + m, 1] = num
            k += m
        counts[n] = (k, len(ln["polys"]))
    return dict(points=points, index=index, counts=counts, scale=np.array([s], F32), boxes=boxes)


# ---------------------------------------------------------------- the inputs of the tests (tests/test_paths_cpu.py, tests/test_gpu_paths.py)
BASIC_GEO = dict(pages=2, height=160, width=256, lines_per_page=3, margin_left=6.0, margin_top=4.0, pitch=48.0)   # tests/test_gpu_page.py
BASIC_LENS = [40, 17, 33, 8, 40]


def basic_batch():
    """The basic batch of tests/test_gpu_page.py: seed 11, N = 5, L = 40, a lift on each line's last row, NaN past it."""
    import page_ref
    st = page_ref.make_strokes(np.random.default_rng(11), 5, 40)
    for b, n in enumerate(BASIC_LENS):
        st[b, n - 1, 2] = 0.98
        st[b, n:] = np.nan
    return st


BOUNDARY_GEO = dict(pages=1, height=96, width=512, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=44.0)
BOUNDARY_LIFTS = [15, 16, 17, 31, 32, 1023, 1024, 1025, 1099]


def boundary_batch():
    """N = 2, L = 1100.  Line 0: lifts on both sides of the thread boundaries 15|16 and 31|32 and of the wave boundary
    1023|1024; line 1: one polyline across rows 990..1060, so ranks and neighbours cross that wave boundary."""
    import page_ref
    st = page_ref.make_strokes(np.random.default_rng(21), 2, 1100, lift_p=0.04)
    st[0, BOUNDARY_LIFTS, 2] = 0.98
    st[1, 990:1061, 2] = 0.3
    st[1, 1099, 2] = 0.98
    return st


DEGENERATE_GEO = dict(pages=4, height=512, width=256, lines_per_page=20, margin_left=4.0, margin_top=6.0, pitch=24.0)


def degenerate_batch():
    """N = 70, L = 24 -> (strokes, lens, slots).  Line 0: every row a lift; 1: no lift; 2: lens = 1; 3, 4: slots off the pages;
    5: a hairpin (every other position the same point: len2 == 0 for every candidate of the first round); 6: rows with
    dx = dy = 0; the rest ordinary, of several lengths."""
    import page_ref
    N, L = 70, 24
    st = page_ref.make_strokes(np.random.default_rng(22), N, L, lift_p=0.06)
    lens = [L - (n % 5) for n in range(N)]
    lens[2] = 1
    for n in range(N):
        st[n, lens[n] - 1, 2] = 0.98
    st[0, :, 2] = 0.98
    st[1, :, 2] = 0.3
    st[5, :, :2], st[5, :, 2] = 0.0, 0.3
    st[5, 1::2, 0], st[5, 2::2, 0] = 1.5, -1.5
    st[5, 1::2, 1], st[5, 2::2, 1] = 0.25, -0.25
    st[5, lens[5] - 1, 2] = 0.98
    st[6, 4:9, :2] = 0.0
    st[6, 4:9, 2] = 0.3
    slots = list(range(N))
    slots[3], slots[4] = -1, 80
    return st, lens, slots
