"""CPU statement of the page ground truth's rules (include/dhw.h dhw_truth): numpy only.

The drawn set comes from vis.strokes_to_polylines (pinned to the reference's show_strokes by golden/vis.npz), the scale from
the two np.float32 divisions of tests/page_ref.py.  Boxes: every operation is one np.float32 operation in the rules' order, on
positions that are float64 prefix sums cast to float32 (exact on inputs whose offsets are multiples of 1/16:
page_ref.make_strokes), so boxes, spans and the scale can be compared bit for bit.  Labels: float64 brute force, which keeps
the minimum distance of every id to every pixel, so that the set of ids a device may answer (``accept``) can be formed."""
import numpy as np

from dhg_amd import vis

F32 = np.float32
EPS = 1e-3   # px: 75 times the error DESIGN.md §24 measured for the device's tile-relative distance


def drawn_segments(strokes, n):
    """(rows int [S], segs float64 [S, 2 endpoints, 2]) of the first n strokes: segment i runs from pos[i-1] to pos[i].  The
    polylines of strokes_to_polylines are pos[0:e0], pos[e0:e1], ...: consecutive rows."""
    rows, segs, i0 = [], [], 0
    for line in vis.strokes_to_polylines(np.asarray(strokes, np.float64)[:n]):
        for k in range(1, len(line)):
            rows.append(i0 + k)
            segs.append((line[k - 1], line[k]))
        i0 += len(line)
    return np.array(rows, np.int64), np.array(segs, np.float64).reshape(-1, 2, 2)


def truth_ref(strokes, groups, G, lens=None, slots=None, *, pages, height, width, lines_per_page, margin_left, margin_top, pitch,
              line_width=2.0, scale=None, labels=False):
    """-> dict(boxes f32 [N,G,4], spans i32 [N,G,3], scale f32 [1]) and, with ``labels``: labels i32 [P,H,W] (the rule in
    float64), ids i64 [K] (the ids that have a drawn segment, ascending) and dist f64 [K,P,H W] (the distance of every pixel
    centre to the nearest segment of each of them, inf on other pages)."""
    strokes, groups = np.asarray(strokes), np.asarray(groups)
    N, L = strokes.shape[:2]
    P, H, W, lpp = pages, height, width, lines_per_page
    availw = F32(W) - F32(2) * F32(margin_left)
    lines = []
    for n in range(N):
        slot = n if slots is None else int(slots[n])
        ln = L if lens is None else min(max(int(lens[n]), 0), L)
        rows, seg = drawn_segments(strokes[n], ln)
        if len(seg) == 0 or not 0 <= slot < P * lpp:
            lines.append(None)
            continue
        s32 = seg.astype(F32)
        assert (s32 == seg).all(), "the positions are not exact in float32"
        xmin, xmax, ymin, ymax = s32[..., 0].min(), s32[..., 0].max(), s32[..., 1].min(), s32[..., 1].max()
        ex, ey = xmax - xmin, ymax - ymin
        sn = F32(np.inf)
        if ey > 0:
            sn = F32(pitch) / ey
        if ex > 0:
            sn = min(sn, availw / ex)
        g = groups[n, rows].astype(np.int64)
        lines.append(dict(rows=rows, seg=s32, g=np.where((g >= 0) & (g < G), g, -1), xmin=xmin, ymax=ymax, ey=ey, sn=F32(sn), slot=slot))
    if scale is None:
        finite = [ln["sn"] for ln in lines if ln is not None and np.isfinite(ln["sn"])]
        s = F32(min(finite)) if finite else F32(1)
    else:
        s = F32(scale)

    boxes, spans = np.zeros((N, G, 4), F32), np.zeros((N, G, 3), np.int32)
    ml, mt, pt = F32(margin_left), F32(margin_top), F32(pitch)
    for n, ln in enumerate(lines):
        if ln is None:
            continue
        top = mt + F32(ln["slot"] % lpp) * pt
        ln["oy"] = oy = top + (pt - ln["ey"] * s) * F32(0.5)
        for g in np.unique(ln["g"][ln["g"] >= 0]):
            pick = ln["g"] == g
            e = ln["seg"][pick]
            gxmin, gxmax, gymin, gymax = e[..., 0].min(), e[..., 0].max(), e[..., 1].min(), e[..., 1].max()
            boxes[n, g] = (ml + (gxmin - ln["xmin"]) * s, oy + (ln["ymax"] - gymax) * s, ml + (gxmax - ln["xmin"]) * s, oy + (ln["ymax"] - gymin) * s)
            spans[n, g] = (ln["rows"][pick].min(), ln["rows"][pick].max() + 1, pick.sum())
    out = dict(boxes=boxes, spans=spans, scale=np.array([s], F32))
    if not labels:
        return out

    sd = float(s)
    ids = np.array(sorted({0 if g < 0 else 1 + n * G + int(g) for n, ln in enumerate(lines) if ln is not None for g in ln["g"]}), np.int64)
    dist = np.full((len(ids), P, H * W), np.inf)
    cy, cx = (v.reshape(-1, 1) for v in np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij"))   # [H W, 1]
    for n, ln in enumerate(lines):
        if ln is None:
            continue
        page, seg = ln["slot"] // lpp, ln["seg"].astype(np.float64)
        oy, x0, y1 = float(ln["oy"]), float(ln["xmin"]), float(ln["ymax"])
        A = np.stack([margin_left + (seg[:, 0, 0] - x0) * sd, oy + (y1 - seg[:, 0, 1]) * sd], -1)
        B = np.stack([margin_left + (seg[:, 1, 0] - x0) * sd, oy + (y1 - seg[:, 1, 1]) * sd], -1)
        for g in np.unique(ln["g"]):
            pick = np.flatnonzero(ln["g"] == g)
            d2 = np.full(H * W, np.inf)
            for k in range(0, len(pick), 64):
                a, b = A[pick[k:k + 64]], B[pick[k:k + 64]]
                abx, aby = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
                l2 = abx * abx + aby * aby
                rx, ry = cx - a[:, 0], cy - a[:, 1]
                t = np.clip((rx * abx + ry * aby) / np.where(l2 > 0, l2, 1.0), 0, 1) * (l2 > 0)   # a zero-length segment is a point
                rx -= t * abx
                ry -= t * aby
                np.minimum(d2, (rx * rx + ry * ry).min(-1), out=d2)
            k = int(np.searchsorted(ids, 0 if g < 0 else 1 + n * G + int(g)))
            np.minimum(dist[k, page], np.sqrt(d2), out=dist[k, page])
    R = line_width / 2 + 0.5
    if len(ids):
        best = dist.argmin(0)               # (the first minimum: ids ascend, so ties go to the smaller id)
        lab = np.where(dist.min(0) < R, ids[best], 0)
    else:
        lab = np.zeros((P, H * W), np.int64)
    out.update(labels=lab.reshape(P, H, W).astype(np.int32), ids=ids, dist=dist, radius=R)
    return out


def accept(ref, eps=EPS):
    """What a device may answer per pixel -> (ok bool [K,P,H W]: id ids[k] is within eps of the nearest; zero_ok bool [P,H W];
    must_zero bool [P,H W]; ink bool [P,H W]: the reference has ink there)."""
    dist, R = ref["dist"], ref["radius"]
    P, HW = ref["labels"].shape[0], ref["labels"].shape[1] * ref["labels"].shape[2]
    dmin = dist.min(0) if len(dist) else np.full((P, HW), np.inf)
    return dist <= dmin + eps, dmin >= R - eps, dmin > R + eps, dmin < R


def label_errors(device, ref, eps=EPS):
    """The pixels at which ``device`` [P,H,W] answers outside the accept set of the issue's rule (a bool array [P,H W])."""
    ok, zero_ok, must_zero, _ = accept(ref, eps)
    v = np.asarray(device).reshape(ok.shape[1:]).astype(np.int64)
    ids = ref["ids"]
    k = np.clip(np.searchsorted(ids, v), 0, max(len(ids) - 1, 0))
    named = np.zeros(v.shape, bool)
    if len(ids):
        named = (ids[k] == v) & np.take_along_axis(ok, k[None], 0)[0]
    good = np.where(must_zero, v == 0, named | ((v == 0) & zero_ok))
    return ~good


def accept_set_sizes(ref, eps=EPS):
    """(ink bool [P,H W], size int [P,H W]): how many different answers the rule accepts at every pixel."""
    ok, zero_ok, must_zero, ink = accept(ref, eps)
    has0 = ok[np.searchsorted(ref["ids"], 0)] if len(ref["ids"]) and ref["ids"][0] == 0 else np.zeros(zero_ok.shape, bool)
    size = np.where(must_zero, 1, (ok.sum(0) - has0) + (zero_ok | has0))
    return ink, size


# ---------------------------------------------------------------- the inputs of tests/test_gpu_truth.py
BASIC_GEO = dict(pages=2, height=160, width=256, lines_per_page=3, margin_left=6.0, margin_top=4.0, pitch=48.0)
BASIC_LENS = [40, 17, 33, 8, 40]


def basic_batch(seed=11):
    """N = 5, L = 40, a lift on each line's last row (BASIC_LENS), groups of 8 rows: G = 5."""
    import page_ref
    st = page_ref.make_strokes(np.random.default_rng(seed), 5, 40)
    for b, n in enumerate(BASIC_LENS):
        st[b, n - 1, 2] = 0.98
    return st, np.tile(np.arange(40) // 8, (5, 1)).astype(np.int32)


BOUNDARY_GEO = dict(pages=1, height=96, width=512, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=44.0)
BOUNDARY_CUTS = [15, 16, 17, 31, 32, 33, 200, 1000, 1023, 1025, 1050]   # the first row of each new group
BOUNDARY_G = len(BOUNDARY_CUTS) + 1


def boundary_batch():
    """N = 2, L = 1100, few lifts.  Line 0: a new group starts on both sides of the thread boundaries 15|16 and 31|32 and of the
    wave boundary 1023|1024 (rows 1023 and 1024 are one group of two rows; group 8 = rows 1000..1022 ends at it).  Line 1: the
    same cuts but one group across the wave boundary, rows 1000..1049."""
    import page_ref
    st = page_ref.make_strokes(np.random.default_rng(21), 2, 1100, lift_p=0.02)
    st[:, 1099, 2] = 0.98
    st[:, 990:1061, 2] = 0.3
    g = np.zeros((2, 1100), np.int32)
    for c in BOUNDARY_CUTS:
        g[:, c:] += 1
    g[1, 1000:1050] = g[1, 1000]
    return st, g


def overlap_batch():
    """Two lines in neighbouring slots at a scale that makes their ink overlap."""
    import page_ref
    st = page_ref.make_strokes(np.random.default_rng(31), 2, 48)
    st[:, 47, 2] = 0.98
    return st, np.tile(np.arange(48) // 8, (2, 1)).astype(np.int32)


OVERLAP_GEO = dict(pages=1, height=96, width=128, lines_per_page=4, margin_left=4.0, margin_top=30.0, pitch=8.0, scale=2.0)


CLAMPED_LENS = [30, 0, 30, 0, 30]   # what the device lengths [37, 0, 2^31 - 1, -5, 30] are clamped to at L = 30


def clamped_batch():
    """The basic batch cut to L = 30 (a lift on row 29): rows 30.. of a line are the next line's memory."""
    st, g = basic_batch()
    st, g = st[:, :30].copy(), g[:, :30].copy()
    st[:, 29, 2] = 0.98
    return st, g


NOPART_SLOTS = [0, 1, 99, 3, 4]


def nopart_batch():
    """The basic batch at full length.  Line 0: no lift; line 1: every row a lift; line 2: a slot off the pages (NOPART_SLOTS);
    lines 3 and 4 draw."""
    st, g = basic_batch()
    st[:, 39, 2] = 0.98
    st[0, :, 2] = 0.3
    st[1, :, 2] = 0.98
    return st, g
