"""CPU statement of the page compositor's rules (include/dhw.h dhw_page): float64, brute force, numpy only.

The drawn set of every line comes from vis.strokes_to_polylines (pinned to the reference's show_strokes by golden/vis.npz).
Positions, boxes and pixels are float64; the per-line scale limits s_n and the shared scale s are formed with np.float32
divisions exactly as the header states them, so that the scale can be compared bit for bit on inputs whose prefix sums are
exact in fp32 (offsets that are multiples of 1/16: ``make_strokes``, which tests/test_gpu_render.py uses too)."""
import numpy as np

from dhg_amd import vis

PENS = np.array([0.02, 0.3, 0.5, 0.7, 0.98])   # (none rounds differently in fp32)


def make_strokes(rng, B, L, lift_p=0.08):
    """Offsets on the 1/16 grid (dx = round(N(0.6,1) 16)/16, dy = round(N(0,1) 16)/16), pens from PENS: every fp32 prefix sum
    and box is exact in any summation order."""
    dx = np.round(rng.normal(0.6, 1.0, (B, L)) * 16) / 16
    dy = np.round(rng.normal(0.0, 1.0, (B, L)) * 16) / 16
    pen = np.where(rng.random((B, L)) < lift_p, rng.choice(PENS[3:], (B, L)), rng.choice(PENS[:3], (B, L)))
    return np.stack([dx, dy, pen], -1).astype(np.float32)


def line_segments(strokes, n):
    """[S, 2 endpoints, 2 coordinates] float64: the consecutive point pairs inside the polylines of the first n strokes."""
    segs = []
    for line in vis.strokes_to_polylines(np.asarray(strokes, np.float64)[:n]):
        for k in range(1, len(line)):
            segs.append((line[k - 1], line[k]))
    return np.array(segs, np.float64).reshape(-1, 2, 2)


def page_ref(strokes, lens=None, slots=None, *, pages, height, width, lines_per_page, margin_left, margin_top, pitch, line_width=2.0,
             scale=None):
    """-> (pages float64 [P,H,W], s np.float32, boxes float64 [N,4] = left, top, right, bottom; segments drawn per line)."""
    strokes = np.asarray(strokes)
    N, L = strokes.shape[:2]
    P, H, W, lpp = pages, height, width, lines_per_page
    f32 = np.float32
    availw = f32(W) - f32(2) * f32(margin_left)
    lines = []
    for n in range(N):
        slot = n if slots is None else int(slots[n])
        seg = line_segments(strokes[n], L if lens is None else int(lens[n]))
        if len(seg) == 0 or not 0 <= slot < P * lpp:
            lines.append(None)
            continue
        xmin, xmax = seg[..., 0].min(), seg[..., 0].max()
        ymin, ymax = seg[..., 1].min(), seg[..., 1].max()
        ex, ey = xmax - xmin, ymax - ymin
        sn = f32(np.inf)
        if ey > 0:
            sn = f32(pitch) / f32(ey)
        if ex > 0:
            sn = min(sn, availw / f32(ex))
        lines.append(dict(seg=seg, xmin=xmin, ymax=ymax, ex=ex, ey=ey, sn=f32(sn), slot=slot))
    if scale is None:
        finite = [ln["sn"] for ln in lines if ln is not None and np.isfinite(ln["sn"])]
        s32 = f32(min(finite)) if finite else f32(1)
    else:
        s32 = f32(scale)
    s = float(s32)

    out = np.full((P, H * W), np.inf)               # squared distance to the nearest ink of the page
    boxes = np.zeros((N, 4))
    counts = [0 if ln is None else len(ln["seg"]) for ln in lines]
    cy, cx = (v.reshape(-1, 1) for v in np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij"))   # [H W, 1]
    for n, ln in enumerate(lines):
        if ln is None:
            continue
        page, top = ln["slot"] // lpp, margin_top + (ln["slot"] % lpp) * pitch
        oy = top + (pitch - ln["ey"] * s) / 2
        boxes[n] = (margin_left, oy, margin_left + ln["ex"] * s, oy + ln["ey"] * s)
        A = np.stack([margin_left + (ln["seg"][:, 0, 0] - ln["xmin"]) * s, oy + (ln["ymax"] - ln["seg"][:, 0, 1]) * s], -1)
        Bp = np.stack([margin_left + (ln["seg"][:, 1, 0] - ln["xmin"]) * s, oy + (ln["ymax"] - ln["seg"][:, 1, 1]) * s], -1)
        d2 = out[page]
        for k in range(0, len(A), 64):
            ax, ay = A[k:k + 64, 0], A[k:k + 64, 1]
            abx, aby = Bp[k:k + 64, 0] - ax, Bp[k:k + 64, 1] - ay
            l2 = abx * abx + aby * aby
            rx, ry = cx - ax, cy - ay                   # [H W, 64]
            t = np.clip((rx * abx + ry * aby) / np.where(l2 > 0, l2, 1.0), 0, 1) * (l2 > 0)   # a zero-length segment is a point
            rx -= t * abx
            ry -= t * aby
            np.minimum(d2, (rx * rx + ry * ry).min(-1), out=d2)
    img = 255.0 * (1 - np.clip(line_width / 2 + 0.5 - np.sqrt(out), 0, 1))
    return img.reshape(P, H, W), s32, boxes, counts
