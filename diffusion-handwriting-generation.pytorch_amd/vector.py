"""Vector output: the pen-down polylines of sampled lines on the GPU (include/dhw.h dhw_paths) and SVG pages
made of them on the host."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _call
from .vis import check_page_geometry, check_page_lines, check_page_strokes

PATHS_MAX_SMOOTH = PATHS_MAX_ROUNDS = 8   # csrc/paths/paths_host.h


@dataclass
class StrokePaths:
    """What ``stroke_paths`` returns.  points f32 [N,L,4] = (x, y, tx, ty) in page pixels, index int32 [N,L,2] = (stroke row,
    polyline number), counts int32 [N,2] = (kept points, polylines), scale f32 [1], boxes f32 [N,4] = left, top, right, bottom
    of each line's ink (tensors, on the GPU as ``stroke_paths`` leaves them; ``page_svg`` also takes CPU tensors or arrays);
    slots = the slot of every line as given (a list, or the int32 device tensor of the call; None: slot n = n); and the
    geometry of the call."""
    points: object
    index: object
    counts: object
    scale: object
    boxes: object
    slots: object
    pages: int
    height: int
    width: int
    lines_per_page: int
    margin_left: float
    margin_top: float
    pitch: float


def _paths_options(smooth, tol, rounds):
    smooth, rounds = _call.check_int("smooth", smooth, 0), _call.check_int("rounds", rounds, 0)
    if smooth > PATHS_MAX_SMOOTH:
        raise ValueError(f"smooth = {smooth} must lie in [0, {PATHS_MAX_SMOOTH}]")
    if rounds > PATHS_MAX_ROUNDS:
        raise ValueError(f"rounds = {rounds} must lie in [0, {PATHS_MAX_ROUNDS}]")
    tol = _call.check_number("tol", tol)
    if tol < 0:
        raise ValueError(f"tol = {tol} must be >= 0")
    return smooth, tol, rounds


def stroke_paths(strokes, lengths=None, slots=None, *, pages=None, height: int = 1980, width: int = 1400, lines_per_page: int = 20,
                 margin_left: float = 70.0, margin_top: float = 70.0, pitch: float = 92.0, scale=None, smooth: int = 1, tol: float = 0.25,
                 rounds: int = 4) -> StrokePaths:
    """The pen-down polylines of a batch of lines as curves in page pixels, on the GPU (include/dhw.h dhw_paths):
    the vector twin of ``render_page``, with the same lines, slots, pages and ONE shared scale.

    strokes, lengths, slots, pages, the geometry and scale are ``render_page``'s (there is no line width: a path has none).
    Each pen-down stretch becomes a polyline; ``smooth`` passes of a (1/4, 1/2, 1/4) filter move its inner points, ``rounds``
    rounds of thinning drop every other point that lies within ``tol`` pixels of the chord between its neighbours, and every
    kept point gets a tangent, so that consecutive points P_k, P_k+1 are joined by the cubic Bezier with control points
    P_k + t_k and P_k+1 - t_k+1.  The tolerance holds per round, not for the result: see the header for what that means.
    The three defaults (smooth 1, tol 0.25, rounds 4) were chosen by eye on a few pages, not measured against anything.

    Returns a ``StrokePaths`` record, its tensors on the GPU.  Every argument rule raises ValueError before a device is
    touched.  One workspace is cached per device: calls on one device must be ordered on one stream."""
    import torch

    x, N, L = check_page_strokes(strokes)
    g = check_page_geometry(pages, height, width, lines_per_page, margin_left, margin_top, pitch, 2.0, scale)   # (no line width here)
    smooth, tol, rounds = _paths_options(smooth, tol, rounds)
    host_lens, host_slots, P = check_page_lines(lengths, slots, N, L, g)
    with _call.open("stroke_paths", like=x) as c:
        x = c.to(x.detach())
        lens, slot_t = _call.stage_ints(c, host_lens, lengths), _call.stage_ints(c, host_slots, slots)
        ws, need = c.workspace("paths", "dhw_paths_workspace_bytes", N, L)
        points, index, counts = c.empty((N, L, 4)), c.empty((N, L, 2), torch.int32), c.empty((N, 2), torch.int32)
        scale_out, boxes = c.empty((1,)), c.empty((N, 4))
        c.run("dhw_paths", x.data_ptr(), c.ptr(lens), c.ptr(slot_t), N, L, P, g["height"], g["width"], g["lines_per_page"], g["margin_left"],
              g["margin_top"], g["pitch"], g["scale"], smooth, tol, rounds, points.data_ptr(), index.data_ptr(), counts.data_ptr(),
              scale_out.data_ptr(), boxes.data_ptr(), c.ptr(ws), need)
    return StrokePaths(points, index, counts, scale_out, boxes, host_slots if host_slots is not None else slot_t, P, g["height"], g["width"],
                       g["lines_per_page"], g["margin_left"], g["margin_top"], g["pitch"])


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def page_svg(paths: StrokePaths, page: int, line_width: float = 2.0, curves: bool = True, precision: int = 2) -> str:
    """One page of a ``StrokePaths`` record as an SVG document (host code; the record's tensors may be on any device).

    An ``<svg>`` of width x height with the same viewBox, and per line that has points on this page, in line order, one
    ``<path id="line{n}" fill="none" stroke="black" stroke-width=... stroke-linecap="round" stroke-linejoin="round">``.  Each
    polyline is ``M x y`` and then, per further point, ``C (P_k + t_k) (P_k+1 - t_k+1) P_k+1`` (``curves``) or ``L x y``.
    Numbers are written with ``precision`` decimals."""
    page = _call.check_int("page", page, 0)
    if page >= paths.pages:
        raise ValueError(f"page = {page} must be below the record's {paths.pages} pages")
    precision = _call.check_int("precision", precision, 0)
    line_width = _call.check_number("line_width", line_width)
    if not line_width > 0:
        raise ValueError(f"line_width = {line_width} must be > 0")
    counts, points, index = _host(paths.counts), _host(paths.points), _host(paths.index)
    N = counts.shape[0]
    slots = [int(v) for v in _host(paths.slots).reshape(-1)] if paths.slots is not None else list(range(N))
    if len(slots) != N:
        raise ValueError(f"the record holds {N} lines and {len(slots)} slots")

    def num(v):
        return format(float(v), f".{precision}f")

    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{paths.width}" height="{paths.height}" viewBox="0 0 {paths.width} {paths.height}">']
    for n in range(N):
        kept = int(counts[n, 0])
        if kept == 0 or not 0 <= slots[n] < paths.pages * paths.lines_per_page or slots[n] // paths.lines_per_page != page:
            continue
        pts, poly = points[n, :kept], index[n, :kept, 1]
        d = []
        for k in range(kept):
            x, y, tx, ty = pts[k]
            if k == 0 or poly[k] != poly[k - 1]:
                d.append(f"M {num(x)} {num(y)}")
            elif curves:
                px, py, ptx, pty = pts[k - 1]
                d.append(f"C {num(px + ptx)} {num(py + pty)} {num(x - tx)} {num(y - ty)} {num(x)} {num(y)}")
            else:
                d.append(f"L {num(x)} {num(y)}")
        out.append(f'<path id="line{n}" fill="none" stroke="black" stroke-width="{num(line_width)}" stroke-linecap="round" '
                   f'stroke-linejoin="round" d="{" ".join(d)}"/>')
    out.append("</svg>")
    return "\n".join(out) + "\n"


def save_page_svg(paths: StrokePaths, page: int, name: str, **svg_kwargs) -> None:
    """Write one page of ``stroke_paths`` to ./<name>.svg (``page_svg``)."""
    with open(f"./{name}.svg", "w", encoding="utf-8") as f:
        f.write(page_svg(paths, page, **svg_kwargs))
