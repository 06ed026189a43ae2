"""Vector output: the pen-down polylines of sampled lines on the GPU (include/dhw.h dhw_paths) and SVG pages
made of them on the host."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .vis import PAGE_MAX_L, PAGE_MAX_N, _check_page_count, _host_ints, _page_float, _page_int, _workspace, check_page_geometry

PATHS_MAX_SMOOTH = PATHS_MAX_ROUNDS = 8   # csrc/paths/paths_host.h
_paths_workspaces = {}                    # of stroke_paths: device index -> workspace tensors (vis._workspace)


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
    smooth, rounds = _page_int("smooth", smooth, 0), _page_int("rounds", rounds, 0)
    if smooth > PATHS_MAX_SMOOTH:
        raise ValueError(f"smooth = {smooth} must lie in [0, {PATHS_MAX_SMOOTH}]")
    if rounds > PATHS_MAX_ROUNDS:
        raise ValueError(f"rounds = {rounds} must lie in [0, {PATHS_MAX_ROUNDS}]")
    tol = _page_float("tol", tol)
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

    x = strokes if isinstance(strokes, torch.Tensor) else torch.as_tensor(np.asarray(strokes))
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"strokes must be [N, L, 3], got {tuple(x.shape)}")
    if not x.is_floating_point():
        raise ValueError(f"strokes must be floating-point, got {x.dtype}")
    N, L = int(x.shape[0]), int(x.shape[1])
    if not 1 <= N <= PAGE_MAX_N or not 1 <= L <= PAGE_MAX_L:
        raise ValueError(f"strokes must be [N, L, 3] with N in [1, {PAGE_MAX_N}] and L in [1, {PAGE_MAX_L}], got {tuple(x.shape)}")
    g = check_page_geometry(pages, height, width, lines_per_page, margin_left, margin_top, pitch, 2.0, scale)   # (no line width here)
    smooth, tol, rounds = _paths_options(smooth, tol, rounds)

    def on_device(v):
        return isinstance(v, torch.Tensor) and v.is_cuda

    host_lens = host_slots = None
    if lengths is not None:
        if on_device(lengths):
            if lengths.numel() != N:
                raise ValueError(f"lengths must hold {N} entries, got {lengths.numel()}")
        else:
            host_lens = _host_ints("lengths", lengths, N)
            if any(v < 1 or v > L for v in host_lens):
                raise ValueError(f"lengths must be {N} integers in [1, {L}], got {host_lens}")
    if slots is not None:
        if on_device(slots):
            if slots.numel() != N:
                raise ValueError(f"slots must hold {N} entries, got {slots.numel()}")
        else:
            host_slots = _host_ints("slots", slots, N)
    P = g["pages"]
    if P is None:
        lpp = g["lines_per_page"]
        P = max(0, max(host_slots)) // lpp + 1 if host_slots is not None else -(-N // lpp)
        _check_page_count(g, P)
    if not torch.cuda.is_available():
        raise RuntimeError("stroke_paths needs an MI355X (HIP device): there is no CPU path in this package")
    from . import _lib

    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    l = _lib.lib()
    with torch.cuda.device(dev):
        x = x.detach().to(dev, torch.float32).contiguous()

        def ints(host, given):
            if given is None:
                return None
            return torch.tensor(host, dtype=torch.int32).to(dev) if host is not None else given.to(dev, torch.int32).contiguous()

        lens, slot_t = ints(host_lens, lengths), ints(host_slots, slots)
        need = int(l.dhw_paths_workspace_bytes(N, L))
        ws = _workspace(_paths_workspaces, dev, need)
        points = torch.empty((N, L, 4), device=dev, dtype=torch.float32)
        index = torch.empty((N, L, 2), device=dev, dtype=torch.int32)
        counts = torch.empty((N, 2), device=dev, dtype=torch.int32)
        scale_out = torch.empty((1,), device=dev, dtype=torch.float32)
        boxes = torch.empty((N, 4), device=dev, dtype=torch.float32)
        st = torch.cuda.current_stream(dev)
        _lib.check(l.dhw_paths(x.data_ptr(), lens.data_ptr() if lens is not None else None, slot_t.data_ptr() if slot_t is not None else None,
                               N, L, P, g["height"], g["width"], g["lines_per_page"], g["margin_left"], g["margin_top"], g["pitch"], g["scale"],
                               smooth, tol, rounds, points.data_ptr(), index.data_ptr(), counts.data_ptr(), scale_out.data_ptr(),
                               boxes.data_ptr(), ws.data_ptr(), need, C.c_void_p(st.cuda_stream)))
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
    page = _page_int("page", page, 0)
    if page >= paths.pages:
        raise ValueError(f"page = {page} must be below the record's {paths.pages} pages")
    precision = _page_int("precision", precision, 0)
    line_width = _page_float("line_width", line_width)
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
