"""Output side of the sampler (reference utils/vis.py:5-36): offsets -> pen positions -> polylines."""
from __future__ import annotations

import numpy as np

from . import _call, _lib

RENDER_CHUNK = 256   # segments per LDS chunk of the raster kernel (csrc/render/render.h RENDER_CHUNK): a tile that keeps more
                     # than this many segments goes through several chunks
RENDER_TILE_W = 32   # columns per raster tile (csrc/render/render.h RENDER_TILE_W)


def render_workspace_segments(device, B: int, L: int):
    """What the last render_strokes call of shape (B, L) on `device` left in the workspace, as host arrays: (header int32
    [B,2] = (drawn segments, width) per row, segments f32 [B,L,4] = (x0, y0, x1, y1) in pixel coordinates, row b valid up to
    header[b,0]).  For tools that look at the cull (tools/bench_render.py)."""
    import torch

    idx = torch.device(device).index
    ws = _call.newest_workspace("render", torch.cuda.current_device() if idx is None else idx).cpu().numpy()
    need = int(_lib.lib().dhw_render_workspace_bytes(B, L))
    hdr_bytes = need - B * L * 16
    return ws[:B * 8].view(np.int32).reshape(B, 2).copy(), ws[hdr_bytes:need].view(np.float32).reshape(B, L, 4).copy()


def strokes_to_polylines(strokes: np.ndarray) -> list[np.ndarray]:
    """[L,3] = (dx, dy, pen) -> list of [n,2] position arrays, one per pen-down stretch.  Positions are the running sum of
    the offsets; a rounded pen value of 1 at row i ends the stretch BEFORE row i (the move to i is a jump), vis.py:13-31."""
    strokes = np.asarray(strokes)
    pos = np.cumsum(strokes[:, :2], axis=0)
    ends = np.flatnonzero(np.round(strokes[:, 2]) != 0)
    lines, prev = [], 0
    for ind in ends:
        lines.append(pos[prev:ind])
        prev = int(ind)
    return lines


def show_strokes(strokes: np.ndarray, name: str = "", show_output: bool = True, scale: int = 1) -> None:
    """Plot the strokes (and save ./<name>.png); needs matplotlib."""
    import matplotlib

    if not show_output:
        matplotlib.use("Agg")
    from matplotlib import pyplot as plt

    pos = np.cumsum(np.asarray(strokes)[:, :2], axis=0).T
    w, h = np.max(pos, axis=-1) - np.min(pos, axis=-1)
    plt.figure(figsize=(scale * w / h, scale))
    plt.axis("off")
    for line in strokes_to_polylines(strokes):
        plt.plot(line[:, 0], line[:, 1], color="black")
    if name:
        plt.savefig(f"./{name}.png", bbox_inches="tight")
    if show_output:
        plt.show()
    else:
        plt.close()


def render_strokes(strokes, lengths=None, height: int = 96, width: int = 1400, line_width: float = 2.0):
    """Rasterise a batch of strokes on the GPU (include/dhw.h dhw_render).

    strokes: [B,L,3] = (dx, dy, pen), a tensor on any device or an array.  lengths (optional, list or tensor of B ints in
    [1, L]): row b uses its first lengths[b] strokes, the rest is never read.  Returns (images, widths), both on the GPU:
    images f32 [B,1,height,width], grey levels 0..255 with the ink left-aligned and white to the right (what
    ``StyleExtractor`` takes), widths int32 [B] = the columns the ink and its margin cover (0 for a row without ink).

    One workspace is cached per device (grown as needed): calls on one device must be ordered on one stream."""
    import torch

    x = strokes if isinstance(strokes, torch.Tensor) else torch.as_tensor(np.asarray(strokes))
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"strokes must be [B, L, 3], got {tuple(x.shape)}")
    B, L = int(x.shape[0]), int(x.shape[1])
    with _call.open("render_strokes", like=x) as c:
        x = c.to(x.detach())
        host = None
        if lengths is not None and not _call.on_device(lengths):   # (a device tensor stays there: no host read, no host check)
            host = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]   # looser than host_ints: §48
            if len(host) != B or any(v < 1 or v > L for v in host):
                raise ValueError(f"lengths must be {B} integers in [1, {L}], got {host}")
        lens = _call.stage_ints(c, host, lengths)
        if lens is not None and lens.numel() != B:
            raise ValueError(f"lengths must hold {B} entries")
        ws, need = c.workspace("render", "dhw_render_workspace_bytes", B, L)
        images, widths = c.empty((B, 1, int(height), int(width))), c.empty((B,), torch.int32)
        c.run("dhw_render", x.data_ptr(), c.ptr(lens), B, L, int(height), int(width), float(line_width), images.data_ptr(),
              widths.data_ptr(), c.ptr(ws), need)
    return images, widths


def save_line_png(image, width, name: str) -> None:
    """Write one rendered line to ./<name>.png: `image` ([H,W] or [1,H,W], tensor or array, grey levels 0..255) cropped to
    its first `width` columns and rounded to uint8."""
    from PIL import Image

    a = image.detach().cpu().numpy() if hasattr(image, "detach") else np.asarray(image)
    a = a.reshape(a.shape[-2], a.shape[-1])[:, :max(1, int(width))]
    Image.fromarray(np.clip(np.rint(a), 0, 255).astype(np.uint8)).save(f"./{name}.png")


PAGE_MAX_N = PAGE_MAX_L = 4096   # csrc/page/page_host.h


def check_page_geometry(pages, height, width, lines_per_page, margin_left, margin_top, pitch, line_width, scale) -> dict:
    """The geometry rules of dhw_page (include/dhw.h) with ValueError, on the host: what render_page and write_page check
    before they touch a device.  ``pages`` may be None (decided later).  Returns the checked values."""
    i, f = _call.check_int, _call.check_number
    g = dict(pages=None if pages is None else i("pages", pages, 1), height=i("height", height, 8), width=i("width", width, 8),
             lines_per_page=i("lines_per_page", lines_per_page, 1), margin_left=f("margin_left", margin_left),
             margin_top=f("margin_top", margin_top), pitch=f("pitch", pitch), line_width=f("line_width", line_width),
             scale=0.0 if scale is None else f("scale", scale))
    if g["width"] % 4:
        raise ValueError(f"width = {g['width']} must be a multiple of 4")
    if not g["pitch"] > 0:
        raise ValueError(f"pitch = {g['pitch']} must be > 0")
    for k in ("margin_left", "margin_top"):
        if g[k] < 0:
            raise ValueError(f"{k} = {g[k]} must be >= 0")
    if not g["width"] - 2 * g["margin_left"] > 0:
        raise ValueError(f"margin_left = {g['margin_left']} leaves no room: width - 2 margin_left must be > 0 (width {g['width']})")
    if not 0.5 <= g["line_width"] <= 16:
        raise ValueError(f"line_width = {g['line_width']} must lie in [0.5, 16]")
    if scale is not None and not g["scale"] > 0:
        raise ValueError(f"scale = {g['scale']} must be > 0 (None: automatic)")
    _check_page_count(g, g["pages"])
    return g


def _check_page_count(g: dict, pages) -> None:
    if pages is None:
        return
    if pages * g["height"] * g["width"] >= 2 ** 31:
        raise ValueError(f"pages x height x width must stay below 2^31 (pages {pages}, height {g['height']}, width {g['width']})")
    if pages * -(-g["width"] // 32) >= 2 ** 24 or -(-g["height"] // 96) > 65535:
        raise ValueError(f"pages x width (or height) is beyond the launch grid (pages {pages}, height {g['height']}, width {g['width']})")


def check_page_strokes(strokes):
    """The strokes rule ``render_page`` and ``stroke_paths`` open with, on the host: (strokes as a tensor [N,L,3] where it was, N, L)."""
    import torch

    x = strokes if isinstance(strokes, torch.Tensor) else torch.as_tensor(np.asarray(strokes))
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"strokes must be [N, L, 3], got {tuple(x.shape)}")
    if not x.is_floating_point():
        raise ValueError(f"strokes must be floating-point, got {x.dtype}")
    N, L = int(x.shape[0]), int(x.shape[1])
    if not 1 <= N <= PAGE_MAX_N or not 1 <= L <= PAGE_MAX_L:
        raise ValueError(f"strokes must be [N, L, 3] with N in [1, {PAGE_MAX_N}] and L in [1, {PAGE_MAX_L}], got {tuple(x.shape)}")
    return x, N, L


def check_page_lines(lengths, slots, N: int, L: int, g: dict):
    """The rules of ``render_page`` and ``stroke_paths`` that follow the geometry ``g`` (check_page_geometry), on the host: (lengths,
    slots as checked host lists (None: not given, or a device tensor, which is only counted), the pages P)."""
    host_lens = host_slots = None
    if lengths is not None:
        if _call.on_device(lengths):
            if lengths.numel() != N:
                raise ValueError(f"lengths must hold {N} entries, got {lengths.numel()}")
        else:
            host_lens = _call.host_ints("lengths", lengths, N)
            if any(v < 1 or v > L for v in host_lens):
                raise ValueError(f"lengths must be {N} integers in [1, {L}], got {host_lens}")
    if slots is not None:
        if _call.on_device(slots):
            if slots.numel() != N:
                raise ValueError(f"slots must hold {N} entries, got {slots.numel()}")
        else:
            host_slots = _call.host_ints("slots", slots, N)
    P = g["pages"]
    if P is None:
        lpp = g["lines_per_page"]
        P = max(0, max(host_slots)) // lpp + 1 if host_slots is not None else -(-N // lpp)
        _check_page_count(g, P)
    return host_lens, host_slots, P


def render_page(strokes, lengths=None, slots=None, *, pages=None, height: int = 1980, width: int = 1400, lines_per_page: int = 20,
                margin_left: float = 70.0, margin_top: float = 70.0, pitch: float = 92.0, line_width: float = 2.0, scale=None):
    """Compose a batch of lines into page images on the GPU, all at ONE scale (include/dhw.h dhw_page).

    strokes: [N,L,3] = (dx, dy, pen), a tensor on any device or an array.  lengths (optional, N ints in [1, L]): line n uses
    its first lengths[n] strokes.  slots (optional, N ints; default slot n = n): line n is drawn in slot ``slots[n] %
    lines_per_page`` of page ``slots[n] // lines_per_page``, ``pitch`` pixels below the slot before; a line whose slot is off
    the pages is not drawn.  Both may be host data or device tensors (a device tensor stays on the device and is not
    checked).  ``pages=None``: enough pages for the largest slot when the slots are host data, else ceil(N / lines_per_page).
    ``scale=None``: the largest scale at which every line fits its slot (height ``pitch``, width ``width - 2 margin_left``);
    a number: that many pixels per stroke unit, and lines may then overlap their neighbours (composed by min).

    Returns (pages f32 [P,1,height,width] grey levels 0..255, scale f32 [1], boxes f32 [N,4] = left, top, right, bottom of each
    line's ink in page pixels, zeros for a line that draws nothing), all on the GPU.  Every argument rule raises ValueError
    before a device is touched.  One workspace is cached per device: calls on one device must be ordered on one stream."""
    x, N, L = check_page_strokes(strokes)
    g = check_page_geometry(pages, height, width, lines_per_page, margin_left, margin_top, pitch, line_width, scale)
    host_lens, host_slots, P = check_page_lines(lengths, slots, N, L, g)
    with _call.open("render_page", like=x) as c:
        x = c.to(x.detach())
        lens, slot_t = _call.stage_ints(c, host_lens, lengths), _call.stage_ints(c, host_slots, slots)
        ws, need = c.workspace("page", "dhw_page_workspace_bytes", N, L)
        out, scale_out, boxes = c.empty((P, 1, g["height"], g["width"])), c.empty((1,)), c.empty((N, 4))
        c.run("dhw_page", x.data_ptr(), c.ptr(lens), c.ptr(slot_t), N, L, P, g["height"], g["width"], g["lines_per_page"], g["margin_left"],
              g["margin_top"], g["pitch"], g["line_width"], g["scale"], out.data_ptr(), scale_out.data_ptr(), boxes.data_ptr(), c.ptr(ws), need)
    return out, scale_out, boxes


def save_page_png(page, name: str) -> None:
    """Write one page of render_page to ./<name>.png: `page` ([H,W] or [1,H,W], tensor or array, grey levels 0..255) rounded
    to uint8."""
    from PIL import Image

    a = page.detach().cpu().numpy() if hasattr(page, "detach") else np.asarray(page)
    a = a.reshape(a.shape[-2], a.shape[-1])
    Image.fromarray(np.clip(np.rint(a), 0, 255).astype(np.uint8)).save(f"./{name}.png")


def render_lines_png(strokes_list, names, height: int = 96, width: int = 1400, line_width: float = 2.0) -> None:
    """Render a list of [L_i,3] stroke arrays in ONE render_strokes call and write ./<names[i]>.png for each."""
    lens = [int(len(s)) for s in strokes_list]
    batch = np.zeros((len(lens), max(lens), 3), np.float32)
    for b, s in enumerate(strokes_list):
        batch[b, :lens[b]] = np.asarray(s, np.float32)
    images, widths = render_strokes(batch, lens, height, width, line_width)
    images, widths = images.cpu(), widths.cpu().tolist()
    for b, name in enumerate(names):
        save_line_png(images[b], widths[b], name)
