"""Output side of the sampler (reference utils/vis.py:5-36): offsets -> pen positions -> polylines."""
from __future__ import annotations

import ctypes as C

import numpy as np

RENDER_CHUNK = 256   # segments per LDS chunk of the raster kernel (csrc/render/render.h RENDER_CHUNK): a tile that keeps more
                     # than this many segments goes through several chunks
RENDER_TILE_W = 32   # columns per raster tile (csrc/render/render.h RENDER_TILE_W)
_render_workspaces = {}   # device index -> [uint8 workspace tensors of render_strokes, the newest (largest) last]


def _render_workspace(dev, need: int):
    """One workspace per device, grown by doubling.  Outgrown buffers stay referenced (a captured graph may still point at
    one): at most one per doubling, together smaller than the newest."""
    import torch

    bufs = _render_workspaces.setdefault(dev.index, [])
    if not bufs or bufs[-1].numel() < need:
        size = 1 << 16
        while size < need:
            size *= 2
        bufs.append(torch.empty(size, dtype=torch.uint8, device=dev))
    return bufs[-1]


def render_workspace_segments(device, B: int, L: int):
    """What the last render_strokes call of shape (B, L) on `device` left in the workspace, as host arrays: (header int32
    [B,2] = (drawn segments, width) per row, segments f32 [B,L,4] = (x0, y0, x1, y1) in pixel coordinates, row b valid up to
    header[b,0]).  For tools that look at the cull (tools/bench_render.py)."""
    import torch

    from . import _lib
    idx = torch.device(device).index
    ws = _render_workspaces[torch.cuda.current_device() if idx is None else idx][-1].cpu().numpy()
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
    if not torch.cuda.is_available():
        raise RuntimeError("render_strokes needs an MI355X (HIP device): there is no CPU path in this package")
    from . import _lib

    B, L = int(x.shape[0]), int(x.shape[1])
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    l = _lib.lib()
    with torch.cuda.device(dev):
        x = x.detach().to(dev, torch.float32).contiguous()
        lens = None
        if lengths is not None:
            if isinstance(lengths, torch.Tensor) and lengths.is_cuda:   # stays on the device: no host read, no host check
                lens = lengths.to(dev, torch.int32).contiguous()
            else:
                host = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
                if len(host) != B or any(v < 1 or v > L for v in host):
                    raise ValueError(f"lengths must be {B} integers in [1, {L}], got {host}")
                lens = torch.tensor(host, dtype=torch.int32).to(dev)
            if lens.numel() != B:
                raise ValueError(f"lengths must hold {B} entries")
        need = int(l.dhw_render_workspace_bytes(B, L))
        ws = _render_workspace(dev, need) if need else None
        images = torch.empty((B, 1, int(height), int(width)), device=dev, dtype=torch.float32)
        widths = torch.empty((B,), device=dev, dtype=torch.int32)
        st = torch.cuda.current_stream(dev)
        _lib.check(l.dhw_render(x.data_ptr(), lens.data_ptr() if lens is not None else None, B, L, int(height), int(width),
                                float(line_width), images.data_ptr(), widths.data_ptr(), ws.data_ptr() if ws is not None else None,
                                need, C.c_void_p(st.cuda_stream)))
    return images, widths


def save_line_png(image, width, name: str) -> None:
    """Write one rendered line to ./<name>.png: `image` ([H,W] or [1,H,W], tensor or array, grey levels 0..255) cropped to
    its first `width` columns and rounded to uint8."""
    from PIL import Image

    a = image.detach().cpu().numpy() if hasattr(image, "detach") else np.asarray(image)
    a = a.reshape(a.shape[-2], a.shape[-1])[:, :max(1, int(width))]
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
