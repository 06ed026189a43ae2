"""Input side of the StyleExtractor: raw writer images of different sizes -> one padded [B,1,H,W] batch on the GPU
(include/dhw.h dhw_prep), and the style features of many images in batched StyleExtractor calls."""
from __future__ import annotations

import numpy as np

from . import _call

# csrc/prep/prep_host.h
PREP_MAX_B, PREP_MAX_HIN, PREP_MAX_WIN, PREP_MIN_H, PREP_MAX_H, PREP_MIN_W, PREP_MAX_W = 65535, 4096, 16384, 8, 512, 8, 4096


def _as_image(i: int, item) -> np.ndarray:
    """One item of `images` -> u8 [h,w] on the host; a path is read as read_img reads it (PIL, convert("L"))."""
    if isinstance(item, (str, bytes)) or hasattr(item, "__fspath__"):
        from PIL import Image
        a = np.asarray(Image.open(item.decode() if isinstance(item, bytes) else str(item)).convert("L"))
    else:
        a = item.detach().cpu().numpy() if hasattr(item, "detach") else np.asarray(item)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"images[{i}] must be a uint8 [h, w] array or a path, got {a.dtype} {a.shape}")
    if not (1 <= a.shape[0] <= PREP_MAX_HIN and 1 <= a.shape[1] <= PREP_MAX_WIN):
        raise ValueError(f"images[{i}] must be 1..{PREP_MAX_HIN} rows by 1..{PREP_MAX_WIN} columns, got {a.shape}")
    return a


def _check_shape(B: int, height, width) -> tuple[int, int]:
    height = _call.check_int("height", height, PREP_MIN_H, PREP_MAX_H)
    width = _call.check_int("width", width, PREP_MIN_W, PREP_MAX_W)
    if width % 4:
        raise ValueError(f"width = {width} must be a multiple of 4")
    if B * height * width >= 1 << 31:
        raise ValueError(f"{B} images of {height} x {width} hold 2^31 values or more")
    return height, width


def prepare_images(images, height: int = 96, width: int = 1400, thresh: int = 127, device=None):
    """Crop, resize and pad a batch of writer images on the GPU (include/dhw.h dhw_prep).

    images: a list; each item is a uint8 [h,w] array or tensor of grey levels, or the path of an image file.  Each image is
    cropped to its ink (pixels < thresh, the reference's remove_whitespace with its exclusive upper bounds), resized to
    `height` rows keeping the aspect ratio (fixed-point cubic, within one grey level of read_img) and padded white to `width`.
    Returns (imgs f32 [B,1,height,width], widths int32 [B], boxes int32 [B,4] = (r0, r1, c0, c1), status int32 [B]), all on
    the GPU; an image whose status is not 0 (2 = no ink or an empty crop, 4 = wider than `width` after the resize, 8 = resized
    to no column at all) is all white and has width 0."""
    import torch

    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError("images must be a non-empty list of images")
    if len(images) > PREP_MAX_B:
        raise ValueError(f"images must hold at most {PREP_MAX_B} images, got {len(images)}")
    height, width = _check_shape(len(images), height, width)
    thresh = _call.check_int("thresh", thresh, 1, 255)
    host = [_as_image(i, im) for i, im in enumerate(images)]
    with _call.open("prepare_images", device=device, record=True) as c:   # (record: kept as it was, see _call on temporaries)
        B, Hin = len(host), max(a.shape[0] for a in host)
        Win = -(-max(a.shape[1] for a in host) // 16) * 16
        packed = np.full((B, Hin, Win), 255, np.uint8)
        for b, a in enumerate(host):
            packed[b, :a.shape[0], :a.shape[1]] = a
        src = c.to(torch.from_numpy(packed), torch.uint8)
        sizes = c.to(torch.tensor([a.shape for a in host], dtype=torch.int32), torch.int32)
        imgs, widths = c.empty((B, 1, height, width)), c.empty((B,), torch.int32)
        boxes, status = c.empty((B, 4), torch.int32), c.empty((B,), torch.int32)
        ws, need = c.workspace(None, "dhw_prep_workspace_bytes", B)
        c.run("dhw_prep", src.data_ptr(), sizes.data_ptr(), B, Hin, Win, height, width, thresh, imgs.data_ptr(), widths.data_ptr(),
              boxes.data_ptr(), status.data_ptr(), c.ptr(ws), need)
    return imgs, widths, boxes, status


def load_styles(sources, style_weights=None, *, width: int = 1400, batch: int = 32, precision: str = "fp32"):
    """The writer-style features of many handwriting images: ([B,14,1280] f32, widths int32 [B], status int32 [B]), on the GPU.

    `sources` is what prepare_images takes; the images are prepared at 96 rows by `width` columns and run through one cached
    StyleExtractor (`style_weights`, `precision` as StyleExtractor takes them) in chunks of `batch` images.

    This is the reference DATASET's convention (IAMDataset): every style image is padded white to one common width before
    the extractor sees it, so its features differ from load_style's, which follows the reference's `infer` and runs the image
    at its own width.  IAMDataset also keeps a sample only when its CONTENT image's resized width is < img_width: that rule is
    the caller's to apply, with `widths` (and a non-zero status marks an image that gave no crop at all: its features are
    those of a white image)."""
    batch = _call.check_int("batch", batch, 1, PREP_MAX_B)
    if precision not in ("bf16", "fp32"):
        raise ValueError("precision must be 'bf16' or 'fp32'")
    width = _call.check_int("width", width, 96, PREP_MAX_W)   # the extractor needs a 3 x 3 feature map: at least 96 columns
    imgs, widths, _, status = prepare_images(sources, 96, width)
    import torch

    from . import inference
    from .style_extractor import StyleExtractor
    key = str(style_weights) if precision == "fp32" else f"{style_weights}|{precision}"   # (fp32: the extractor load_style caches)
    if key not in inference._extractors:
        inference._extractors[key] = StyleExtractor(style_weights, precision=precision)
    ex = inference._extractors[key]
    return torch.cat([ex(imgs[i:i + batch]) for i in range(0, len(imgs), batch)]), widths, status
