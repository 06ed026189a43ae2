"""The int64 numpy statement of dhw_prep's rules 1 to 8 (include/dhw.h): crop box, output width, status bits, the fixed-point
cubic resize and the white padding, for one image and for a batch.  Test support, not part of the package."""
import numpy as np


def crop_box(img: np.ndarray, thresh: int):
    """Rule 2: (r0, r1, c0, c1) = the first / last row and column holding a pixel < thresh, or None without one."""
    dark = img < thresh
    rows, cols = np.flatnonzero(dark.any(axis=1)), np.flatnonzero(dark.any(axis=0))
    if not len(rows):
        return None
    return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def cubic_taps(n_in: int, n_out: int):
    """Rule 5 for one axis: tap indices [n_out,4] relative to the crop and integer coefficients [n_out,4] (sum 2048)."""
    d = np.arange(n_out, dtype=np.int64)
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    x0 = num // den                                           # floor, also for a negative num
    t = (num - x0 * den).astype(np.float64) / np.float64(den)
    a = -0.75
    w = [((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a,
         ((a + 2) * t - (a + 3)) * t * t + 1,
         ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1]
    c = [np.rint(2048 * wk).astype(np.int64) for wk in w]     # ties to even
    c.append(2048 - c[0] - c[1] - c[2])
    idx = np.clip(x0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, np.stack(c, axis=1)


def resize_sums(crop: np.ndarray, ow: int, H: int) -> np.ndarray:
    """The int64 double sums of rule 5 before the rounding shift, [H, ow] (separable, the horizontal pass first)."""
    f = crop.astype(np.int64)
    idx, c = cubic_taps(f.shape[1], ow)
    f = (f[:, idx] * c[None]).sum(-1)
    idx, c = cubic_taps(f.shape[0], H)
    return (f[idx] * c[:, :, None]).sum(1)


def resize_fixed(crop: np.ndarray, ow: int, H: int) -> np.ndarray:
    """Rule 5: u8 [H, ow]."""
    return np.clip((resize_sums(crop, ow, H) + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def prep_ref(img, H: int, W: int, thresh: int = 127):
    """One image (u8 [h,w]: exactly the valid region; None = a size that does not fit its slot) ->
    (out f32 [H,W], width, box int32 [4], status)."""
    out, box = np.full((H, W), 255, np.float32), np.zeros(4, np.int32)
    if img is None:
        return out, 0, box, 1
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and img.size
    bx = crop_box(img, thresh)
    if bx is None:
        return out, 0, box, 2
    box[:] = bx
    r0, r1, c0, c1 = bx
    ch, cw = r1 - r0, c1 - c0
    if ch == 0 or cw == 0:
        return out, 0, box, 2
    ow = H * cw // ch
    if ow > W:
        return out, 0, box, 4
    if ow == 0:
        return out, 0, box, 8
    out[:, :ow] = resize_fixed(img[r0:r1, c0:c1], ow, H)
    return out, ow, box, 0


def prep_batch_ref(images, H: int, W: int, thresh: int = 127):
    """(out f32 [B,1,H,W], widths int32 [B], boxes int32 [B,4], status int32 [B]) of a list of images (rule 8: one by one)."""
    parts = [prep_ref(im, H, W, thresh) for im in images]
    return (np.stack([p[0] for p in parts])[:, None], np.array([p[1] for p in parts], np.int32),
            np.stack([p[2] for p in parts]).astype(np.int32), np.array([p[3] for p in parts], np.int32))
