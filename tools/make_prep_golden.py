"""Write the writer-image preparation's fixtures (tests/golden/prep_images.npz) from the reference.

    python tools/make_prep_golden.py --reference <checkout of the reference project>

Runs only where the reference is at hand.  Eight deterministic synthetic grey images (numpy PCG64, at most 64 x 256) go through
the reference's remove_whitespace(img, 127) and, for x = the fixed-point resize of that crop (tests/prep_ref.py: the reference
resizes with cv2, which is not importable here and whose parity stays unpinned), through its pad_img(x, W, H).  The fixtures
hold the images, the reference's crops and its padded float32 outputs.  cv2 and torchvision, which the reference imports but
these functions do not use, are empty placeholder modules."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prep_ref  # noqa: E402

H, W, THRESH = 32, 160, 127


def text_like(h: int, w: int, seed: int, margin=(5, 4, 9, 7)) -> np.ndarray:
    """A white page with a few light specks (never dark) and dark pen-like loops inside the margins (top, bottom, left, right)."""
    g = np.random.Generator(np.random.PCG64(seed))
    img = np.full((h, w), 255, np.uint8)
    speck = g.random((h, w)) < 0.05
    img[speck] = g.integers(140, 250, int(speck.sum()))
    top, bottom, left, right = margin
    ys, xs = h - top - bottom, w - left - right
    t = np.linspace(0, 1, 6 * w)
    x = left + t * (xs - 1)
    y = top + (ys - 1) * (0.5 + 0.5 * np.sin(t * g.uniform(25, 40) + g.uniform(0, 6)) * np.cos(t * g.uniform(3, 9)))
    pen = np.sin(t * g.uniform(40, 70)) > -0.6                      # the pen lifts now and then
    r, c = np.rint(y[pen]).astype(int), np.rint(x[pen]).astype(int)
    img[r, c] = g.integers(0, 110, len(r))
    img[np.clip(r + 1, 0, h - bottom - 1), c] = g.integers(30, 126, len(r))
    img[top, left], img[h - bottom - 1, w - right - 1] = 0, 0        # the box is the margins' exactly
    return img


def cases() -> list:
    out = [text_like(48, 200, 1)]                                    # 0: a line with margins, downscaled
    out.append(text_like(40, 180, 2, margin=(0, 0, 0, 0)))           # 1: ink touching all four image edges
    two = np.full((20, 40), 255, np.uint8)                           # 2: ink in exactly two rows: the crop is one row
    two[7, 10:15], two[8, 11:14] = (0, 90, 126, 40, 10), (60, 0, 100)
    out.append(two)
    thr = np.full((24, 64), 255, np.uint8)                           # 3: 126 is dark, 127 and 128 are not: they lie outside the
    thr[4:18, 8:50] = 128                                            #    box of the 126s and must not move it
    thr[6, 12], thr[15, 40], thr[10, 25] = 126, 126, 126
    thr[2, 30], thr[20, 30], thr[10, 3], thr[10, 60] = 127, 127, 127, 128
    out.append(thr)
    out.append(text_like(16, 44, 5, margin=(3, 3, 6, 7)))            # 4: a 9-row crop, upscaled
    out.append(text_like(64, 256, 6, margin=(1, 2, 3, 2)))           # 5: the largest image, downscaled by 2
    out.append(text_like(40, 120, 7, margin=(4, 3, 10, 9)))          # 6: 33 inked rows: ch = 32 = H, the identity resize
    g = np.random.Generator(np.random.PCG64(8))
    out.append(g.integers(0, 256, (20, 70)).astype(np.uint8))        # 7: noise, every grey level on both sides of the threshold
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="directory of the reference project (holds diffusion_handwriting_generation/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args(argv)
    for name in ("cv2", "torchvision", "torchvision.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.path.insert(0, a.reference)
    from diffusion_handwriting_generation.utils.preprocessing import pad_img, remove_whitespace

    data = {"H": np.array(H), "W": np.array(W), "thresh": np.array(THRESH)}
    for i, img in enumerate(cases()):
        assert img.dtype == np.uint8 and img.shape[0] <= 64 and img.shape[1] <= 256
        crop = remove_whitespace(img, THRESH)
        out, ow, box, status = prep_ref.prep_ref(img, H, W, THRESH)
        assert status == 0 and crop.shape == (box[1] - box[0], box[3] - box[2]), (i, status, crop.shape, box)
        x = prep_ref.resize_fixed(crop, ow, H)
        padded = pad_img(x, W, H)
        assert padded.dtype == np.float32 and padded.shape == (H, W)
        data[f"image_{i}"], data[f"crop_{i}"], data[f"padded_{i}"] = img, crop, padded
        print(f"case {i}: image {img.shape} crop {crop.shape} box {box.tolist()} ow {ow}")
    path = os.path.join(a.out, "prep_images.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
