#!/usr/bin/env python3
"""Prepare writer images on the GPU (crop, cubic resize to 96 rows, white padding to one width), run them through the
StyleExtractor in batches and write the features [B,14,1280] that make_batches and train.py --data take as `style`.

    python tools/extract_styles.py a01-000u-01.png a01-000u-02.png --weights mobilenet_v2.pth --out styles.npy [--width 1400] [--batch 32]

Prints each image's resized width and status (0 = prepared; 2 = no ink or an empty crop, 4 = wider than --width, 8 = resized to
no column: such an image went in all white).  The reference's dataset keeps a sample only when its content image's width is
< --width: apply that rule with the printed widths.  Exit status 1 if any image was not prepared."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("images", nargs="+", help="image files, one line of handwriting each")
    ap.add_argument("--weights", default=None, help="torchvision MobileNetV2 state_dict file (default: random initialisation)")
    ap.add_argument("--out", required=True, help="the .npy file to write")
    ap.add_argument("--width", type=int, default=1400)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import numpy as np

    import dhg_amd

    styles, widths, status = dhg_amd.load_styles(a.images, a.weights, width=a.width, batch=a.batch, precision=a.precision)
    widths, status = widths.cpu().tolist(), status.cpu().tolist()
    for p, w, s in zip(a.images, widths, status):
        print(f"{p}: width {w} status {s}")
    np.save(a.out, styles.cpu().numpy())
    print(f"wrote {a.out}: {tuple(styles.shape)}")
    return 1 if any(status) else 0


if __name__ == "__main__":
    sys.exit(main())
