#!/usr/bin/env python3
"""Encode IAM-OnDB lineStrokes files into the model's strokes on the GPU and write the padded array [B,L,3] that
infer.py --restyle / --align / --score read.

    python tools/encode_strokes.py a01-000u-01.xml a01-000u-02.xml --out lines.npy [--length L] [--rounds 3] [--max-abs 15]

Prints each line's length (rows before the padding) and status (0 = encoded; 2 = non-finite or constant input, 4 = longer
than L, 8 = an offset above --max-abs: such a line is all padding).  Exit status 1 if any line was not encoded."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("xml", nargs="+", help="lineStrokes files, one line of handwriting each")
    ap.add_argument("--out", required=True, help="the .npy file to write")
    ap.add_argument("--length", type=int, default=None, help="rows per line (default: the longest line's bound, a multiple of 8)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-abs", type=float, default=15.0)
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import numpy as np

    import dhg_amd

    lines = [dhg_amd.read_strokes_xml(p) for p in a.xml]
    strokes, lengths, status = dhg_amd.encode_strokes(lines, L=a.length, rounds=a.rounds, max_abs=a.max_abs)
    lengths, status = lengths.cpu().tolist(), status.cpu().tolist()
    for p, n, s in zip(a.xml, lengths, status):
        print(f"{p}: length {n} status {s}")
    np.save(a.out, strokes.cpu().numpy())
    print(f"wrote {a.out}: {tuple(strokes.shape)}")
    return 1 if any(status) else 0


if __name__ == "__main__":
    sys.exit(main())
