"""Write the stroke encoder's fixtures (tests/golden/encode_lines.npz, tests/golden/encode_line.xml) from the reference.

    python tools/make_encode_golden.py --reference <checkout of the reference project>

Runs only where the reference is at hand.  Deterministic synthetic pen lines (integer tablet coordinates, several pen-down
strokes per line, numpy PCG64) are written as IAM-layout lineStrokes files and fed to the reference's parse_strokes_xml
(+ combine_strokes) and pad_stroke_seq; the fixtures hold the inputs, the reference's float64 rows, whether it dropped the
line, and per round the gap between the k-th and (k+1)-th smallest merge key.  A line is reseeded until every gap is >= 1e-9
and no round has more exact-zero keys than k: the merged set then depends neither on the sort's tie handling nor on last-bit
rounding.  cv2 and torchvision, which the reference imports but these functions do not use, are empty placeholder modules."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import encode_ref  # noqa: E402

LENGTHS = (6, 7, 9, 40, 65, 66, 258, 333, 700, 1500)
JUMP_LENGTH = 400      # the extra line with one far jump: the reference drops it for max_abs
MAX_SEQ_LEN = 480      # the 1500-point line ends at 768 rows: the reference drops it for max_seq_len
MIN_GAP = 1e-9


def pen_line(n: int, seed: int, far_jump: bool = False) -> np.ndarray:
    """n tablet points [n,3] = (x, y, end): smooth loops drifting to the right, cut into pen-down strokes of 5 to 40 points."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) * g.uniform(0.25, 0.45) + g.uniform(0, 6)
    x = 900 + np.cumsum(g.uniform(4, 14, n)) + 60 * np.sin(t) + g.normal(0, 1.5, n)
    y = 2400 + 90 * np.cos(t * g.uniform(0.9, 1.1)) + 30 * np.sin(0.31 * t) + g.normal(0, 1.5, n)
    end = np.zeros(n)
    i = 0
    while i < n:
        i += int(g.integers(5, 41)) if n > 12 else int(g.integers(2, 5))
        end[min(i, n) - 1] = 1
        if i < n:                                   # the pen lands somewhere else
            x[i:] += g.uniform(20, 120)
            y[i:] += g.uniform(-40, 40)
    if far_jump:
        cut = int(np.flatnonzero(end)[len(np.flatnonzero(end)) // 2]) + 1
        x[cut:] += 100000
    end[-1] = 1
    return np.stack([np.rint(x), np.rint(y), end], axis=1).astype(np.float32)


def write_xml(path: str, pts: np.ndarray) -> None:
    """The IAM-OnDB lineStrokes layout: WhiteboardCaptureSession / StrokeSet / Stroke / Point."""
    out = ['<?xml version="1.0" encoding="ISO-8859-1"?>', "<WhiteboardCaptureSession>", "  <WhiteboardDescription>",
           '    <SensorLocation corner="top_left"/>', "  </WhiteboardDescription>", "  <StrokeSet>"]
    time, open_ = 0.0, False
    for x, y, e in pts:
        if not open_:
            out.append(f'    <Stroke colour="black" start_time="{time:.2f}" end_time="{time:.2f}">')
            open_ = True
        out.append(f'      <Point x="{int(x)}" y="{int(y)}" time="{time:.2f}"/>')
        time += 0.01
        if e:
            out.append("    </Stroke>")
            open_ = False
    out += ["  </StrokeSet>", "</WhiteboardCaptureSession>", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="directory of the reference project (holds diffusion_handwriting_generation/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args(argv)
    for name in ("cv2", "torchvision", "torchvision.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.path.insert(0, a.reference)
    from diffusion_handwriting_generation.utils.io import parse_strokes_xml
    from diffusion_handwriting_generation.utils.preprocessing import pad_stroke_seq

    data, seed = {}, 0
    cases = [(n, False) for n in LENGTHS] + [(JUMP_LENGTH, True)]
    with tempfile.TemporaryDirectory() as tmp:
        for c, (n, far) in enumerate(cases):
            while True:
                seed += 1
                pts = pen_line(n, seed, far)
                gaps = []
                mine, ok = encode_ref.encode_rows(pts, 3, gaps)
                if ok and all(gap >= MIN_GAP and zeros <= k for gap, zeros, k in gaps):
                    break
                print(f"case {c} (n = {n}): seed {seed} rejected, gaps {gaps}")
            path = os.path.join(tmp, f"line{c}.xml")
            write_xml(path, pts)
            rows = parse_strokes_xml(path)                       # float64 [M,3]
            padded = pad_stroke_seq(rows.copy(), maxlength=MAX_SEQ_LEN)
            assert rows.shape == mine.shape and np.abs(rows - mine).max() < 1e-9, (c, rows.shape, mine.shape)
            data[f"points_{c}"], data[f"rows_{c}"] = pts, rows
            data[f"dropped_{c}"] = np.array(padded is None)
            data[f"gaps_{c}"] = np.array([gap for gap, _, _ in gaps])
            if padded is not None:
                data[f"padded_{c}"] = padded
            print(f"case {c}: n {n} seed {seed} rows {len(rows)} dropped {padded is None} max|d| {np.abs(rows[:, :2]).max():.3f} "
                  f"min gap {min(gap for gap, _, _ in gaps):.3g}")
            if n == 40:
                write_xml(os.path.join(a.out, "encode_line.xml"), pts)
                data["xml_case"] = np.array(c)
    data["max_seq_len"] = np.array(MAX_SEQ_LEN)
    np.savez_compressed(os.path.join(a.out, "encode_lines.npz"), **data)
    print("wrote", os.path.join(a.out, "encode_lines.npz"), os.path.getsize(os.path.join(a.out, "encode_lines.npz")), "bytes")


if __name__ == "__main__":
    main()
