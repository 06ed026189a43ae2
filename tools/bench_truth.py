#!/usr/bin/env python3
"""Page ground truth benchmark: the 64 seeded random-walk lines of tools/bench_page.py (L = 488, four 1980 x 1400 pages) with
groups of 8 stroke rows (G = 61) through group_boxes without and with the label map, and, in the same session and interleaved
rep by rep, the same lines through render_page, the yardstick: a label map is a page with an id next to every distance.

  boxes_ms / labels_ms / page_ms    median of --reps timed calls after warm-up, each under hipEvents (every kernel of the call)
  labels_over_page                   labels_ms / page_ms

No speed is promised and nothing is thresholded; both figures are recorded.

    python tools/bench_truth.py [--reps 30] [--out profiles/truth.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, L, SEED, ROWS = 64, 488, 2024, 8
G = L // ROWS
PAGES, H, W, LPP, MARGIN_LEFT, MARGIN_TOP, PITCH, LINE_WIDTH = 4, 1980, 1400, 20, 70.0, 70.0, 92.0, 2.0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truth.json"))
    a = ap.parse_args(argv)
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dhg_amd

    rng = np.random.Generator(np.random.PCG64(SEED))
    walk = np.stack([rng.normal(0.6, 1.0, (N, L)), rng.normal(0.0, 1.0, (N, L)), (rng.random((N, L)) < 0.08).astype(np.float64)], -1)
    walk[:, L - 1, 2] = 1.0
    strokes = torch.from_numpy(walk.astype(np.float32)).cuda()
    groups = (torch.arange(L, dtype=torch.int32, device="cuda") // ROWS).repeat(N, 1)
    geo = dict(pages=PAGES, height=H, width=W, lines_per_page=LPP, margin_left=MARGIN_LEFT, margin_top=MARGIN_TOP, pitch=PITCH,
               line_width=LINE_WIDTH)

    def boxes():
        return dhg_amd.group_boxes(strokes, groups, G, **geo)

    def labels():
        return dhg_amd.group_boxes(strokes, groups, G, labels=True, **geo)

    def page():
        return dhg_amd.render_page(strokes, **geo)

    for _ in range(3):
        boxes()
        rec = labels()
        pages, scale, _ = page()
    torch.cuda.synchronize()
    disagree = int(((rec.labels > 0) != (pages < 255)).sum())
    ts = {"boxes": [], "labels": [], "page": []}
    for _ in range(a.reps):                       # interleaved: all see the same clocks and the same neighbours
        for name, f in (("boxes", boxes), ("labels", labels), ("page", page)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1))

    med = {k: float(np.median(v)) for k, v in ts.items()}
    out = {"N": N, "L": L, "G": G, "rows_per_group": ROWS, "pages": PAGES, "H": H, "W": W, "lines_per_page": LPP, "margin_left": MARGIN_LEFT,
           "margin_top": MARGIN_TOP, "pitch": PITCH, "line_width": LINE_WIDTH, "reps": a.reps, "scale": float(scale[0]),
           "groups_that_draw": int((rec.spans[..., 2] > 0).sum()), "labelled_pixels": int((rec.labels > 0).sum()),
           "pixels_where_labels_and_page_disagree": disagree}
    for k in ("boxes", "labels", "page"):
        out.update({f"{k}_ms": round(med[k], 4), f"{k}_ms_min": round(min(ts[k]), 4), f"{k}_ms_max": round(max(ts[k]), 4)})
    out.update(labels_over_page=round(med["labels"] / med["page"], 3), boxes_over_page=round(med["boxes"] / med["page"], 3),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
