#!/usr/bin/env python3
"""Page compositor benchmark: 64 seeded random-walk lines at L = 488 (the generator of tools/bench_render.py: dx ~ N(0.6, 1),
dy ~ N(0, 1), 8 % pen lifts, a lift on the last stroke) composed onto four 1980 x 1400 pages in one render_page call, and, in
the same session and interleaved call by call, the same 64 lines through render_strokes (64 line images of 96 x 1400).

  page_ms / line_ms    median of --reps timed calls after warm-up, each under hipEvents (both kernels of the call)
  *_bytes_stored       the image bytes the call must write; *_store_GBps = bytes / median time
  workgroups           raster workgroups of the page call, and how many of them a line's placed box reaches (from boxes)
  white_ms / fill_ms   the same page call with every slot off the pages (prepare + headers + white stores only), and a plain
                       fill of the page tensor: what the stores alone cost, in the same interleaved loop

    python tools/bench_page.py [--reps 30] [--out profiles/page.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, L, SEED = 64, 488, 2024
PAGES, H, W, LPP, MARGIN_LEFT, MARGIN_TOP, PITCH, LINE_WIDTH = 4, 1980, 1400, 20, 70.0, 70.0, 92.0, 2.0
LINE_H, LINE_W = 96, 1400
TILE_W, BAND_H = 32, 96   # csrc/page/page_host.h


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page.json"))
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
    geo = dict(pages=PAGES, height=H, width=W, lines_per_page=LPP, margin_left=MARGIN_LEFT, margin_top=MARGIN_TOP, pitch=PITCH,
               line_width=LINE_WIDTH)

    def page():
        return dhg_amd.render_page(strokes, **geo)

    def line():
        return dhg_amd.render_strokes(strokes, height=LINE_H, width=LINE_W, line_width=LINE_WIDTH)

    off = torch.full((N,), PAGES * LPP, dtype=torch.int32, device="cuda")   # every slot off the pages: nothing draws

    def white():
        return dhg_amd.render_page(strokes, None, off, **geo)

    def fill():
        return pages.fill_(255.0)

    for _ in range(3):
        pages, scale, boxes = page()
        line()
        white()
    torch.cuda.synchronize()
    ink_share = round(float((pages < 255).float().mean()), 5)
    ts = {"page": [], "line": [], "white": [], "fill": []}
    for _ in range(a.reps):                       # interleaved: all see the same clocks and the same neighbours
        for name, f in (("page", page), ("line", line), ("white", white), ("fill", fill)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1))

    bx = boxes.cpu().numpy().astype(np.float64)
    r = LINE_WIDTH / 2 + 0.5
    tiles, bands = -(-W // TILE_W), -(-H // BAND_H)
    reached = np.zeros((PAGES, bands, tiles), bool)
    for n in range(N):
        if not bx[n].any():
            continue
        x_lo, x_hi = int(max(0, (bx[n, 0] - r) // TILE_W)), int(min(tiles - 1, (bx[n, 2] + r) // TILE_W))
        y_lo, y_hi = int(max(0, (bx[n, 1] - r) // BAND_H)), int(min(bands - 1, (bx[n, 3] + r) // BAND_H))
        reached[n // LPP, y_lo:y_hi + 1, x_lo:x_hi + 1] = True
    page_bytes, line_bytes = PAGES * H * W * 4, N * LINE_H * LINE_W * 4
    pm, lm = float(np.median(ts["page"])), float(np.median(ts["line"]))
    wm, fm = float(np.median(ts["white"])), float(np.median(ts["fill"]))
    out = {"N": N, "L": L, "pages": PAGES, "H": H, "W": W, "lines_per_page": LPP, "margin_left": MARGIN_LEFT, "margin_top": MARGIN_TOP,
           "pitch": PITCH, "line_width": LINE_WIDTH, "reps": a.reps, "scale": float(scale[0]),
           "page_ms": round(pm, 4), "page_ms_min": round(min(ts["page"]), 4), "page_ms_max": round(max(ts["page"]), 4),
           "page_bytes_stored": page_bytes, "page_store_GBps": round(page_bytes / (pm * 1e-3) / 1e9, 1),
           "line_ms": round(lm, 4), "line_ms_min": round(min(ts["line"]), 4), "line_ms_max": round(max(ts["line"]), 4),
           "line_bytes_stored": line_bytes, "line_store_GBps": round(line_bytes / (lm * 1e-3) / 1e9, 1),
           "workgroups": int(PAGES * tiles * bands), "workgroups_reached_by_a_line": int(reached.sum()),
           "white_ms": round(wm, 4), "white_store_GBps": round(page_bytes / (wm * 1e-3) / 1e9, 1),
           "fill_ms": round(fm, 4), "fill_store_GBps": round(page_bytes / (fm * 1e-3) / 1e9, 1),
           "ink_pixels_share": ink_share, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
