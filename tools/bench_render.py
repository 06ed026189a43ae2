#!/usr/bin/env python3
"""Stroke rasteriser benchmark: 64 lines at L = 488 rendered to 96 x 1400 grey images in one render_strokes call.

The strokes come from `sample` on the synthetic state dict (bf16, T = 60); the last stroke of every line is marked as a pen
lift so that every line draws (nothing after the last lift is drawn).  Recorded:

  render_ms            median of >= 20 timed render_strokes calls after warm-up, each under hipEvents (both kernels)
  store_GBps           the 34.4 MB of image the call must write / render_ms
  kept_segments_*      segments a tile keeps after the cull, over the tiles that hold ink (from the workspace)
  random_walk          the same figures for 64 seeded random-walk lines that advance left to right as handwriting does
  show_strokes_host_s  host time of vis.show_strokes (matplotlib, one figure + PNG per line) for the same 64 lines

    python tools/bench_render.py [--reps 30] [--out profiles/render.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, L, LT, T, H, W, SEED = 64, 488, 30, 60, 96, 1400, 2024


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--no-matplotlib", action="store_true", help="skip the show_strokes host timing")
    a = ap.parse_args(argv)
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dhg_amd
    from dhg_amd import spec, vis

    inp = spec.synthetic_inputs(B, L, LT, seed=SEED, T=1)
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    strokes = dhg_amd.sample(m, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=L, T=T, seed=1)
    strokes[:, L - 1, 2] = 1.0
    torch.cuda.synchronize()

    def measure(strokes):
        """render_ms (median / min / max over a.reps calls, each under hipEvents) and what the cull keeps per inked tile,
        recomputed on the host from the segment list the prepare kernel left in the workspace"""
        for _ in range(3):
            images, widths = dhg_amd.render_strokes(strokes, height=H, width=W)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            images, widths = dhg_amd.render_strokes(strokes, height=H, width=W)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        hdr, segs = vis.render_workspace_segments(strokes.device, B, L)
        tile_w, radius = vis.RENDER_TILE_W, 2.0 / 2 + 0.5
        kept = []
        for b in range(B):
            n, wd = int(hdr[b, 0]), int(hdr[b, 1])
            lo, hi = np.minimum(segs[b, :n, 0], segs[b, :n, 2]), np.maximum(segs[b, :n, 0], segs[b, :n, 2])
            for x0 in range(0, wd, tile_w):
                kept.append(int(((lo < x0 + tile_w + radius) & (hi > x0 - radius)).sum()))
        wd_host = widths.cpu().numpy()
        return {"render_ms": round(ms, 4), "render_ms_min": round(min(ts), 4), "render_ms_max": round(max(ts), 4),
                "store_GBps": round(image_bytes / (ms * 1e-3) / 1e9, 1),
                "segments_per_line_mean": round(float(hdr[:, 0].mean()), 1), "ink_width_mean": round(float(wd_host.mean()), 1),
                "lines_with_ink": int((wd_host > 0).sum()), "tiles_with_ink": len(kept),
                "kept_segments_per_tile_mean": round(float(np.mean(kept)), 2) if kept else 0.0,
                "kept_segments_per_tile_max": int(max(kept)) if kept else 0}

    image_bytes = B * H * W * 4
    sampled = measure(strokes)
    # a second input shaped like handwriting, which advances left to right (the synthetic weights scribble in place): a seeded
    # random walk, dx ~ N(0.6, 1), dy ~ N(0, 1), 8 % pen lifts
    rng = np.random.Generator(np.random.PCG64(SEED))
    walk = np.stack([rng.normal(0.6, 1.0, (B, L)), rng.normal(0.0, 1.0, (B, L)), (rng.random((B, L)) < 0.08).astype(np.float64)], -1)
    walk[:, L - 1, 2] = 1.0
    walked = measure(torch.from_numpy(walk.astype(np.float32)).cuda())

    host_s, host_err = None, None
    if not a.no_matplotlib:
        lines = strokes.cpu().numpy()
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as d:
            os.chdir(d)
            try:
                vis.show_strokes(lines[0], name="warm", show_output=False)
                t0 = time.perf_counter()
                for b in range(B):
                    vis.show_strokes(lines[b], name=f"line_{b}", show_output=False)
                host_s = time.perf_counter() - t0
            except Exception as e:   # (a figure matplotlib refuses: recorded, the GPU figures stand)
                host_err = f"{type(e).__name__}: {e}"
            finally:
                os.chdir(cwd)

    out = {"B": B, "L": L, "H": H, "W": W, "line_width": 2.0, "T": T, "reps": a.reps, "image_MB": round(image_bytes / 1e6, 1),
           "tile_w": vis.RENDER_TILE_W, **sampled, "random_walk": walked,
           "show_strokes_host_s": None if host_s is None else round(host_s, 3),
           "show_strokes_error": host_err, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
