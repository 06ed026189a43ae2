#!/usr/bin/env python3
"""Vector output benchmark: 1024 seeded random-walk lines of 488 rows (offsets on the 1/16 grid of tests/page_ref.make_strokes,
8 % pen lifts, a lift on the last row) through dhg_amd.stroke_paths at its defaults (52 pages of 1980 x 1400, smooth 1,
tol 0.25, rounds 4), next to tests/paths_ref.py, the numpy statement of the same rules, on the host's cores.

  paths_ms             median of --reps timed calls after warm-up, each under hipEvents (both kernels of the call; strokes
                       already on the device, outputs left there), with the smallest and the largest
  paths_batch_ms       the mean of --reps back-to-back calls under one pair of events: what a caller in a loop sees
  bytes_moved, GBps    what the call must read (the strokes, twice: each kernel scans them) and write (points and index,
                       every row), and that over the median time
  host_ms_1            paths_ref on one core, the whole batch in one call (the automatic scale included)
  host_ms_pool         the same lines in --workers chunks, one process each, at the scale the first pass found (wall time of
                       the pool's map: the processes are started, and have imported numpy, before the clock starts)
  identical            the device's five outputs have the bits of the host's

    python tools/bench_paths.py [--reps 50] [--workers 16] [--out profiles/paths.json]
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, L, SEED = 1024, 488, 2024


def make_lines():
    import numpy as np
    import page_ref
    st = page_ref.make_strokes(np.random.Generator(np.random.PCG64(SEED)), N, L, lift_p=0.08)
    st[:, L - 1, 2] = 0.98
    return st


def _ready(_):
    import paths_ref  # noqa: F401
    return os.getpid()


def _chunk(args):
    import paths_ref
    st, slots, scale, pages = args
    return paths_ref.paths_ref(st, None, slots, pages=pages, height=1980, width=1400, lines_per_page=20, margin_left=70.0, margin_top=70.0,
                               pitch=92.0, scale=scale)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths.json"))
    a = ap.parse_args(argv)
    if a.reps < 20 or a.workers < 1:
        ap.error("--reps must be at least 20 and --workers at least 1")
    import numpy as np
    import paths_ref

    st = make_lines()
    pages = -(-N // 20)
    geo = dict(pages=pages, height=1980, width=1400, lines_per_page=20, margin_left=70.0, margin_top=70.0, pitch=92.0)

    # the host first, and its processes started before this one opens the device
    t0 = time.perf_counter()
    want = paths_ref.paths_ref(st, **geo)
    host_1 = (time.perf_counter() - t0) * 1e3
    scale = float(want["scale"][0])
    bounds = np.linspace(0, N, a.workers + 1).astype(int)
    jobs = [(st[lo:hi], list(range(lo, hi)), scale, pages) for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
    with multiprocessing.get_context("spawn").Pool(a.workers) as pool:
        pool.map(_ready, range(4 * a.workers))
        t0 = time.perf_counter()
        parts = pool.map(_chunk, jobs, chunksize=1)
        host_pool = (time.perf_counter() - t0) * 1e3
    for k in ("points", "index", "counts", "boxes"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), want[k]), k

    import torch

    import dhg_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_paths needs an MI355X (HIP device): nothing is timed without one")
    strokes = torch.from_numpy(st).cuda()

    def call():
        return dhg_amd.stroke_paths(strokes, **geo)

    for _ in range(5):
        got = call()
    torch.cuda.synchronize()
    identical = all(np.array_equal(getattr(got, k).cpu().numpy().view(np.uint32), want[k].view(np.uint32)) for k in ("points", "index", "counts", "scale", "boxes"))
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        call()
    e1.record()
    e1.synchronize()
    batch = e0.elapsed_time(e1) / a.reps

    med = float(np.median(ts))
    moved = 2 * N * L * 12 + N * L * (16 + 8)
    kept = want["counts"][:, 0]
    out = {"N": N, "L": L, **geo, "smooth": 1, "tol": 0.25, "rounds": 4, "reps": a.reps, "scale": scale,
           "path_points": int(paths_ref.paths_ref(st, scale=scale, smooth=0, rounds=0, **geo)["counts"][:, 0].sum()),
           "kept_points": int(kept.sum()), "polylines": int(want["counts"][:, 1].sum()),
           "paths_ms": round(med, 4), "paths_ms_min": round(min(ts), 4), "paths_ms_max": round(max(ts), 4), "paths_batch_ms": round(batch, 4),
           "bytes_moved": moved, "GBps": round(moved / (med * 1e-3) / 1e9, 1),
           "host_ms_1": round(host_1, 1), "host_ms_pool": round(host_pool, 1), "workers": a.workers,
           "host_1_over_device": round(host_1 / med, 1), "host_pool_over_device": round(host_pool / med, 1),
           "identical": bool(identical), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
