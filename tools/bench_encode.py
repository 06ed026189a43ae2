#!/usr/bin/env python3
"""Stroke encoder benchmark: B = 1024 seeded synthetic pen lines of 700 points (integer tablet coordinates, pen-down strokes of
5 to 40 points), rounds = 3, L = 480, through one dhw_encode call on device-resident points, next to the float64 numpy
statement of the rules (tests/encode_ref.py) on the host's cores for the same lines.

  gpu_ms           median of --reps timed calls (at least 20) after 3 warm-up calls, each under hipEvents: the kernel alone,
                   points already on the device (the wrapper's host-to-device copy of 8.6 MB is not in it)
  wrapper_ms       dhg_amd.encode_strokes on the host lists (padding, copy, call), host clock around a device synchronise
  cpu_ms           tests/encode_ref.py over the same lines in a process pool of --workers, host clock, best of 2
  agree            lengths, status and pen equal, dx / dy at most one f32 step (or 1e-12) apart, on every line

    python tools/bench_encode.py [--reps 20] [--workers 16] [--out profiles/encode.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, N, L, ROUNDS, SEED = 1024, 700, 480, 3, 2025


def pen_line(n, seed):
    import numpy as np
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) * g.uniform(0.25, 0.45)
    x = 900 + np.cumsum(g.uniform(4, 14, n)) + 60 * np.sin(t) + g.normal(0, 1.5, n)
    y = 2400 + 90 * np.cos(1.07 * t) + 30 * np.sin(0.31 * t) + g.normal(0, 1.5, n)
    end = np.zeros(n)
    i = 0
    while i < n:
        i += int(g.integers(5, 41))
        end[min(i, n) - 1] = 1
        if i < n:
            x[i:] += g.uniform(20, 120)
    return np.stack([np.rint(x), np.rint(y), end], axis=1).astype(np.float32)


def _cpu_chunk(lines):
    import encode_ref
    return encode_ref.encode_batch_ref(lines, L, ROUNDS)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode.json"))
    a = ap.parse_args(argv)
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    sys.path.insert(0, ROOT)
    import ctypes as C
    from concurrent.futures import ProcessPoolExecutor

    import numpy as np
    import torch

    import dhg_amd
    from dhg_amd import _lib

    lines = [pen_line(N, SEED + b) for b in range(B)]

    # the host's cores first: the pool forks before this process has touched the GPU
    chunks = [lines[i::a.workers] for i in range(a.workers)]
    cpu = []
    with ProcessPoolExecutor(a.workers) as ex:
        for _ in range(2):
            t0 = time.perf_counter()
            parts = list(ex.map(_cpu_chunk, chunks))
            cpu.append((time.perf_counter() - t0) * 1e3)
    ref_s, ref_l, ref_st = (np.empty((B, L, 3), np.float32), np.empty(B, np.int32), np.empty(B, np.int32))
    for i, (s, l, st) in enumerate(parts):
        ref_s[i::a.workers], ref_l[i::a.workers], ref_st[i::a.workers] = s, l, st

    points = torch.from_numpy(np.stack(lines)).cuda()
    strokes = torch.empty((B, L, 3), device="cuda")
    lens = torch.empty((B,), device="cuda", dtype=torch.int32)
    status = torch.empty((B,), device="cuda", dtype=torch.int32)
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.dhw_encode(points.data_ptr(), None, B, N, L, ROUNDS, 15.0, strokes.data_ptr(), lens.data_ptr(), status.data_ptr(),
                                  None, 0, stream))

    for _ in range(3):
        call()
        dhg_amd.encode_strokes(lines, L=L, rounds=ROUNDS)
    torch.cuda.synchronize()
    gpu, wrap = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        gpu.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        dhg_amd.encode_strokes(lines, L=L, rounds=ROUNDS)
        torch.cuda.synchronize()
        wrap.append((time.perf_counter() - t0) * 1e3)

    # dx / dy: one f32 step, or 1e-12 where a merged offset cancels to the fp64 noise around 0 (there an f32 step means nothing)
    got = strokes.cpu().numpy()
    diff = np.abs(got[..., :2].astype(np.float64) - ref_s[..., :2])
    step = np.spacing(np.maximum(np.abs(got[..., :2]), np.abs(ref_s[..., :2])))
    agree = bool(np.array_equal(lens.cpu().numpy(), ref_l) and np.array_equal(status.cpu().numpy(), ref_st)
                 and np.array_equal(got[..., 2], ref_s[..., 2]) and (diff <= step + 1e-12).all())
    gm = float(np.median(gpu))
    out = {"B": B, "N": N, "L": L, "rounds": ROUNDS, "reps": a.reps, "gpu_ms": round(gm, 4), "gpu_ms_min": round(min(gpu), 4),
           "gpu_ms_max": round(max(gpu), 4), "gpu_lines_per_s": round(B / (gm * 1e-3)), "wrapper_ms": round(float(np.median(wrap)), 3),
           "cpu_workers": a.workers, "cpu_ms": round(min(cpu), 1), "cpu_lines_per_s": round(B / (min(cpu) * 1e-3)),
           "rows_out": int(ref_l[0]), "max_abs_diff": float(diff.max()), "values_not_bit_equal": int((diff > 0).sum()), "agree": agree, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
