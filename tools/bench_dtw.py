#!/usr/bin/env python3
"""Dynamic-time-warping benchmark (include/dhw.h dhw_dtw): synthetic pen lines (the rows of
tools/eval_samples.py --synthetic) turned into features by dhg_amd.stroke_features, every line at its full length.

  all pairs    one call at M = N = 1024, La = Lb = 488, F = 3: `dist_steps` (dist_out + steps_out, normalised) and `nearest_only`
               (nearest_out + nearest_idx, not normalised: the K carry is compiled out and the matrix stays in the workspace)
  yardstick    at M = N = 256 the `dist_steps` call alternates with what one would write without the kernel: torch ops over all
               pairs, one anti-diagonal at a time (it lives in this tool only; the product never calls it)

Every call is timed under device events after warm-up calls; medians with min .. max.  gcups = M N La Lb / time / 1e9, the cell
updates per second.  `agree`: the largest absolute difference between the entry's distances and the yardstick's, and whether the
path lengths are equal.  No time is asserted anywhere.

    python tools/bench_dtw.py [--out profiles/dtw.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, F = 488, 3
BIG, SMALL = (1024, 3, 10), (256, 1, 3)   # lines per set, warm-up calls, timed calls


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ctypes as C

    import numpy as np
    import torch

    import dhg_amd
    from dhg_amd import _lib
    from eval_samples import synthetic_rows

    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms, cells):
        m = float(np.median(ms))
        return {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "gcups": round(cells / (m * 1e-3) / 1e9, 2)}

    def sets(n, seed):
        return [dhg_amd.stroke_features(synthetic_rows(n, L, 8, seed=s)["strokes"]).contiguous() for s in (seed, seed + 100)]

    def entry(fa, fb, mode):
        n = fa.shape[0]
        need = int(lib.dhw_dtw_workspace_bytes(n, n, L, L, F))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        dist, steps = torch.empty((n, n), dtype=torch.float32, device="cuda"), torch.empty((n, n), dtype=torch.int32, device="cuda")
        near, idx = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        outs = (dist.data_ptr(), steps.data_ptr(), None, None) if mode == "dist_steps" else (None, None, near.data_ptr(), idx.data_ptr())

        def call():
            _lib.check(lib.dhw_dtw(fa.data_ptr(), None, n, L, fb.data_ptr(), None, n, L, F, int(mode == "dist_steps"), 0, *outs, ws.data_ptr(), need,
                                   stream))
        return call, (dist, steps, near, idx, ws)

    def yardstick(fa, fb):
        """(dist, steps) of every pair, full lengths, by the rules of include/dhw.h one anti-diagonal at a time."""
        M, N = fa.shape[0], fb.shape[0]
        inf = float("inf")
        d1 = torch.full((M, N, L + 1), inf, device="cuda")
        k1 = torch.zeros((M, N, L + 1), dtype=torch.int32, device="cuda")
        d2, k2 = d1.clone(), k1.clone()
        sq = fa[:, None, 0] - fb[None, :, 0]
        sq = sq * sq
        d1[:, :, 1] = sq[..., 0] + sq[..., 1] + sq[..., 2]
        k1[:, :, 1] = 1
        for d in range(1, 2 * L - 1):
            lo, hi = max(0, d - L + 1), min(L - 1, d)
            i = torch.arange(lo, hi + 1, device="cuda")
            sq = fa[:, None, i] - fb[None, :, d - i]
            sq = sq * sq
            c = sq[..., 0] + sq[..., 1] + sq[..., 2]
            best, kb = d2[:, :, lo:hi + 1], k2[:, :, lo:hi + 1]
            up, ku = d1[:, :, lo:hi + 1], k1[:, :, lo:hi + 1]
            w = up < best
            best, kb = torch.where(w, up, best), torch.where(w, ku, kb)
            left, kl = d1[:, :, lo + 1:hi + 2], k1[:, :, lo + 1:hi + 2]
            w = left < best
            best, kb = torch.where(w, left, best), torch.where(w, kl, kb)
            d2, k2, d1, k1 = d1, k1, d2, k2          # the buffers of d - 2 become those of d
            d1.fill_(inf)
            d1[:, :, lo + 1:hi + 2] = c + best
            k1[:, :, lo + 1:hi + 2] = kb + 1
        return d1[:, :, L] / k1[:, :, L].float(), k1[:, :, L].clone()

    out = {"L": L, "F": F, "device": torch.cuda.get_device_name(0)}
    n, warm, reps = BIG
    fa, fb = sets(n, 2026)
    cells = float(n) * n * L * L
    res = {}
    for mode in ("dist_steps", "nearest_only"):
        call, keep = entry(fa, fb, mode)
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        res[mode] = stats([timed(call) for _ in range(reps)], cells)
    res["workspace_mb"] = round(int(lib.dhw_dtw_workspace_bytes(n, n, L, L, F)) / 2 ** 20, 1)
    out["all_pairs_1024"] = res
    print(1024, json.dumps(res), flush=True)

    n, warm, reps = SMALL
    fa, fb = sets(n, 2027)
    cells = float(n) * n * L * L
    call, (dist, steps, _, _, _) = entry(fa, fb, "dist_steps")
    for _ in range(warm):
        call()
        yardstick(fa, fb)
    torch.cuda.synchronize()
    times = {"dist_steps": [], "torch_antidiagonals": []}
    for _ in range(reps):
        times["dist_steps"].append(timed(call))
        times["torch_antidiagonals"].append(timed(lambda: yardstick(fa, fb)))
    res = {name: stats(ms, cells) for name, ms in times.items()}
    res["ratio"] = round(res["torch_antidiagonals"]["ms"] / res["dist_steps"]["ms"], 1)
    yd, yk = yardstick(fa, fb)
    torch.cuda.synchronize()
    res["agree_dist_abs"] = float((yd - dist).abs().max())
    res["agree_steps"] = bool(torch.equal(yk, steps))
    out["yardstick_256"] = res
    print(256, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
