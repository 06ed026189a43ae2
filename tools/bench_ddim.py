#!/usr/bin/env python3
"""What deterministic sampling and inversion cost next to the plain sampler, at bench.py's shape (B = 64, L = 488, Lt = 30,
bf16, synthetic weights, T = 60).  Six calls:

  sample          sample() at T = 60: a replay of its captured graph, 60 denoiser calls
  ddim_60/20/10   sample_ddim() at 60, 20 and 10 levels (ddim_levels): one denoiser call + one small launch per level, eager
  invert_20_i1/2  invert() at 20 levels with 1 and 2 fixed-point iterations: 20 and 40 denoiser calls, eager

The new entries launch eagerly; capturing them into a graph is out of scope.  The variants are timed in turn, round after
round (so drift of the box hits all of them alike): wall time of one call that ends in a device synchronise; median and
quartiles over the rounds, and ms per denoiser call.  No target is set.

    python tools/bench_ddim.py [--reps 30] [--out profiles/ddim.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, L, LT, SEED = 64, 60, 488, 30, 2025


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30, help="timed rounds per variant (at least 30)")
    ap.add_argument("--out", help="also write the JSON result to this file")
    a = ap.parse_args(argv)
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dhg_amd
    from dhg_amd import spec

    if not torch.cuda.is_available():
        raise SystemExit("bench_ddim.py needs the MI355X: there is nothing to time without it")
    inp = spec.synthetic_inputs(B, L, LT, seed=SEED, T=1)
    tx = torch.from_numpy(inp["text"]).cuda()
    sv = torch.from_numpy(inp["style"]).cuda()
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    lines = dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1)

    variants = {"sample": (T, lambda: dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1))}
    for s in (60, 20, 10):
        variants[f"ddim_{s}"] = (s, lambda s=s: dhg_amd.sample_ddim(m, tx, sv, L=L, T=T, steps=s, seed=1))
    for it in (1, 2):
        variants[f"invert_20_i{it}"] = (20 * it, lambda it=it: dhg_amd.invert(m, lines, tx, sv, T=T, steps=20, iters=it))
    outs = {}
    for name, (_, fn) in variants.items():   # graph capture / first-call allocations, then two more warm calls
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
    assert torch.equal(outs["sample"], lines), "a ddim call in between must not change what the sampler's graph computes"
    assert all(torch.isfinite(o).all() for o in outs.values())
    ts = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, (_, fn) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for name, v in ts.items():
        v = np.asarray(v)
        n = variants[name][0]
        res[name] = {"denoiser_calls": n, "ms_median": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                     "ms_p25": round(float(np.percentile(v, 25)), 4), "ms_p75": round(float(np.percentile(v, 75)), 4),
                     "ms_per_call_of_denoiser": round(float(np.median(v)) / n, 4)}
    step = res["sample"]["ms_per_call_of_denoiser"]
    for name in res:
        if name != "sample":
            res[name]["ms_per_call_minus_graph_step"] = round(res[name]["ms_per_call_of_denoiser"] - step, 4)
            res[name]["time_relative_to_sample"] = round(res[name]["ms_median"] / res["sample"]["ms_median"], 4)
    out = {"B": B, "T": T, "L": L, "Lt": LT, "precision": "bf16", "reps": a.reps,
           "timing": "host clock around one call ending in a device synchronise; variants interleaved; sample = graph replay, ddim / invert = eager launches",
           **res, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
