#!/usr/bin/env python3
"""What conditioned sampling costs on top of the plain sampler, at bench.py's shape (B = 64, T = 60, L = 488, Lt = 30, bf16,
synthetic weights).  Four calls, each a replay of its own captured graph:

  plain        sample() without conditioning arguments
  cond_empty   known given, keep all zero, t_start = T      (start + one replace launch per step + finish, nothing written)
  cond_half    every second row kept, t_start = T           (the same launches, half the rows rewritten)
  restyle_half nothing kept, t_start = T/2                  (half the iterations)

The variants are timed in turn, round after round (so drift of the box hits all of them alike): wall time of one call that
ends in a device synchronise, median over the rounds.  per_step_extra_us = (variant - plain) / T: what the extra launches of
one sampler step cost.

    python tools/bench_cond.py [--reps 30] [--out profiles/cond.json]
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
    ap.add_argument("--reps", type=int, default=30, help="timed graph replays per variant (at least 30)")
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
        raise SystemExit("bench_cond.py needs the MI355X: there is nothing to time without it")
    inp = spec.synthetic_inputs(B, L, LT, seed=SEED, T=1)
    tx = torch.from_numpy(inp["text"]).cuda()
    sv = torch.from_numpy(inp["style"]).cuda()
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    g = torch.Generator().manual_seed(SEED)
    known = torch.randn((B, L, 3), generator=g)
    known[..., 2] = (known[..., 2] > 0).float()
    known = known.cuda()
    empty = torch.zeros((B, L), dtype=torch.uint8, device="cuda")
    half = empty.clone()
    half[:, ::2] = 1

    variants = {
        "plain": lambda: dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1),
        "cond_empty": lambda: dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1, known=known, keep=empty, t_start=T),
        "cond_half": lambda: dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1, known=known, keep=half, t_start=T),
        "restyle_half": lambda: dhg_amd.sample(m, tx, sv, L=L, T=T, seed=1, known=known, t_start=T // 2),
    }
    outs = {}
    for name, fn in variants.items():   # graph capture, then two more warm replays of every shape that is timed
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
    assert torch.equal(outs["plain"], outs["cond_empty"]), "nothing kept at t_start = T must be the plain call, bit for bit"
    assert torch.equal(outs["cond_half"][:, ::2], known[:, ::2]), "kept rows must come back as known"
    ts = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for name, v in ts.items():
        v = np.asarray(v)
        res[name] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                     "ms_p25": round(float(np.percentile(v, 25)), 4), "ms_p75": round(float(np.percentile(v, 75)), 4)}
    base = res["plain"]["ms_median"]
    for name in ("cond_empty", "cond_half"):
        res[name]["per_step_extra_us"] = round((res[name]["ms_median"] - base) * 1e3 / T, 3)
    res["restyle_half"]["share_of_plain"] = round(res["restyle_half"]["ms_median"] / base, 4)
    out = {"B": B, "T": T, "L": L, "Lt": LT, "precision": "bf16", "reps": a.reps, "timing": "host clock around one call ending in a device synchronise; variants interleaved",
           "extra_launches_per_step": 1, "extra_launches_per_call": 2, **res, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
