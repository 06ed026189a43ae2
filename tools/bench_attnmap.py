#!/usr/bin/env python3
"""What an attention-map call costs next to the plain denoiser call, at bench.py's shape (B = 64, L = 488, Lt = 30, bf16,
synthetic weights, layer = the last attention layer).  Two calls on the same inputs:

  forward    model(strokes, text, sigma, style): dhw_forward
  attention  attention(model, ..., heads=True): dhw_attention = that forward + one GEMM launch (Q) + the map kernel,
             writing probs, mean and token

The two are timed in turn, round after round (so drift of the box hits both alike): wall time of one call that ends in a
device synchronise; median and quartiles over the rounds, and the difference of the medians.  No target is set.

    python tools/bench_attnmap.py [--reps 30] [--out profiles/attnmap.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, L, LT, SEED = 64, 488, 30, 2025


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
        raise SystemExit("bench_attnmap.py needs the MI355X: there is nothing to time without it")
    inp = spec.synthetic_inputs(B, L, LT, seed=SEED, T=1)
    tx, sv, st = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "strokes"))
    sg = torch.full((B,), 0.5, device="cuda")
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    variants = {
        "forward": lambda: m(st, tx, sg, sv),
        "attention": lambda: dhg_amd.attention(m, st, tx, sg, sv, layer=-1, heads=True),
    }
    outs = {}
    for name, fn in variants.items():
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
    probs = outs["attention"][2]
    assert tuple(probs.shape) == (B, 6, L // 8, LT) and torch.isfinite(probs).all()
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
    out = {"B": B, "L": L, "Lt": LT, "precision": "bf16", "layer": "att_layers.1", "reps": a.reps,
           "timing": "host clock around one call ending in a device synchronise; variants interleaved; both launch eagerly",
           **res, "attention_minus_forward_ms": round(res["attention"]["ms_median"] - res["forward"]["ms_median"], 4),
           "the_difference_is": "one GEMM launch (Q = Wq(x + PE), [B*61, 384] x [384, 384]) + the map kernel (256 workgroups of 384 threads) + three output allocations on the host side",
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
