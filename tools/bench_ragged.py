#!/usr/bin/env python3
"""Ragged-batch throughput: one fixed, seeded mix of 64 prompts (8..30 tokens, so L = 16 n + 8 runs from 136 to 488), T = 60,
bf16, synthetic weights.  Three ways to sample it:

  (a) ragged:   ONE sample(..., lengths=) call;
  (b) padded:   the same batch as one uniform call at max(L) (an upper bound on the time only: its samples differ);
  (c) per-length: one uniform sample call per distinct length, run in sequence (correct samples, small batches).

For each: the median wall time of a whole call (ms) and the valid stroke points per second (sum of the prompts' own L / time).

    python tools/bench_ragged.py [--reps 5] [--out profiles/ragged_mix.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, SEED = 64, 60, 2024


def mix():
    """(token counts, stroke lengths) of the benchmark batch: 64 prompts, 8..30 tokens, L = stroke_length(n)."""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(SEED))
    tokens = [int(n) for n in rng.integers(8, 31, size=B)]
    return tokens, [16 * n + 8 for n in tokens]   # == tokenizer.stroke_length(n)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON result to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dhg_amd
    from dhg_amd import spec

    tokens, lens = mix()
    assert lens == [dhg_amd.stroke_length(n) for n in tokens]
    Lmax, Lt = max(lens), max(tokens)
    inp = spec.synthetic_inputs(B, Lmax, Lt, seed=SEED, T=1)
    for b, n in enumerate(tokens):
        inp["text"][b, n:] = 0
    tx = torch.from_numpy(inp["text"]).cuda()
    sv = torch.from_numpy(inp["style"]).cuda()
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=Lmax, max_Lt=Lt).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    groups = {}
    for b, n in enumerate(lens):
        groups.setdefault(n, []).append(b)
    group_inputs = [(n, tx[idx][:, :(n - 8) // 16].contiguous(), sv[idx].contiguous(), idx[0]) for n, idx in sorted(groups.items())]

    def run_a():
        return dhg_amd.sample(m, tx, sv, T=T, seed=1, lengths=lens)

    def run_b():
        return dhg_amd.sample(m, tx, sv, L=Lmax, T=T, seed=1)

    def run_c():
        return [dhg_amd.sample(m, t, s, L=n, T=T, seed=1, first_sample=f) for n, t, s, f in group_inputs]

    res = {}
    for name, fn in (("a_ragged", run_a), ("b_padded_uniform", run_b), ("c_per_length", run_c)):
        fn()   # graph capture(s)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(ts))
        res[name] = {"ms": round(ms, 3), "ms_all": [round(t, 3) for t in ts], "valid_points_per_s": round(sum(lens) / (ms * 1e-3), 1)}
    out = {"B": B, "T": T, "precision": "bf16", "tokens_min": min(tokens), "tokens_max": max(tokens), "L_min": min(lens), "L_max": Lmax,
           "distinct_lengths": len(groups), "valid_points": sum(lens), "padded_points": B * Lmax, "reps": a.reps, **res,
           "a_over_b": round(res["a_ragged"]["ms"] / res["b_padded_uniform"]["ms"], 4),
           "a_over_c": round(res["a_ragged"]["ms"] / res["c_per_length"]["ms"], 4),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
