#!/usr/bin/env python3
"""What the second-order multistep solver costs next to DDIM over the same levels, at bench.py's shape (B = 64,
L = 488, Lt = 30, bf16, synthetic weights, T = 60).  Four calls and two kernels:

  ddim_10 / ddim_20      sample_ddim() at 10 and 20 levels, order 1: one denoiser call + one step_update launch per level, eager
  dpm_10 / dpm_20        the same levels at order 2: one denoiser call + one dpm_update launch per level, eager
  ddim_update, dpm_update_first, dpm_update_second
                         the update kernels alone (dhw_ddim_update; dhw_dpm_update with a first- and a second-order row):
                         device events around 200 launches, us per launch

The calls are timed in turn, round after round (so drift of the box hits all of them alike): wall time of one call that ends in
a device synchronise.  A round is `--reps` interleaved repetitions and gives one median per variant; the figure of a variant is
the median over `--rounds` rounds and its spread the largest minus the smallest round median.  The rule is DESIGN.md §28's:
order 2 passes at a level count if its median is not above order 1's by more than order 1's own spread over rounds.  No target
is set in advance.

    python tools/bench_solver.py [--reps 30] [--rounds 3] [--out profiles/solver.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, L, LT, SEED = 64, 60, 488, 30, 2025
LAUNCHES = 200


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions per variant and round (at least 10)")
    ap.add_argument("--rounds", type=int, default=3, help="rounds (at least 3)")
    ap.add_argument("--out", help="also write the JSON result to this file")
    a = ap.parse_args(argv)
    if a.reps < 10 or a.rounds < 3:
        ap.error("--reps must be at least 10 and --rounds at least 3")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dhg_amd
    from dhg_amd import _lib, spec

    if not torch.cuda.is_available():
        raise SystemExit("bench_solver.py needs the MI355X: there is nothing to time without it")
    inp = spec.synthetic_inputs(B, L, LT, seed=SEED, T=1)
    tx = torch.from_numpy(inp["text"]).cuda()
    sv = torch.from_numpy(inp["style"]).cuda()
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})

    variants = {}
    for s in (10, 20):
        variants[f"ddim_{s}"] = (s, lambda s=s: dhg_amd.sample_ddim(m, tx, sv, L=L, T=T, steps=s, seed=1))
        variants[f"dpm_{s}"] = (s, lambda s=s: dhg_amd.sample_ddim(m, tx, sv, L=L, T=T, steps=s, seed=1, order=2))
    outs = {}
    for name, (_, fn) in variants.items():   # first-call allocations, then two more warm calls
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs.values())
    assert not torch.equal(outs["ddim_10"], outs["dpm_10"])

    # the update kernels alone
    lib = _lib.lib()
    g = torch.Generator().manual_seed(SEED)
    x, e, h = (torch.randn((B, L, 2), generator=g).cuda() for _ in range(3))
    out = torch.empty((B, L, 2)).cuda()
    lv = dhg_amd.ddim_levels(T, 20)
    tab = (C.c_float * (9 * 20))()
    assert lib.dhw_dpm_coefs(T, (C.c_int32 * 20)(*lv), 20, 2, tab) == 0
    rows = np.array(tab, np.float32).reshape(20, 9)
    first, second = (C.c_float * 9)(*map(float, rows[0])), (C.c_float * 9)(*map(float, rows[10]))
    assert rows[0, 0] == 1.0 and rows[10, 0] == 2.0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    c = [float(v) for v in rows[10, 1:5]]
    kernels = {"ddim_update": lambda: lib.dhw_ddim_update(x.data_ptr(), e.data_ptr(), None, B, L, *c, out.data_ptr(), st),
               "dpm_update_first": lambda: lib.dhw_dpm_update(x.data_ptr(), e.data_ptr(), None, None, None, h.data_ptr(), B, L, first, out.data_ptr(), None, st),
               "dpm_update_second": lambda: lib.dhw_dpm_update(x.data_ptr(), e.data_ptr(), None, None, None, h.data_ptr(), B, L, second, out.data_ptr(), None, st)}
    for fn in kernels.values():
        for _ in range(10):
            assert fn() == 0
    torch.cuda.synchronize()

    def time_kernel(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(LAUNCHES):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / LAUNCHES

    per_round = {name: [] for name in list(variants) + list(kernels)}
    for _ in range(a.rounds):
        ts = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, (_, fn) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        for name, v in ts.items():
            per_round[name].append(float(np.median(v)))
        for name, fn in kernels.items():
            per_round[name].append(time_kernel(fn))

    res = {}
    for name, v in per_round.items():
        unit = "ms" if name in variants else "us"
        res[name] = {f"{unit}_median": round(float(np.median(v)), 4), f"{unit}_spread": round(float(max(v) - min(v)), 4), f"{unit}_rounds": [round(t, 4) for t in v]}
        if name in variants:
            res[name]["denoiser_calls"] = variants[name][0]
            res[name]["ms_per_call_of_denoiser"] = round(float(np.median(v)) / variants[name][0], 4)
    verdict = {}
    for s in (10, 20):
        one, two = res[f"ddim_{s}"], res[f"dpm_{s}"]
        verdict[f"order2_at_{s}"] = {"ms_above_order1": round(two["ms_median"] - one["ms_median"], 4), "order1_spread": one["ms_spread"],
                                     "passes": bool(two["ms_median"] <= one["ms_median"] + one["ms_spread"])}
    out_json = {"B": B, "T": T, "L": L, "Lt": LT, "precision": "bf16", "reps": a.reps, "rounds": a.rounds,
                "timing": "calls: host clock around one call ending in a device synchronise, variants interleaved, median per round, median and "
                          "spread (max - min) over rounds; kernels: device events around 200 launches per round, us per launch",
                "rule": "order 2 passes if its median is not above order 1's by more than order 1's own spread over rounds (DESIGN.md 28)",
                **res, **verdict, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out_json))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out_json, indent=1) + "\n")


if __name__ == "__main__":
    main()
