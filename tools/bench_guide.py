#!/usr/bin/env python3
"""What classifier-free guidance costs next to unguided deterministic sampling, at bench.py's shape (B = 64, L = 488,
Lt = 30, bf16, synthetic weights, T = 60), 20 levels each.  Three calls on one handle of 128 rows:

  ddim_20         sample_ddim() of 64 prompts: 20 forwards of 64 rows
  guided_20       sample_ddim(guidance=2.5) of 64 prompts: 20 forwards of 128 rows (64 real + 64 null conditions)
  ddim_20_B128    sample_ddim() of 128 prompts: 20 forwards of 128 rows — what the doubled batch alone costs

All launch eagerly.  The variants are timed in turn, round after round (so drift of the box hits all of them alike): wall time
of one call that ends in a device synchronise; median and quartiles over the rounds.  guided / unguided is reported as measured;
no target is set.  The step kernels alone (dhw_guide_update's three kinds, dhw_ddim_update for comparison) are timed with
device events around a run of back-to-back launches on arrays of the same shape.

    python tools/bench_guide.py [--reps 30] [--out profiles/guide.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, T, L, LT, SEED, STEPS, SCALE = 64, 60, 488, 30, 2025, 20, 2.5
KERNEL_LAUNCHES = 200


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
    from dhg_amd import _lib, spec

    if not torch.cuda.is_available():
        raise SystemExit("bench_guide.py needs the MI355X: there is nothing to time without it")
    inp = spec.synthetic_inputs(2 * B, L, LT, seed=SEED, T=1)
    tx2 = torch.from_numpy(inp["text"]).cuda()
    sv2 = torch.from_numpy(inp["style"]).cuda()
    tx, sv = tx2[:B].contiguous(), sv2[:B].contiguous()
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=2 * B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})

    kw = dict(L=L, T=T, steps=STEPS, seed=1)
    variants = {"ddim_20": (B, lambda: dhg_amd.sample_ddim(m, tx, sv, **kw)),
                "guided_20": (2 * B, lambda: dhg_amd.sample_ddim(m, tx, sv, guidance=SCALE, **kw)),
                "ddim_20_B128": (2 * B, lambda: dhg_amd.sample_ddim(m, tx2, sv2, **kw))}
    outs = {}
    for name, (_, fn) in variants.items():   # first-call allocations, then two more warm calls
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs.values())
    # does a row depend on its batch at this shape?  Recorded, not asserted: it is a property of the forward, not of the guidance
    g1 = dhg_amd.sample_ddim(m, tx, sv, guidance=1.0, **kw)
    same = {"rows_0_63_of_B128_equal_B64_bitwise": bool(torch.equal(outs["ddim_20"], outs["ddim_20_B128"][:B])),
            "rows_0_63_of_B128_vs_B64_max_abs": float((outs["ddim_20"] - outs["ddim_20_B128"][:B]).abs().max()),
            "guided_scale_1_equal_B64_as_values": bool((g1 == outs["ddim_20"]).all()),
            "guided_scale_1_vs_B64_max_abs": float((g1 - outs["ddim_20"]).abs().max()),
            "abs_max_of_the_lines": float(outs["ddim_20"].abs().max())}
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
        rows = variants[name][0]
        res[name] = {"forward_rows": rows, "ms_median": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                     "ms_p25": round(float(np.percentile(v, 25)), 4), "ms_p75": round(float(np.percentile(v, 75)), 4),
                     "ms_per_step": round(float(np.median(v)) / STEPS, 4)}
    ratios = np.asarray(ts["guided_20"]) / np.asarray(ts["ddim_20"])
    res["guided_over_unguided"] = {"median_of_round_ratios": round(float(np.median(ratios)), 4), "p25": round(float(np.percentile(ratios, 25)), 4),
                                   "p75": round(float(np.percentile(ratios, 75)), 4), "ratio_of_medians": round(res["guided_20"]["ms_median"] / res["ddim_20"]["ms_median"], 4)}
    res["guided_over_B128"] = round(res["guided_20"]["ms_median"] / res["ddim_20_B128"]["ms_median"], 4)

    # the step kernels alone, device events around KERNEL_LAUNCHES back-to-back launches
    lib = _lib.lib()
    g = torch.Generator().manual_seed(SEED)
    x2 = torch.randn((2 * B, L, 2), generator=g).cuda()
    e2 = torch.randn((2 * B, L, 2), generator=g).cuda()
    z = torch.randn((B, L, 2), generator=g).cuda()
    out2 = torch.empty((2 * B, L, 2)).cuda()
    sc = torch.full((B,), SCALE).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kernels = {"ddim_update": lambda: lib.dhw_ddim_update(x2.data_ptr(), e2.data_ptr(), None, B, L, 0.9, 0.4, 0.95, 0.3, out2.data_ptr(), st)}
    for kind, name in ((0, "guide_update_ddim"), (1, "guide_update_new"), (2, "guide_update_standard")):
        kernels[name] = lambda kind=kind: lib.dhw_guide_update(kind, x2.data_ptr(), e2.data_ptr(), None, None, sc.data_ptr(), z.data_ptr() if kind else None, B, L,
                                                               0.9, 0.4, 0.95, 0.3, out2.data_ptr(), None, st)
    kt = {name: [] for name in kernels}
    for name, fn in kernels.items():
        for _ in range(10):
            assert fn() == 0, lib.dhw_last_error(None)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, fn in kernels.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(KERNEL_LAUNCHES):
                fn()
            ev1.record()
            ev1.synchronize()
            kt[name].append(ev0.elapsed_time(ev1) * 1e3 / KERNEL_LAUNCHES)
    res["step_kernels_us_per_launch"] = {name: {"median": round(float(np.median(v)), 3), "p25": round(float(np.percentile(v, 25)), 3),
                                                "p75": round(float(np.percentile(v, 75)), 3)} for name, v in kt.items()}
    out = {"B": B, "T": T, "L": L, "Lt": LT, "levels": STEPS, "scale": SCALE, "precision": "bf16", "reps": a.reps,
           "timing": "host clock around one call ending in a device synchronise, variants interleaved, all eager; step kernels: device events around "
                     f"{KERNEL_LAUNCHES} back-to-back launches (launch-rate bound: an upper bound on the kernel's own time)",
           **res, "batch_independence": same, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
