#!/usr/bin/env python3
"""Feature-moments benchmark: one dhw_moments_update at N = 4096, S = 14, D = 1280 (seeded clipped normals, zeroed state) next
to torch.matmul of the pooled float64 matrix with its transpose on the same GPU.  The matmul is a yardstick of this tool only:
the product calls no BLAS.

  update_ms        median of 100 timed calls after 20 warm-up calls, each under device events: pooling, column sums and Gram
  matmul_ms        the same for p.T @ p (f64 [1280,4096] x [4096,1280]), the calls alternating with the update's
  *_tflops         2 N D^2 / time: the full product's count for both (the update computes the upper triangle and mirrors it)
  ratio            update_ms / matmul_ms (above 1: the update is slower); the update also pools 14 positions and sums columns
  agree            the update's Gram matrix against the matmul's, largest |difference| / ((N + S + 4) 2^-53 sum |p_i| |p_j|)

    python tools/bench_moments.py [--out profiles/moments.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, D, WARM, REPS, SEED = 4096, 14, 1280, 20, 100, 2025


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import ctypes as C

    import numpy as np
    import torch

    from dhg_amd import _lib

    g = np.random.Generator(np.random.PCG64(SEED))
    feat = torch.from_numpy(np.clip(g.normal(1.5, 1.5, size=(N, S, D)), 0, 6).astype(np.float32)).cuda()
    lib = _lib.lib()
    need = int(lib.dhw_moments_workspace_bytes(N, S, D))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    state = torch.zeros(D + D * D, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pooled = feat.double().sum(1) / S
    pooled_t = pooled.t().contiguous()

    def update():
        _lib.check(lib.dhw_moments_update(feat.data_ptr(), N, S, D, state.data_ptr(), state[D:].data_ptr(), ws.data_ptr(), need, stream))

    def matmul():
        return torch.matmul(pooled_t, pooled)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(WARM):
        update()
        matmul()
    torch.cuda.synchronize()
    up, mm = [], []
    for _ in range(REPS):
        up.append(timed(update))
        mm.append(timed(matmul))

    state.zero_()
    update()
    ref = matmul()
    torch.cuda.synchronize()
    gram = state[D:].view(D, D)
    bound = (N + S + 4) * 2.0 ** -53 * torch.matmul(pooled_t.abs(), pooled.abs())
    agree = float(((gram - ref).abs() / bound).max())
    flop = 2.0 * N * D * D
    um, mmm = float(np.median(up)), float(np.median(mm))
    out = {"N": N, "S": S, "D": D, "warmup": WARM, "reps": REPS, "update_ms": round(um, 4), "update_ms_min": round(min(up), 4),
           "update_ms_max": round(max(up), 4), "update_tflops": round(flop / (um * 1e-3) / 1e12, 3), "matmul_ms": round(mmm, 4),
           "matmul_ms_min": round(min(mm), 4), "matmul_ms_max": round(max(mm), 4), "matmul_tflops": round(flop / (mmm * 1e-3) / 1e12, 3),
           "ratio_update_over_matmul": round(um / mmm, 3), "gram_symmetric_bits": bool(torch.equal(gram, gram.t())),
           "largest_difference_over_bound": agree, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
