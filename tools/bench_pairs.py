#!/usr/bin/env python3
"""Pairwise-metrics benchmark: what one precision / recall / density / coverage + KID evaluation launches, at two set sizes
(n = 1024 and n = 16384 rows per set, D = 1280, seeded clipped normals pooled over S = 14, the generated set shifted by 0.05):

  knn              dhw_pairs_knn of the real set, k = 3
  cover_gen        dhw_pairs_cover, generated rows against the real set's balls (count, nearest, index)
  cover_real       dhw_pairs_cover, real rows against the generated set (nearest only)
  polysum_xx / _yy / _xy   the three cubic sums of KID (the within-set ones with skip_diag)

next to a torch float64 yardstick on the same GPU that lives in this tool only (the product calls no BLAS): `matmul` = x @ y.T,
and `matmul_topk` = the squared distances from that product and torch.topk of the k + 1 smallest per row.  Each entry's calls
alternate with the yardstick's; every call is timed under device events after warm-up calls; medians with min .. max.
*_tflops = 2 n^2 D / time.  `agree`: the largest relative difference between dhw_pairs_knn's radius and the yardstick's.

    python tools/bench_pairs.py [--out profiles/pairs.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, S, K, SEED = 1280, 14, 3, 2026
SIZES = {1024: (10, 50), 16384: (3, 10)}   # n -> (warm-up calls, timed calls)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs.json"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import ctypes as C

    import numpy as np
    import torch

    from dhg_amd import _lib

    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms, flop):
        m = float(np.median(ms))
        return {"ms": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "tflops": round(flop / (m * 1e-3) / 1e12, 3)}

    out = {"D": D, "S": S, "k": K, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n, (warm, reps) in SIZES.items():
        g = torch.Generator(device="cuda").manual_seed(SEED + n)
        sets = []
        for shift in (0.0, 0.05):   # pooled in chunks: the unpooled features of 16384 rows would be 1.2 GB
            rows = torch.empty((n, D), dtype=torch.float64, device="cuda")
            for lo in range(0, n, 1024):
                f = (torch.randn((min(1024, n - lo), S, D), generator=g, device="cuda") * 1.5 + 1.5).clamp_(0, 6) + shift
                _lib.check(lib.dhw_pairs_pool(f.data_ptr(), f.shape[0], S, D, rows[lo:].data_ptr(), stream))
            sets.append(rows)
        torch.cuda.synchronize()
        x, y = sets
        need = int(lib.dhw_pairs_workspace_bytes(n, n, D))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        r_real, r_gen = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
        count, idx = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        near, acc = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.float64, device="cuda")
        _lib.check(lib.dhw_pairs_knn(y.data_ptr(), n, D, K, r_gen.data_ptr(), ws.data_ptr(), need, stream))

        entries = {
            "knn": lambda: _lib.check(lib.dhw_pairs_knn(x.data_ptr(), n, D, K, r_real.data_ptr(), ws.data_ptr(), need, stream)),
            "cover_gen": lambda: _lib.check(lib.dhw_pairs_cover(y.data_ptr(), n, x.data_ptr(), n, D, r_real.data_ptr(), count.data_ptr(), near.data_ptr(),
                                                                idx.data_ptr(), ws.data_ptr(), need, stream)),
            "cover_real": lambda: _lib.check(lib.dhw_pairs_cover(x.data_ptr(), n, y.data_ptr(), n, D, None, None, near.data_ptr(), None, ws.data_ptr(),
                                                                 need, stream)),
            "polysum_xx": lambda: _lib.check(lib.dhw_pairs_polysum(x.data_ptr(), n, x.data_ptr(), n, D, 1, acc.data_ptr(), ws.data_ptr(), need, stream)),
            "polysum_yy": lambda: _lib.check(lib.dhw_pairs_polysum(y.data_ptr(), n, y.data_ptr(), n, D, 1, acc.data_ptr(), ws.data_ptr(), need, stream)),
            "polysum_xy": lambda: _lib.check(lib.dhw_pairs_polysum(x.data_ptr(), n, y.data_ptr(), n, D, 0, acc.data_ptr(), ws.data_ptr(), need, stream)),
        }
        yt = y.t().contiguous()
        xt = x.t().contiguous()
        sq = (x * x).sum(1)

        def matmul():
            return torch.matmul(x, yt)

        def matmul_topk():
            d = sq[:, None] + sq[None, :] - 2.0 * torch.matmul(x, xt)
            return d.topk(K + 1, dim=1, largest=False).values

        yard = {"matmul": matmul, "matmul_topk": matmul_topk}
        for _ in range(warm):
            for fn in list(entries.values()) + list(yard.values()):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in list(entries) + list(yard)}
        names = list(yard)
        for i in range(reps):
            for j, (name, fn) in enumerate(entries.items()):
                times[name].append(timed(fn))
                other = names[(i + j) % len(names)]
                times[other].append(timed(yard[other]))
        flop = 2.0 * n * n * D
        res = {name: stats(ms, flop) for name, ms in times.items()}
        res["all_six_ms"] = round(sum(res[name]["ms"] for name in entries), 4)
        # the yardstick's k + 1 smallest include the row itself (distance about 0): its k-th neighbour is entry k
        entries["knn"]()
        ref = matmul_topk()[:, K].clamp_min(0)
        torch.cuda.synchronize()
        res["agree_knn_radius_rel"] = float(((r_real - ref).abs() / ref).max())
        res["workspace_mb"] = round(need / 2 ** 20, 1)
        out["sizes"][str(n)] = res
        print(n, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
