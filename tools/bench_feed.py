#!/usr/bin/env python3
"""What feeding the training step costs: fit()'s loop body — next_batch + step — timed with the batch built on the host (a
torch.randint, three fancy-index gathers, get_alphas, one pinned block and one H2D copy per update) and with the dataset
resident on the GPU (train_model.ResidentData: the replayed graph draws and gathers the batch itself), in ONE process, the two
feeds alternating, several repeats each.  Beside them the fixed-batch figure of tools/bench_train.py (the same host batch every
update: no gather, the copy still made) — the floor neither feed can beat.
  python tools/bench_feed.py [--batches 32 96] [--updates 200] [--warmup 20] [--repeats 5] [--samples 4096]
Synthetic dataset of --samples lines at L = 480, Lt = 50, S = 14 (configs/best.yml dataset_args), random-init weights, fp32.
Prints one JSON line per batch size: median and (min, max) of ms per update over the repeats, for each feed."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dhg_amd  # noqa: E402
from dhg_amd import spec, train, train_model as tm  # noqa: E402


def dataset(N, L, Lt, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, spec.VOCAB, (N, Lt), generator=g)
    text[torch.arange(Lt)[None, :] >= torch.randint(5, Lt, (N, 1), generator=g)] = 0          # zero padding behind a random length
    return {"strokes": torch.cat([torch.randn(N, L, 2, generator=g), (torch.rand(N, L, 1, generator=g) < 0.1).float()], dim=-1),
            "text": text, "style": torch.randn(N, S, 1280, generator=g).abs(), "writer": torch.arange(N) // 8}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 96])
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--L", type=int, default=480)
    ap.add_argument("--Lt", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feed needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    data = dataset(a.samples, a.L, a.Lt, 14)
    rd = tm.ResidentData(data, dev)
    alpha_set = dhg_amd.get_alpha_set(60).float()
    sd = spec.synthetic_state_dict(2, 128, 192, 256, seed=0)
    for B in a.batches:
        def new_step(**kw):
            model = tm.TrainModel(sd, num_layers=2, device=dev)
            return tm.GraphedTrainStep(model, train.Adam(model.parameters()), B, a.L, a.Lt, **kw)
        host, fixed, res = new_step(), new_step(), new_step(data=rd, alpha_set=alpha_set)
        gen = torch.Generator().manual_seed(1)
        one = {k: data[k][:B] for k in ("strokes", "text", "style")}
        count = {"host": 0, "fixed": 0, "resident": 0}

        def update(mode):           # fit()'s loop body
            count[mode] += 1
            if mode == "host":
                idx = torch.randint(0, a.samples, (B,), generator=gen)
                return host({k: data[k][idx] for k in ("strokes", "text", "style")}, alpha_set, count[mode]).clone()
            if mode == "fixed":
                return fixed(one, alpha_set, count[mode]).clone()
            return res(step=count[mode]).clone()

        def timed(mode, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = update(mode)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3, out
        ms = {m: [] for m in count}
        for m in count:
            timed(m, a.warmup)
        for _ in range(a.repeats):
            for m in ("host", "resident", "fixed"):     # alternating: a drift of the box hits every feed alike
                t, out = timed(m, a.updates)
                if not bool(torch.isfinite(out).all()):
                    raise SystemExit(f"{m}: the loss is not finite")
                ms[m].append(t)
        r = {"metric": "fit() loop body, ms per update", "batch": B, "L": a.L, "Lt": a.Lt, "samples": a.samples, "updates": a.updates, "repeats": a.repeats,
             "dtype": "f32", "resident_bytes": rd.nbytes}
        for m, v in ms.items():
            r[m] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        r["host_minus_resident_ms"] = round(r["host"]["median"] - r["resident"]["median"], 3)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
