#!/usr/bin/env python3
"""Sample quality of a checkpoint: the Fréchet distance between the lines of a data set and lines the model samples for the same
rows, in the StyleExtractor's feature space (dhg_amd.sample_quality).

    python tools/eval_samples.py --data val.pt --experiment-path runs/exp1 --weights mobilenet_v2.pth \\
        [--n 1024] [--guidance 2.5] [--steps 20 [--order 1 2]] [--mode new] [--real-stats real.npz] [--save-real-stats real.npz] [--metrics [--k 3]] [--dtw]

--data is the file train.py --val reads: {"strokes" [N,L,3], "text" [N,Lt], "style" [N,14,1280]}.  Several values of --guidance,
--steps or --order (sample_ddim's solver order) give one line per combination; the real statistics are computed once (or read from --real-stats).  One line per run:

    FD <value> | n <count> | sampler <sample|ddim> | T .. | steps .. | guidance .. | mode .. | seconds: sample .. features .. moments .. eig ..

--metrics: a second line per run, from dhg_amd.sample_metrics (at most 16384 lines, not with --real-stats):

    PR precision .. | recall .. | density .. | coverage .. | KID .. | k ..

--dtw: one more line per run, the stroke-space distances of dhg_amd.sample_metrics(dtw=True) (not with --real-stats):

    DTW paired .. | nearest .. | self ..

--synthetic: the model holds spec.synthetic_state_dict(2) instead of a checkpoint (with --synthetic-rows R, --data is first
written with R synthetic rows); without --weights the extractor is random-initialised.  Such distances only exercise the path.
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_rows(rows, L, Lt, seed=0):
    """{"strokes", "text", "style"} of `rows` synthetic lines: rightward strokes on a wavy baseline with a lift every 9 to 15 rows."""
    import numpy as np
    import torch

    from dhg_amd import spec
    g = np.random.Generator(np.random.PCG64(seed))
    strokes = np.zeros((rows, L, 3), np.float32)
    for b in range(rows):
        t = np.arange(L) * g.uniform(0.4, 1.1)
        strokes[b, :, 0] = g.uniform(0.2, 1.2, L)
        strokes[b, :, 1] = g.uniform(0.5, 1.5) * np.cos(t + g.uniform(0, 6)) + g.normal(0, 0.3, L)
        i = 0
        while i < L:
            i += int(g.integers(9, 16))
            strokes[b, min(i, L) - 1, 2] = 1
    inp = spec.synthetic_inputs(rows, 8, Lt, seed=seed + 1, T=1)
    return {"strokes": torch.from_numpy(strokes), "text": torch.from_numpy(inp["text"]), "style": torch.from_numpy(inp["style"])}


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True)
    ap.add_argument("--experiment-path")
    ap.add_argument("--config-path")
    ap.add_argument("--checkpoint-path")
    ap.add_argument("--weights", help="torchvision's mobilenet_v2 state_dict for the StyleExtractor")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--n", type=int)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--T", type=int, default=60)
    ap.add_argument("--guidance", type=float, nargs="*", default=[None])
    ap.add_argument("--steps", type=int, nargs="*", default=[None])
    ap.add_argument("--order", type=int, nargs="*", default=[None], choices=(1, 2), help="solver order of sample_ddim (needs --steps): one setting per value")
    ap.add_argument("--mode", default=None, choices=("new", "standard"))
    ap.add_argument("--real-stats")
    ap.add_argument("--save-real-stats")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--synthetic-rows", type=int)
    ap.add_argument("--synthetic-L", type=int, default=256)
    ap.add_argument("--synthetic-Lt", type=int, default=32)
    ap.add_argument("--json", help="also write the runs to this file")
    ap.add_argument("--metrics", action="store_true", help="also print precision / recall / density / coverage and KID (a PR line per setting)")
    ap.add_argument("--k", type=int, default=3, help="neighbours of the k-NN balls of --metrics (1 to 8)")
    ap.add_argument("--dtw", action="store_true", help="also print the stroke-space DTW distances (a DTW line per setting)")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.mode is not None and any(s is not None for s in a.steps):
        ap.error("--mode belongs to the ancestral sampler: it cannot be combined with --steps")
    if any(o is not None for o in a.order) and any(s is None for s in a.steps):
        ap.error("--order belongs to deterministic sampling: it needs --steps")
    if a.synthetic_rows is not None and not a.synthetic:
        ap.error("--synthetic-rows needs --synthetic")
    if (a.metrics or a.dtw) and a.real_stats:
        ap.error("--metrics and --dtw need the real lines themselves: they cannot be combined with --real-stats")
    if not 1 <= a.k <= 8:
        ap.error("--k must be in [1, 8]")
    sys.path.insert(0, ROOT)
    import torch

    import dhg_amd
    from dhg_amd import spec
    from dhg_amd.inference import _resolve_experiment

    if a.synthetic_rows is not None:
        torch.save(synthetic_rows(a.synthetic_rows, a.synthetic_L, a.synthetic_Lt), a.data)
    data = torch.load(a.data, map_location="cpu", weights_only=True)
    cap = dict(max_B=2 * a.batch if any(g is not None for g in a.guidance) else a.batch, max_L=int(data["strokes"].shape[1]),
               max_Lt=int(data["text"].shape[1]), style_rows=int(data["style"].shape[1]))
    if a.synthetic:
        model = dhg_amd.DiffusionModel(2, precision=a.precision, **cap).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}, strict=True)
    else:
        config, ckpt = _resolve_experiment(a.config_path, a.checkpoint_path, a.experiment_path)
        model = dhg_amd.load_model(config, ckpt, precision=a.precision, **cap)
    with warnings.catch_warnings():
        if a.synthetic:
            warnings.simplefilter("ignore")   # the random initialisation is what --synthetic asks for
        extractor = dhg_amd.StyleExtractor(a.weights)
    real = dhg_amd.FeatureStats.load(a.real_stats) if a.real_stats else None
    real_pair = None   # --metrics: (statistics, rows) of the real lines, computed by the first run
    runs = []
    for steps, order, guidance in ((s, o, g) for s in a.steps for o in a.order for g in a.guidance):
        kw = {"T": a.T}
        if steps is not None:
            kw["steps"] = steps
        elif a.mode is not None:
            kw["diffusion_mode"] = a.mode
        if order is not None:
            kw["order"] = order
        if guidance is not None:
            kw["guidance"] = guidance
        sec = {}
        if a.metrics or a.dtw:
            if a.dtw:
                kw["dtw"] = True
            m = dhg_amd.sample_metrics(model, data, extractor, n=a.n, batch=a.batch, seed=a.seed, k=a.k, real=real_pair, timings=sec, **kw)
            fd, real, gen, real_pair = m["fd"], m["real_stats"], m["gen_stats"], (m["real_stats"], m["real_set"])
        else:
            fd, real, gen = dhg_amd.sample_quality(model, data, extractor, n=a.n, batch=a.batch, seed=a.seed, real=real, timings=sec, **kw)
        run = {"fd": fd, "n": gen.count, "n_real": real.count, "sampler": "ddim" if steps is not None else "sample", "T": a.T, "steps": steps,
               "guidance": guidance, "mode": None if steps is not None else (a.mode or "new"), "seconds": {k: round(v, 4) for k, v in sec.items()}}
        if order is not None:
            run["order"] = order
        runs.append(run)
        print(f"FD {fd:.6g} | n {gen.count} | sampler {run['sampler']} | T {a.T} | steps {steps}{'' if order is None else f' | order {order}'} | guidance {guidance} | mode {run['mode']} | "
              "seconds: " + " ".join(f"{k} {v:.3f}" for k, v in sec.items()), flush=True)
        if a.metrics:
            run.update({name: m[name] for name in ("precision", "recall", "density", "coverage", "kid", "k")})
            print(f"PR precision {m['precision']:.4f} | recall {m['recall']:.4f} | density {m['density']:.4f} | coverage {m['coverage']:.4f} | "
                  f"KID {m['kid']:.6g} | k {m['k']}", flush=True)
        if a.dtw:
            run.update({name: m[name] for name in ("dtw_paired", "dtw_nearest", "dtw_self")})
            print(f"DTW paired {m['dtw_paired']:.6g} | nearest {m['dtw_nearest']:.6g} | self {m['dtw_self']:.6g}", flush=True)
    if a.save_real_stats:
        real.save(a.save_real_stats)
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps({"data": os.path.basename(a.data), "synthetic": a.synthetic, "batch": a.batch, "device": torch.cuda.get_device_name(0),
                                "runs": runs}, indent=1) + "\n")


if __name__ == "__main__":
    main()
