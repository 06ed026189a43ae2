"""The loop: ``read_train_config`` (the keys of a reference experiment config) and ``fit`` (the reference's TrainingLoop)."""
from __future__ import annotations

import math
import os

import torch

from ..train import Adam, check_ema_decay, dist_state
from .data import ResidentData
from .net import TrainModel
from .step import GraphedTrainStep, check_cond_drop
from .state import load_train_state, read_train_state, save_train_state
from .evaluate import EvalStep


def _granted_cores() -> int:
    """The CPU share the cgroup grants this process (cpu.max), else the visible cores."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        return os.cpu_count() if quota == "max" else max(1, int(int(quota) / int(period)))
    except (OSError, ValueError):
        return os.cpu_count() or 1


def read_train_config(config_path) -> dict:
    """The keys of a reference experiment config the training loop uses (configs/best.yml; train.py:136-151).  Missing keys
    raise, as attribute access on the reference's config object does."""
    import yaml
    with open(config_path) as f:
        cfg = yaml.safe_load(f) or {}
    ta, ds, opt = cfg.get("training_args"), cfg.get("dataset_args"), (cfg.get("optimizer") or {}).get("params")
    for name, sec in (("training_args", ta), ("dataset_args", ds), ("optimizer.params", opt)):
        if not isinstance(sec, dict):
            raise KeyError(f"{config_path}: no `{name}` section")
    need = ("steps", "batch_size", "warmup_steps", "clip_grad", "dropout", "att_layers_num", "channels", "log_freq", "save_freq")
    missing = [k for k in need if k not in ta] + [f"dataset_args.{k}" for k in ("max_seq_len", "max_text_len") if k not in ds]
    if missing:
        raise KeyError(f"{config_path}: missing {', '.join(missing)}")
    ch = int(ta["channels"])
    return {"steps": int(ta["steps"]), "batch_size": int(ta["batch_size"]), "warmup": int(ta["warmup_steps"]),
            "clip_grad": None if ta["clip_grad"] is None else float(ta["clip_grad"]), "dropout": float(ta["dropout"]),
            "num_layers": int(ta["att_layers_num"]), "c1": ch, "c2": ch * 3 // 2, "c3": ch * 2, "log_freq": int(ta["log_freq"]),
            "save_freq": int(ta["save_freq"]), "L": int(ds["max_seq_len"]), "Lt": int(ds["max_text_len"]),
            "betas": tuple(float(b) for b in opt.get("betas", (0.9, 0.999))), "weight_decay": float(opt.get("weight_decay", 0.0)),
            "seed": int((cfg.get("experiment") or {}).get("seed", 0))}


def fit(config_path, data_path=None, out_dir="runs/exp", steps=None, init=None, seed=0, log=print, precision="fp32", resident=False, cond_drop=0.0,
        ema=None, save_state=False, resume=None, val_path=None, eval_freq=None):
    """The reference's ``TrainingLoop.train`` (train.py:84-134): updates until ``training_args.steps``, a log line every
    ``log_freq`` updates (mean losses since the last line), ``checkpoint_<n>.pth`` every ``save_freq``, ``model_final.pth`` at
    the end.  Cadence and numbering are the reference's own (train.py:111-126): after update number ``count`` it tests
    ``(count + 1) % freq`` and labels the line / file ``count + 1`` — so ``checkpoint_1000.pth`` holds 999 updates, and runs line
    up with the reference step for step.  One process per GPU under ``torch.distributed.run`` (LOCAL_RANK picks the device,
    gradients averaged by RCCL); rank 0 logs and saves.  ``training_args.batch_size`` is the PER-RANK batch (the reference is
    single-process, so its 96 is one GPU's batch): N ranks train on a global batch of N x batch_size — divide it in the config to
    keep the reference's global batch.  ``precision``: "fp32" (the reference's) or "bf16" (bf16-rounded GEMM operands, fp32
    accumulation and fp32 master weights / optimizer state).  ``resident``: upload the dataset of ``data_path`` once
    (``ResidentData``, with its "writer" key if it has one) and let every update draw and gather its batch on the device — no
    per-update host work beyond the draw index; every rank keeps the whole set and draws with its own index step * world + rank.
    ``cond_drop``: the probability with which a sample trains under ``null_condition`` instead of its prompt and writer
    (``GraphedTrainStep``), which gives the checkpoint the unconditional branch that guided sampling needs; 0.1 is customary.

    Three options, all off by default (a run without them issues the launches and writes the files it always did):
    ``ema`` = a decay in (0, 1), 0.9999 is customary: keep the exponential moving average of the weights inside the optimizer's pass
    (``Adam(ema_decay=...)``, warmed up by ``ema_decay_at``); rank 0 writes ``ema_<n>.pth`` beside every ``checkpoint_<n>.pth``, in
    the same form, and the bare ``ema_final.pth`` at the end — the weights to sample from (``infer.py --checkpoint-path``).
    ``save_state``: rank 0 also keeps ONE ``train_state.pth`` in ``out_dir`` (``save_train_state``), rewritten at every ``save_freq``
    test and at the end.  ``resume`` = such a file (implies ``save_state``): every rank loads it and the loop continues at update
    ``count + 1`` up to the same ``steps``, with a fresh log accumulator and clock; ``count >= steps`` just writes the final files.
    What continues exactly — up to the run-to-run noise of the fp32 atomics: a resident run, whose batch, noise levels, eps and
    masks are functions of (seed, update number); a one-rank host-fed run, whose host generators the file carries.  Further
    host-fed ranks do NOT: their batch generators are reseeded from (config seed, rank, count) and torch's global generator is left
    as the process has it.  ``val_path``: a validation set in the form ``make_batches`` writes, uploaded once; every
    ``eval_freq`` updates (default: the ``save_freq`` cadence) every rank evaluates it (``EvalStep``: fixed noise levels and noise)
    and rank 0 logs the mean over levels as ``Eval <n> | Loss: ... | Score: ... | Pen: ...``, and with ``ema`` a second line
    ``Eval <n> (ema) | ...`` for the averaged weights.
    Returns the trained ``TrainModel``."""
    import time
    from .. import spec
    from ..checkpoint import read_state_dict
    if resident and not data_path:
        raise ValueError("resident=True trains from a dataset on the device: it needs data_path")
    check_cond_drop(cond_drop)
    check_ema_decay(ema)
    if eval_freq is not None and (isinstance(eval_freq, bool) or not isinstance(eval_freq, int) or eval_freq < 1):
        raise ValueError(f"eval_freq = {eval_freq!r} must be a positive integer")
    if eval_freq is not None and not val_path:
        raise ValueError("eval_freq sets how often the validation set is evaluated: it needs val_path")
    if resume is not None and not os.path.isfile(resume):
        raise ValueError(f"resume: no training state at {resume}")
    save_state = bool(save_state) or resume is not None
    cfg = read_train_config(config_path)
    n_steps = steps if steps is not None else cfg["steps"]
    # the host side draws abar and assembles batches with small torch CPU ops: with one thread per VISIBLE core on a box whose
    # cgroup grants fewer, each of them takes milliseconds (31 vs 7 ms per update on the GPU box) — cap at the granted share
    threads = max(1, min(_granted_cores(), 16))
    if torch.get_num_threads() > threads:
        torch.set_num_threads(threads)
    dist = torch.distributed
    world, rank = 1, 0
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
        _, rank, world = dist_state()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, L, Lt = cfg["batch_size"], cfg["L"], cfg["Lt"]
    if L % 8:
        raise ValueError("dataset_args.max_seq_len must be a multiple of 8 (configs/best.yml:12)")
    sd = read_state_dict(init) if init else spec.synthetic_state_dict(cfg["num_layers"], cfg["c1"], cfg["c2"], cfg["c3"], seed=seed)
    model = TrainModel(sd, num_layers=cfg["num_layers"], device=dev, drop_rate=cfg["dropout"], seed=seed, precision=precision)
    opt = Adam(model.parameters(), betas=cfg["betas"], weight_decay=cfg["weight_decay"], max_norm=cfg["clip_grad"] or 0.0, ema_decay=ema)
    alpha_set = torch.cumprod(1 - (0.02 + torch.exp(torch.linspace(math.log(1e-5), math.log(0.4), 60))), dim=0)   # utils/nn.py:19-39
    gen = torch.Generator().manual_seed(cfg["seed"] * 1000 + rank)
    data = None
    if data_path:
        data = torch.load(data_path, map_location="cpu", weights_only=True)
        for k, shape in (("strokes", (L, 3)), ("text", (Lt,)), ("style", (14, 1280))):
            if k not in data or tuple(data[k].shape[1:]) != shape:
                raise ValueError(f"{data_path}: `{k}` must be [N, {', '.join(map(str, shape))}]")
    rd = ResidentData(data, dev) if resident else None
    step_fn = GraphedTrainStep(model, opt, B, L, Lt, d_model=2 * cfg["c1"], warmup=cfg["warmup"], seed=seed, data=rd, alpha_set=alpha_set if resident else None,
                               cond_drop=cond_drop)

    def next_batch():
        if data is not None:                      # a random batch, as `next(iter(shuffled loader))` gives (train.py:99)
            idx = torch.randint(0, data["strokes"].shape[0], (B,), generator=gen)
            return {k: data[k][idx] for k in ("strokes", "text", "style")}
        pen = (torch.rand(B, L, 1, generator=gen) < 0.1).float()
        return {"strokes": torch.cat([torch.randn(B, L, 2, generator=gen), pen], dim=-1),
                "text": torch.randint(1, 73, (B, Lt), generator=gen), "style": torch.randn(B, 14, 1280, generator=gen).abs()}

    eval_fn = aside = None
    if val_path:
        val = torch.load(val_path, map_location="cpu", weights_only=True)
        for k, shape in (("strokes", (L, 3)), ("text", (Lt,)), ("style", (14, 1280))):
            if k not in val or tuple(val[k].shape[1:]) != shape:
                raise ValueError(f"{val_path}: `{k}` must be [N, {', '.join(map(str, shape))}]")
        eval_fn = EvalStep(model, ResidentData({k: val[k] for k in ("strokes", "text", "style")}, dev), B, seed=seed)   # (no writer groups: a row's style is its own)
        aside = torch.empty_like(model.flat) if ema is not None else None

    def evaluate(label):
        """The Eval line(s) of update ``label``: the raw weights, then — flat aside, ema into flat, evaluate, flat back: three device
        copies, every address unchanged — the averaged ones."""
        rows = [("", eval_fn().mean(0).tolist())]
        if aside is not None:
            aside.copy_(model.flat)
            model.flat.copy_(opt.ema[0])
            rows.append((" (ema)", eval_fn().mean(0).tolist()))
            model.flat.copy_(aside)
        for tag, m in rows:     # (sums of squares and cross-entropies: a negative one is not a loss — DESIGN.md 36, what a second graph did to the loss triple)
            if any(v < 0.0 for v in m):
                raise RuntimeError(f"held-out loss of update {label}{tag} is not a loss: {m}")
        if rank == 0:
            for tag, m in rows:
                log(f"Eval {label}{tag} | Loss: {m[0]:.3f} | Score: {m[1]:.3f} | Pen: {m[2]:.3f}")

    cpu_sd = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}   # noqa: E731

    def write_state(count):
        save_train_state(os.path.join(out_dir, "train_state.pth"), model, opt, count, {"gen": gen.get_state(), "torch": torch.get_rng_state()})

    done = 0
    if resume is not None:
        state = read_train_state(resume)
        done = load_train_state(state, model, opt)
        if rank == 0 and state.get("host_rng") is not None:
            gen.set_state(state["host_rng"]["gen"])
            torch.set_rng_state(state["host_rng"]["torch"])
        elif rank > 0:
            gen.manual_seed((cfg["seed"] * 1000 + rank) * 1000003 + done)
        del state
    os.makedirs(out_dir, exist_ok=True)
    eval_every = eval_freq or cfg["save_freq"]
    acc, t0 = [], time.time()
    for count in range(done + 1, n_steps + 1):
        acc.append((step_fn(step=count) if resident else step_fn(next_batch(), alpha_set, count)).clone())
        if (count + 1) % cfg["log_freq"] == 0:      # (train.py:111: the reference's own off-by-one, reproduced)
            m = torch.stack(acc).mean(0).tolist()   # (one host sync per log line)
            acc = []
            if rank == 0:
                log(f"Step {count + 1} | Loss: {m[0]:.3f} | Score: {m[1]:.3f} | Pen: {m[2]:.3f} | Time: {time.time() - t0:.3f} sec")
        if eval_fn is not None and (count + 1) % eval_every == 0:
            evaluate(count + 1)
        if rank == 0 and (count + 1) % cfg["save_freq"] == 0:
            # save_checkpoint's form (checkpoint.py:244): {"meta", "state_dict"}; model_final.pth is the bare state_dict (train.py:131)
            torch.save({"meta": None, "state_dict": cpu_sd(model.state_dict())}, os.path.join(out_dir, f"checkpoint_{count + 1}.pth"))
            if ema is not None:
                torch.save({"meta": None, "state_dict": cpu_sd(model.ema_state_dict(opt))}, os.path.join(out_dir, f"ema_{count + 1}.pth"))
            if save_state:
                write_state(count)
    if rank == 0:
        torch.save(cpu_sd(model.state_dict()), os.path.join(out_dir, "model_final.pth"))
        if ema is not None:
            torch.save(cpu_sd(model.ema_state_dict(opt)), os.path.join(out_dir, "ema_final.pth"))
        if save_state:
            write_state(max(done, n_steps))
    if world > 1:
        dist.barrier()
    return model
