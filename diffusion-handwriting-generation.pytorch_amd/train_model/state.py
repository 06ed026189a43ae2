"""The full training state in one file: ``save_train_state`` / ``load_train_state`` (weights, Adam's moments and counter, the EMA),
so that a stopped run continues where it was instead of restarting with zero moments at a warm-up learning rate."""
from __future__ import annotations

import os

import torch

FORMAT = 1


def _optim(opt) -> dict:
    return {"betas": [float(b) for b in opt.betas], "eps": float(opt.eps), "weight_decay": float(opt.weight_decay), "max_norm": float(opt.max_norm)}


def _layout(model) -> list:
    return [(str(k), int(model.sizes[k])) for k in model.layout]


def _one(bufs, what):
    if len(bufs) != 1:
        raise ValueError(f"the training state holds ONE flat buffer per quantity; this optimizer has {len(bufs)} for {what}")
    return bufs[0]


def save_train_state(path, model, opt, count: int, host_rng=None):
    """Everything an interrupted run needs to continue after update number ``count``, as one dict that
    ``torch.load(weights_only=True)`` reads: format, count, step_count (Adam's update counter, which also places the run on the Noam
    schedule and the EMA warm-up), flat / m / v / ema (or None) in flat-buffer order on the CPU, ema_decay, layout [(name, numel)],
    optim {betas, eps, weight_decay, max_norm}, precision, host_rng (None, or what the caller's host-side generators hold: ``fit``
    stores rank 0's batch generator and torch's global CPU generator, which ``get_alphas`` draws from).  Written to ``path + ".tmp"``
    and moved into place, so a run killed while saving leaves the previous file whole.  One host synchronisation (the copies)."""
    if isinstance(count, bool) or not isinstance(count, int) or count < 0:
        raise ValueError(f"count = {count!r} must be the number of updates done, an integer >= 0")
    cpu = lambda t: t.detach().to("cpu", copy=True)   # noqa: E731
    state = {"format": FORMAT, "count": count, "step_count": int(opt.step_count), "flat": cpu(model.flat), "m": cpu(_one(opt.m, "m")),
             "v": cpu(_one(opt.v, "v")), "ema": None if opt.ema is None else cpu(_one(opt.ema, "ema")), "ema_decay": opt.ema_decay,
             "layout": _layout(model), "optim": _optim(opt), "precision": model.precision, "host_rng": host_rng}
    path = os.fspath(path)
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def read_train_state(path) -> dict:
    """The dict ``save_train_state`` wrote (``weights_only=True``: tensors and plain containers only), its format checked."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or state.get("format") != FORMAT:
        raise ValueError(f"{path}: `format` is {state.get('format') if isinstance(state, dict) else type(state).__name__!r}, this build reads format {FORMAT}")
    return state


def load_train_state(path, model, opt) -> int:
    """Put a saved state back INTO the buffers ``model`` and ``opt`` already have (``copy_``: a captured graph holds their addresses)
    and return ``count``, the updates done.  ``path``: the file, or the dict ``read_train_state`` gave for it.  Nothing is written
    unless everything matches: a ValueError names the key when format, layout, optim, precision or the presence / decay of the EMA
    differ from this model and optimizer, or when count / step_count are not integers >= 0."""
    state = path if isinstance(path, dict) else read_train_state(path)
    if state.get("format") != FORMAT:
        raise ValueError(f"`format` is {state.get('format')!r}, this build reads format {FORMAT}")
    want = {"layout": _layout(model), "optim": _optim(opt), "precision": model.precision}
    got = dict(state)
    got["layout"] = [(str(k), int(n)) for k, n in state.get("layout") or []]
    if isinstance(got.get("optim"), dict) and "betas" in got["optim"]:
        got["optim"] = dict(got["optim"], betas=[float(b) for b in got["optim"]["betas"]])
    for key in ("layout", "optim", "precision"):
        if got.get(key) != want[key]:
            raise ValueError(f"`{key}` of the saved state differs from this run's: saved {_brief(got.get(key))}, here {_brief(want[key])}")
    if (state.get("ema") is None) != (opt.ema is None):
        raise ValueError(f"`ema`: the saved state {'has none' if state.get('ema') is None else 'has one'}, this optimizer {'keeps none' if opt.ema is None else 'keeps one'}")
    if state.get("ema_decay") != opt.ema_decay:
        raise ValueError(f"`ema_decay` of the saved state is {state.get('ema_decay')!r}, this optimizer's {opt.ema_decay!r}")
    for key in ("count", "step_count"):
        c = state.get(key)
        if isinstance(c, bool) or not isinstance(c, int) or c < 0:
            raise ValueError(f"`{key}` = {c!r} must be an integer >= 0")
    pairs = [("flat", model.flat), ("m", _one(opt.m, "m")), ("v", _one(opt.v, "v"))] + ([("ema", _one(opt.ema, "ema"))] if opt.ema is not None else [])
    for key, dst in pairs:
        src = state.get(key)
        if not isinstance(src, torch.Tensor) or src.dtype != torch.float32 or tuple(src.shape) != tuple(dst.shape):
            raise ValueError(f"`{key}` must be a float32 tensor {tuple(dst.shape)}")
    for key, dst in pairs:
        dst.copy_(state[key])
    opt.step_count = state["step_count"]
    return state["count"]


def _brief(v, limit: int = 120) -> str:
    s = repr(v)
    return s if len(s) <= limit else s[:limit] + "..."
