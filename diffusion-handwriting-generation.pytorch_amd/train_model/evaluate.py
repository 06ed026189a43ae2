"""Held-out loss on the device: ``EvalStep`` — forward passes over a resident validation set at fixed noise levels and noise."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..train import _stream, _tcheck
from .data import ResidentData
from .net import TrainModel


class EvalStep:
    """The training loss of ``model`` on a validation set, at fixed noise levels with fixed noise, so that two evaluations of one
    run — or of its raw and its averaged weights — are comparable: calling it returns the device tensor [K, 3] of (loss, score loss,
    pen loss) per level, the mean over the first ``(N // B) * B`` rows of ``data`` taken batch by batch (the caller's first read of it
    is the one host synchronisation).

    Per (batch i, level k) the host sends one small block from pinned memory — idx = style_src = i B .. i B + B - 1, alphas =
    abar[levels[k]] and its square root, rng = (seed, i K + k) — and issues dhw_train_batch_gather, dhw_train_draw (for eps),
    dhw_train_perturb, the model's forward and dhw_train_loss without gradients; out3 is added into row k of the accumulator.  The
    blocks are filled once, here: they never change.  The forward runs in eval mode: ``model.drop_rate`` and ``model.style_drop`` are 0
    for the duration of the call (both restored) and the style keep-mask is ones.  ``levels``: schedule indices as ``score`` takes them
    (default ``default_levels(T)``: 7, 22, 37, 52 at T = 60).  It evaluates whatever weights ``model.flat`` holds at the call.

    The launches are issued from the host, not replayed from a graph of their own (with a second captured graph alive
    beside the training step's, the loss triple of whichever graph had been captured first came back as a repeated byte pattern in
    4 of 10 runs on MI355X; the cause was not found, and an evaluation is a few dozen forward passes per ``save_freq`` updates)."""

    def __init__(self, model: TrainModel, data: ResidentData, B: int, levels=None, T: int = 60, seed: int = 0):
        from ..inference import _check_int, _check_levels, get_alpha_set
        self.levels = _check_levels(levels, T)
        _check_int("B", B, 1)
        _check_int("seed", seed, 0)
        if data.N < B:
            raise ValueError(f"the validation set holds {data.N} rows, fewer than one batch of B = {B}")
        if data.L < 8 or data.L % 8:
            raise ValueError(f"the stroke length must be a positive multiple of 8, got {data.L}")
        # ---- the model and the device, from here on
        if data.max_token >= model.p["text_style_model.emb.weight"].d.shape[0]:
            raise ValueError("token id out of the embedding's range")
        index = lambda d: torch.cuda.current_device() if torch.device(d).index is None else torch.device(d).index   # noqa: E731
        if index(data.dev) != index(model.dev):
            raise ValueError(f"the validation data lives on {data.dev}, the model on {model.dev}")
        dev = model.dev
        self.model, self.data, self.B, self.seed = model, data, B, seed
        self.batches = data.N // B
        K, L, Lt, S = len(self.levels), data.L, data.Lt, data.S
        abar = get_alpha_set(T).numpy().astype(np.float32)
        fields = [("rng", (2,), torch.int64), ("idx", (B,), torch.int32), ("style_src", (B,), torch.int32), ("alphas", (B,), torch.float32),
                  ("sigma", (B, 1), torch.float32)]
        offs, off = {}, 0
        for name, shape, dt in fields:
            n = int(np.prod(shape)) * (8 if dt == torch.int64 else 4)
            offs[name] = (off, n, shape, dt)
            off += (n + 15) // 16 * 16
        carve = lambda buf: {k: buf[o:o + n].view(dt).view(shape) for k, (o, n, shape, dt) in offs.items()}   # noqa: E731
        self._stage_dev = torch.zeros(off, dtype=torch.uint8, device=dev)
        self._stage_host = torch.zeros(self.batches * K, off, dtype=torch.uint8).pin_memory()
        for i in range(self.batches):
            for k, level in enumerate(self.levels):
                hv = carve(self._stage_host[i * K + k])
                hv["rng"][0], hv["rng"][1] = seed, i * K + k
                hv["idx"].copy_(torch.arange(i * B, i * B + B, dtype=torch.int32))
                hv["style_src"].copy_(hv["idx"])
                hv["alphas"].fill_(float(abar[level]))
                hv["sigma"].copy_(torch.from_numpy(np.sqrt(abar[level:level + 1])).expand(B, 1))
        self._dv = carve(self._stage_dev)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
        self.x, self.pen, self.eps = z(B, L, 2), z(B, L), z(B, L, 2)
        self.ids, self.mask, self.style = z(B, Lt, dt=torch.int64), z(B, Lt), z(B, S, 1280)
        self.keep = torch.ones(B, S, 1280, device=dev)       # eval mode: every style feature kept
        self._keep_drawn = z(B, S, 1280)                     # dhw_train_draw's second output, unused
        self.out, self.acc = z(3), z(K, 3)
        model.prepare_tables(L, Lt)

    def _body(self):
        m, dt, d = self.model, self.data, self._dv
        B, L = self.B, dt.L
        lib, st = _lib.lib(), _stream(m.dev)
        _tcheck(lib.dhw_train_batch_gather(dt.strokes.data_ptr(), dt.text.data_ptr(), dt.style.data_ptr(), d["idx"].data_ptr(), d["style_src"].data_ptr(),
                                           dt.N, B, L, dt.Lt, dt.S, self.x.data_ptr(), self.pen.data_ptr(), self.ids.data_ptr(), self.mask.data_ptr(),
                                           self.style.data_ptr(), st))
        _tcheck(lib.dhw_train_draw(d["rng"].data_ptr(), B, L, self.eps.data_ptr(), self._keep_drawn.numel(), self._keep_drawn.numel() // B, 0.0,
                                   self._keep_drawn.data_ptr(), st))
        x_pert = torch.empty_like(self.x)
        _tcheck(lib.dhw_train_perturb(self.x.data_ptr(), self.eps.data_ptr(), d["alphas"].data_ptr(), B, L, x_pert.data_ptr(), st))
        score, pen_pred = m.forward_device(x_pert, self.ids, self.mask, d["sigma"], self.style, self.keep)
        _tcheck(lib.dhw_train_loss(self.eps.data_ptr(), score.data_ptr(), self.pen.data_ptr(), pen_pred.data_ptr(), d["alphas"].data_ptr(), B, L,
                                   self.out.data_ptr(), None, None, st))

    def __call__(self) -> torch.Tensor:
        K, model = len(self.levels), self.model
        saved = (model.drop_rate, model.style_drop)
        model.drop_rate, model.style_drop = 0.0, 0.0
        try:
            self.acc.zero_()
            for i in range(self.batches):
                for k in range(K):
                    self._stage_dev.copy_(self._stage_host[i * K + k], non_blocking=True)
                    self._body()
                    self.acc[k] += self.out
        finally:
            model.drop_rate, model.style_drop = saved
            model.tape = None
        return self.acc / self.batches
