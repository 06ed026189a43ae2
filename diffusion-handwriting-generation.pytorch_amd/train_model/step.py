"""One update: ``train_step`` (eager, host-fed) and ``GraphedTrainStep`` (the staging block, the graph capture and the bucketed
graph segments)."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _lib
from ..train import Adam, GradBucketReducer, _stream, _tcheck, allreduce_grads, dist_state, get_alphas, loss_fn, noam_lr, perturb
from .data import ResidentData
from .net import N_BUCKETS, TrainModel

# DHW_TRAIN_BUCKETS=0: one flat SUM all-reduce behind the whole backward (rounds 2-4) instead of bucketed all-reduces overlapped with its tail (A/B)
GRAD_BUCKETS = os.environ.get("DHW_TRAIN_BUCKETS", "1") != "0"


def train_step(model: TrainModel, optimizer: Adam, batch: dict, alpha_set: torch.Tensor, step: int, *, eps: torch.Tensor | None = None,
               alphas: torch.Tensor | None = None, style_keep: torch.Tensor | None = None, drop_masks=None, d_model: int = 256,
               warmup: int = 10000, lr_mul: float = 1.0):
    """One update, in the reference's order (train.py:26-67): abar draw, eps draw, perturbation, forward, loss, backward,
    (data-parallel gradient mean when torch.distributed is initialised), clip + Adam at the Noam rate of update number ``step`` >= 1.
    batch: {"strokes" [B,L,3], "text" [B,Lt], "style" [B,S,1280]}.  Returns the device tensor (loss, score_loss, pen_loss)."""
    strokes3 = batch["strokes"]
    x, pen = strokes3[:, :, :2].float(), strokes3[:, :, 2].float()
    B = x.shape[0]
    if alphas is None:
        alphas = get_alphas(B, alpha_set)                    # [B, 1], torch's CPU generator like the reference
    if eps is None:
        eps = torch.randn(x.shape)
    x_pert = perturb(x, eps, alphas)
    model.zero_grad()
    dist_on, rank, world = dist_state()
    model.rng.copy_(torch.tensor([model.seed, step * world + rank], dtype=torch.int64))
    score, pen_pred = model.forward(x_pert, batch["text"], torch.sqrt(alphas), batch["style"], style_keep, drop_masks)
    out, d_score, d_pen = loss_fn(eps, score, pen, pen_pred, alphas)
    reducer = GradBucketReducer(model.flat_grad, model.bucket_ranges) if dist_on and GRAD_BUCKETS else None
    model.bucket_hook = reducer.launch if reducer else None
    try:
        model.backward(d_score, d_pen)
    finally:
        model.bucket_hook = None
    grads = model.grads()
    if reducer:
        reducer.launch(N_BUCKETS - 1)
        reducer.wait(average=True)
    elif dist_on:
        allreduce_grads(grads)
    model.last_grad_norm = float(optimizer.step(grads, noam_lr(step, d_model, warmup, lr_mul)))   # (one host sync per update)
    return out


def check_cond_drop(cond_drop) -> float:
    """The one rule for a conditioning-dropout probability (``GraphedTrainStep``, ``fit``): a real number in [0, 1]."""
    if isinstance(cond_drop, bool) or not isinstance(cond_drop, (int, float)) or not 0.0 <= float(cond_drop) <= 1.0:
        raise ValueError(f"cond_drop = {cond_drop!r} must be a number in [0, 1]")
    return float(cond_drop)


class GraphedTrainStep:
    """``train_step`` with its gradient computation captured once into a hipGraph and replayed: the ~1100 kernel launches of
    an update (draws, perturbation, forward, loss, backward) become one graph launch, which takes the host off the critical
    path; the gradient all-reduce (multi-rank) and clip + Adam follow as three eager launches.  The batch
    lives in static device buffers that each call overwrites; the step's learning rate and Adam bias corrections are 8 floats
    in device memory rewritten before every replay.  One instance serves one batch shape (B, L, Lt, S).  With an optimizer
    that keeps an EMA (``Adam(ema_decay=...)``) the block carries its two scalars as well and the fused pass updates the average
    wherever the optimizer runs: as the graph's last node, eagerly, or behind the collectives (every rank computes the same EMA).

    With ``data`` (a ``ResidentData``) the batch never crosses the bus: the step's first two launches draw B sample indices, the
    noise levels and the style sources (dhw_train_batch_draw) and gather the rows into the static buffers (dhw_train_batch_gather),
    inside the graph; the host sends the draw index and the optimizer's scalars only, and the call is ``step(step=n)``."""

    def __init__(self, model: TrainModel, optimizer: Adam, B: int, L: int, Lt: int, S: int = 14, d_model: int = 256, warmup: int = 10000,
                 lr_mul: float = 1.0, device_rng: bool = True, seed: int = 0, data: "ResidentData | None" = None, alpha_set=None,
                 cond_drop: float = 0.0):
        """``device_rng``: eps and the style Dropout mask are drawn inside the step by the library's Philox generator (as the
        reference draws them on its device, train.py:39, text_style.py:97); False: the caller passes them (tests).
        ``data`` with ``alpha_set`` (the schedule's cumulative products, uploaded here): train from the resident dataset; the step
        keeps ``data`` alive, since the captured graph holds its addresses.
        ``cond_drop`` in [0, 1]: conditioning dropout for classifier-free guidance (dhw_train_cond_drop) — with that probability a
        sample trains under ``null_condition`` instead of its prompt and writer; one launch on the step's own input buffers, behind
        the gather or the copy from the host and in front of the draws.  It needs ``device_rng=True``; 0 allocates and launches
        nothing."""
        check_cond_drop(cond_drop)
        if cond_drop > 0 and not device_rng:
            raise ValueError("cond_drop > 0 draws which samples lose their condition on the device: it needs device_rng=True")
        self.cond_drop = float(cond_drop)
        if data is not None:
            if not device_rng:
                raise ValueError("a step that draws its batch from resident data draws eps and the masks on the device too (device_rng=True)")
            if (data.L, data.Lt, data.S) != (L, Lt, S):
                raise ValueError(f"the resident data holds strokes [N, {data.L}, 3], text [N, {data.Lt}], style [N, {data.S}, 1280]; "
                                 f"this step is built for L = {L}, Lt = {Lt}, S = {S}")
            if alpha_set is None or len(alpha_set) < 2:
                raise ValueError("a step on resident data needs alpha_set (at least two cumulative products) at construction")
            if data.max_token >= model.p["text_style_model.emb.weight"].d.shape[0]:
                raise ValueError("token id out of the embedding's range")
            index = lambda d: torch.cuda.current_device() if torch.device(d).index is None else torch.device(d).index   # noqa: E731
            if index(data.dev) != index(model.dev):
                raise ValueError(f"the resident data lives on {data.dev}, the model on {model.dev}")
        elif alpha_set is not None:
            raise ValueError("alpha_set at construction belongs to a step on resident data; a host-fed step takes it per call")
        dev = model.dev
        self.data = data
        self.device_rng, self.seed = device_rng, seed
        self.model, self.opt = model, optimizer
        self.shape = (B, L, Lt, S)
        self.sched = (d_model, warmup, lr_mul)
        z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
        # Every per-update input lives in ONE device block that a single asynchronous copy from pinned host memory fills (the
        # separate pageable copies of round 3 — strokes, pen, alphas, sigma, ids, mask, style, hyper, rng: nine host-blocking
        # transfers — left the GPU idle for ~0.4 ms between two updates, rocprofv3 trace of tools/bench_train.py).  Two pinned
        # blocks alternate, so the host fills update k + 1's inputs while update k runs.
        fields = [("ids", (B, Lt), torch.int64), ("rng", (2,), torch.int64), ("x", (B, L, 2), torch.float32), ("pen", (B, L), torch.float32),
                  ("alphas", (B,), torch.float32), ("sigma", (B, 1), torch.float32), ("mask", (B, Lt), torch.float32),
                  ("hyper", (9,), torch.float32), ("style", (B, S, 1280), torch.float32)]
        if data is not None:       # the batch is gathered on the device: the block is the draw index and the optimizer's scalars, 64 bytes
            resident = {name: torch.zeros(shape, dtype=dt, device=dev) for name, shape, dt in fields if name not in ("rng", "hyper")}
            fields = [f for f in fields if f[0] in ("rng", "hyper")]
            self.idx, self.style_src = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            self.abar = torch.as_tensor(alpha_set, dtype=torch.float32).contiguous().to(dev)
        if not device_rng:
            fields += [("eps", (B, L, 2), torch.float32), ("keep", (B, S, 1280), torch.float32)]
        if getattr(optimizer, "ema", None) is not None:   # (appended, and only then: the block of a step without EMA is laid out as it always was)
            fields += [("ema", (2,), torch.float32)]
        offs, off = {}, 0
        for name, shape, dt in fields:
            n = int(np.prod(shape)) * (8 if dt == torch.int64 else 4)
            offs[name] = (off, n, shape, dt)
            off += (n + 15) // 16 * 16
        self._stage_dev = torch.zeros(off, dtype=torch.uint8, device=dev)
        self._stage_host = [torch.zeros(off, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._stage_ev = [None, None]
        self._stage_turn = 0
        carve = lambda buf: {k: buf[o:o + n].view(dt).view(shape) for k, (o, n, shape, dt) in offs.items()}   # noqa: E731
        self._dv, self._hv = carve(self._stage_dev), [carve(h) for h in self._stage_host]
        d = self._dv if data is None else {**self._dv, **resident}
        self.x, self.pen, self.alphas, self.sigma, self.ids, self.mask, self.style, self.hyper = (d[k] for k in ("x", "pen", "alphas", "sigma", "ids", "mask", "style", "hyper"))
        self.ema_hyper = d.get("ema")           # the optimizer's {decay, 1 - decay} in the block, or None
        self.eps = d["eps"] if not device_rng else z(B, L, 2)
        self.keep = d["keep"] if not device_rng else z(B, S, 1280)
        d["rng"].copy_(model.rng)
        self.rng = model.rng = d["rng"]      # (the model's dropout sites read the same generator state: one pointer, inside the block)
        self.sqnorm, self.out = z(1), z(3)
        self.dropped = torch.zeros(B, dtype=torch.int32, device=dev) if self.cond_drop > 0 else None
        model.prepare_tables(L, Lt)
        self.graph = None
        self.segments, self._reducer = None, None     # with a process group: N_BUCKETS graph segments + the bucketed all-reduce
        self._opt_in_graph = False

    def _body(self):
        """Everything of one update that runs on the device (what the graph holds)."""
        m = self.model
        B, L = self.shape[:2]
        x_pert = torch.empty_like(self.x)
        lib = _lib.lib()
        st = _stream(m.dev)
        if self.data is not None:
            dt, tb = self.data, self.data.tables or (None,) * 4
            ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
            _tcheck(lib.dhw_train_batch_draw(self.rng.data_ptr(), dt.N, B, self.abar.data_ptr(), self.abar.numel(), *(ptr(t) for t in tb), self.idx.data_ptr(),
                                             self.style_src.data_ptr(), self.alphas.data_ptr(), self.sigma.data_ptr(), st))
            _tcheck(lib.dhw_train_batch_gather(dt.strokes.data_ptr(), dt.text.data_ptr(), dt.style.data_ptr(), self.idx.data_ptr(), self.style_src.data_ptr(),
                                               dt.N, B, L, dt.Lt, dt.S, self.x.data_ptr(), self.pen.data_ptr(), self.ids.data_ptr(), self.mask.data_ptr(),
                                               self.style.data_ptr(), st))
        if self.cond_drop > 0:
            _tcheck(lib.dhw_train_cond_drop(self.rng.data_ptr(), B, self.shape[2], self.shape[3], self.cond_drop, self.ids.data_ptr(), self.mask.data_ptr(),
                                            self.style.data_ptr(), self.dropped.data_ptr(), st))
        if self.device_rng:
            _tcheck(lib.dhw_train_draw(self.rng.data_ptr(), B, L, self.eps.data_ptr(), self.keep.numel(), self.keep.numel() // B,
                                       TrainModel.STYLE_DROP, self.keep.data_ptr(), st))
        _tcheck(lib.dhw_train_perturb(self.x.data_ptr(), self.eps.data_ptr(), self.alphas.data_ptr(), B, L, x_pert.data_ptr(), st))
        m.zero_grad()
        score, pen_pred = m.forward_device(x_pert, self.ids, self.mask, self.sigma, self.style, self.keep)
        d_score, d_pen = torch.empty_like(score), torch.empty_like(pen_pred)
        _tcheck(lib.dhw_train_loss(self.eps.data_ptr(), score.data_ptr(), self.pen.data_ptr(), pen_pred.data_ptr(), self.alphas.data_ptr(), B, L,
                                   self.out.data_ptr(), d_score.data_ptr(), d_pen.data_ptr(), st))
        m.backward(d_score, d_pen)

    def _apply(self, reducer=None):
        """The optimizer behind the gradient all-reduce.  ``reducer``: the update's bucketed all-reduces are already in flight
        (GradBucketReducer: launched bucket by bucket while the backward was still running) — wait for them; without one
        (DHW_TRAIN_BUCKETS=0) ONE SUM all-reduce of the flat 40 MB buffer, issued here, behind the whole backward.  Adam applies
        1 / world size (hyper[8]) in its own pass either way; the collectives stay outside the captured graphs."""
        m = self.model
        if reducer is not None:
            reducer.launch(N_BUCKETS - 1)
            reducer.wait()
        elif dist_state()[0]:
            allreduce_grads(m.grads(), average=False)
        self.opt.step_dev(m.grads(), self.hyper, self.sqnorm, self.ema_hyper)

    def _capture_segments(self):
        """With a process group the update is captured as N_BUCKETS graph SEGMENTS cut at the tape's bucket markers (one shared
        memory pool, replayed in capture order): after segment i has been enqueued, gradient bucket i is final and its all-reduce is
        issued beside segment i + 1."""
        import gc
        m = self.model
        gc.collect()
        torch.cuda.synchronize(m.dev)
        segs = []
        side = torch.cuda.Stream(device=m.dev)
        side.wait_stream(torch.cuda.current_stream(m.dev))
        with torch.cuda.stream(side):
            cur = torch.cuda.CUDAGraph()
            cur.capture_begin()

            def cut(i):
                nonlocal cur
                cur.capture_end()
                segs.append(cur)
                if i != len(segs) - 1:
                    raise RuntimeError(f"gradient bucket markers fired out of order: {i} after {len(segs) - 1} segments")
                cur = torch.cuda.CUDAGraph()
                cur.capture_begin(pool=segs[0].pool())
            m.bucket_hook = cut
            try:
                self._body()
            finally:
                m.bucket_hook = None
                cur.capture_end()
            segs.append(cur)
        torch.cuda.current_stream(m.dev).wait_stream(side)
        if len(segs) != N_BUCKETS:
            raise RuntimeError(f"captured {len(segs)} graph segments for {N_BUCKETS} gradient buckets")
        return segs

    def last_draw(self):
        """The device tensors (idx int32 [B], style_src int32 [B], alphas f32 [B]) of the last update of a step on resident data:
        the samples it trained on, where each one's style row came from, and the noise levels."""
        if self.data is None:
            raise ValueError("this step is fed from the host: it draws no batch")
        return self.idx, self.style_src, self.alphas

    def last_dropped(self):
        """The device tensor int32 [B] of the last update of a step with ``cond_drop`` > 0: 1 where the sample trained under the
        null condition."""
        if self.dropped is None:
            raise ValueError("this step was built with cond_drop = 0: it drops no condition")
        return self.dropped

    def __call__(self, batch: dict | None = None, alpha_set=None, step: int | None = None, *, eps=None, alphas=None, style_keep=None, graph: bool = True):
        """Host-fed: ``step(batch, alpha_set, n)``.  On resident data: ``step(step=n)`` — the batch, the noise levels, eps and the
        masks are all drawn on the device from (seed, n), so passing any of them is an error."""
        alphas = self._check_args(batch, alpha_set, step, eps, alphas, style_keep)
        dist_on, rank, world = dist_state()
        self._send(step, rank, world, batch, alphas, eps, style_keep)
        return self._run(graph, dist_on)

    def _check_args(self, batch, alpha_set, step, eps, alphas, style_keep):
        """The argument rules, before anything is written -> the noise levels of a host-fed step (drawn here when omitted)."""
        if self.data is not None:
            given = [k for k, v in (("batch", batch), ("alpha_set", alpha_set), ("alphas", alphas), ("eps", eps), ("style_keep", style_keep)) if v is not None]
            if given:
                raise ValueError(f"this step draws its batch from resident data: call step(step=n) without {', '.join(given)}")
        if step is None:
            raise ValueError("step (the update number, >= 1) is required")
        B, L, Lt, S = self.shape
        if self.data is None:
            if batch is None:
                raise ValueError("a host-fed step needs a batch")
            if tuple(batch["strokes"].shape) != (B, L, 3) or tuple(batch["text"].shape) != (B, Lt) or tuple(batch["style"].shape) != (B, S, 1280):
                raise ValueError(f"this step was built for strokes {(B, L, 3)}, text {(B, Lt)}, style {(B, S, 1280)}")
            self.model.check_tokens(batch["text"])
            if alphas is None:
                alphas = get_alphas(B, alpha_set)
        if self.device_rng and (eps is not None or style_keep is not None):
            raise ValueError("this step draws eps and the dropout mask on the device (device_rng=True)")
        return alphas

    def _send(self, step, rank, world, batch, alphas, eps, style_keep):
        """Fill this turn's pinned block — the draw index, the optimizer's scalars and, host-fed, the batch — and send it with one
        asynchronous copy, in this order: wait for the copy that last read the block, fill, copy, record the block's event."""
        B, L, _, S = self.shape
        turn = self._stage_turn
        self._stage_turn ^= 1
        if self._stage_ev[turn] is not None:
            self._stage_ev[turn].synchronize()       # the copy that last read this pinned block (two updates ago) has finished
        hv = self._hv[turn]
        hv["rng"][0], hv["rng"][1] = self.seed, step * world + rank
        if not self.device_rng:
            hv["eps"].copy_(eps if eps is not None else torch.randn(B, L, 2))
            hv["keep"].copy_(style_keep if style_keep is not None else (torch.rand(B, S, 1280) >= TrainModel.STYLE_DROP).float())
        if self.data is None:
            strokes3 = batch["strokes"]
            hv["x"].copy_(strokes3[:, :, :2])
            hv["pen"].copy_(strokes3[:, :, 2])
            hv["alphas"].copy_(alphas.reshape(B))
            hv["sigma"].copy_(torch.sqrt(alphas).reshape(B, 1))
            hv["ids"].copy_(batch["text"])
            hv["mask"].copy_(batch["text"] == 0)
            hv["style"].copy_(batch["style"])
        hv["hyper"].copy_(torch.tensor(self.opt.hyper(noam_lr(step, *self.sched), 1.0 / world), dtype=torch.float32))
        if self.ema_hyper is not None:      # (behind hyper(): the decay of the update it has just counted)
            hv["ema"].copy_(torch.tensor(self.opt.ema_hyper(), dtype=torch.float32))
        self._gscale = 1.0 / world
        self._stage_dev.copy_(self._stage_host[turn], non_blocking=True)
        ev = self._stage_ev[turn] = self._stage_ev[turn] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.model.dev))

    def _run(self, graph: bool, dist_on: bool):
        """The update on the block just sent: eagerly, as graph segments around the bucketed all-reduces, or as one graph."""
        bucketed = dist_on and GRAD_BUCKETS
        if bucketed and self._reducer is None:
            self._reducer = GradBucketReducer(self.model.flat_grad, self.model.bucket_ranges)
        reducer = self._reducer if bucketed else None
        if not graph:
            self.model.bucket_hook = reducer.launch if bucketed else None
            try:
                self._body()
            finally:
                self.model.bucket_hook = None
        elif bucketed:
            if self.graph is not None:
                raise RuntimeError("this step was captured without a process group; build a new GraphedTrainStep after init_process_group")
            if self.segments is None:
                self.segments = self._capture_segments()
            for i, g in enumerate(self.segments):
                g.replay()
                if i < N_BUCKETS - 1:
                    reducer.launch(i)       # bucket i is final behind segment i: its all-reduce runs beside segment i + 1
        else:
            if self.graph is None:
                # loss_kernel accumulates into out[1], out[2] — dhw_train_loss zeroes them itself; capture on torch's capture stream.
                # Without a process group there is nothing between the backward and the optimizer: clip + Adam are the graph's last
                # nodes and an update is ONE launch; with one, the collective stays outside the capture and the optimizer follows it.
                self._opt_in_graph = not dist_on
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self._body()
                    if self._opt_in_graph:
                        self.opt.step_dev(self.model.grads(), self.hyper, self.sqnorm, self.ema_hyper)
            elif self._opt_in_graph and dist_on:
                raise RuntimeError("this step was captured without a process group; build a new GraphedTrainStep after init_process_group")
            self.graph.replay()
            if self._opt_in_graph:
                return self.out
        self._apply(reducer)
        return self.out

    def grad_norm(self) -> float:
        """||g|| of the last update before clipping (one host synchronisation)."""
        return float(self.sqnorm.sqrt()) * getattr(self, "_gscale", 1.0)
