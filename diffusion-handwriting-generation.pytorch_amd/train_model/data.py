"""The resident dataset: ``group_tables`` (the style-source tables, on the host) and ``ResidentData`` (the training set uploaded
once, for a step that draws and gathers its batch in-graph)."""
from __future__ import annotations

import numpy as np
import torch

from .. import spec

def group_tables(writers):
    """The four int32 tables ``dhw_train_batch_draw`` picks a style source from, on the host: for ``writers`` = one integer id per
    sample [N] -> (grp_start [N], grp_size [N], grp_pos [N], members [N]).  ``members`` lists the samples writer by writer (each
    group in ascending sample order); sample n's group is ``members[grp_start[n] : grp_start[n] + grp_size[n]]`` and n itself sits
    at ``grp_pos[n]`` in it."""
    w = np.asarray(writers.cpu() if isinstance(writers, torch.Tensor) else writers)
    if w.ndim != 1 or w.size < 1 or w.dtype.kind not in "iu":
        raise ValueError(f"writers must be a non-empty 1-D integer array, got shape {tuple(w.shape)} dtype {w.dtype}")
    if w.size >= 2 ** 31:
        raise ValueError(f"{w.size} samples: the group tables are int32")
    n = w.size
    members = np.argsort(w, kind="stable")                                  # writer by writer, ascending sample index inside one
    sw = w[members]
    first = np.flatnonzero(np.concatenate(([True], sw[1:] != sw[:-1])))    # where each group starts in members
    sizes = np.diff(np.concatenate((first, [n])))
    start_of = np.repeat(first, sizes)                                      # per position in members: its group's start
    grp_start, grp_size, grp_pos = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    grp_start[members] = start_of
    grp_size[members] = np.repeat(sizes, sizes)
    grp_pos[members] = np.arange(n) - start_of
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (grp_start, grp_size, grp_pos, members))


class ResidentData:
    """A training set resident on the device: what ``train.py --data`` reads — {"strokes" f32 [N,L,3], "text" int64 [N,Lt], "style"
    f32 [N,S,1280]} and optionally ``writers`` (default ``data.get("writer")``), one integer id per sample — uploaded ONCE, for a
    ``GraphedTrainStep`` that draws and gathers its batch inside the replayed graph (dhw_train_batch_draw / _gather).  With writers
    the step takes each sample's style from a random OTHER line of the same writer at every update (reference dataset.py:110-115).
    Shapes, dtypes and every token id are checked here, once, before the device is touched; the upload is refused with both
    numbers when the bytes do not fit the device's free memory.  The tensors must not be written or replaced afterwards: captured
    graphs hold their addresses."""

    def __init__(self, data: dict, device=None, writers=None):
        for k in ("strokes", "text", "style"):
            if k not in data or not isinstance(data[k], torch.Tensor):
                raise ValueError(f"data[`{k}`] must be a torch tensor")
        st, tx, sy = data["strokes"], data["text"], data["style"]
        if st.dim() != 3 or st.shape[2] != 3 or st.dtype != torch.float32:
            raise ValueError(f"`strokes` must be float32 [N, L, 3], got {st.dtype} {tuple(st.shape)}")
        N, L = int(st.shape[0]), int(st.shape[1])
        if N < 1 or N >= 2 ** 31:
            raise ValueError(f"the dataset must hold 1 to 2^31 - 1 samples, got {N}")
        if L < 8 or L % 8:
            raise ValueError(f"the stroke length must be a positive multiple of 8 (three AvgPool1d(2) stages), got {L}")
        if tx.dim() != 2 or tx.shape[0] != N or tx.shape[1] < 1 or tx.dtype != torch.int64:
            raise ValueError(f"`text` must be int64 [{N}, Lt], got {tx.dtype} {tuple(tx.shape)}")
        if sy.dim() != 3 or sy.shape[0] != N or sy.shape[1] < 1 or sy.shape[2] != 1280 or sy.dtype != torch.float32:
            raise ValueError(f"`style` must be float32 [{N}, S, 1280], got {sy.dtype} {tuple(sy.shape)}")
        if int(tx.min()) < 0 or int(tx.max()) >= spec.VOCAB:
            raise ValueError(f"token id out of the embedding's range [0, {spec.VOCAB})")
        if writers is None:
            writers = data.get("writer")
        tables = None
        if writers is not None:
            w = np.asarray(writers.cpu() if isinstance(writers, torch.Tensor) else writers)
            if w.shape != (N,) or w.dtype.kind not in "iu":
                raise ValueError(f"writers must be an integer array [{N}], got shape {tuple(w.shape)} dtype {w.dtype}")
            tables = group_tables(w)
        self.N, self.L, self.Lt, self.S = N, L, int(tx.shape[1]), int(sy.shape[1])
        self.max_token = int(tx.max())
        need = sum(t.numel() * t.element_size() for t in (st, tx, sy)) + (16 * N if tables else 0)
        # ---- the device, from here on
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        free, _ = torch.cuda.mem_get_info(dev)
        if need > free:
            raise ValueError(f"the dataset needs {need} bytes on {dev}, which has {free} bytes free")
        self.dev, self.nbytes = dev, need
        self._strokes, self._text, self._style = (t.contiguous().to(dev) for t in (st, tx, sy))
        self._tables = tuple(t.to(dev) for t in tables) if tables else None

    strokes = property(lambda self: self._strokes)
    text = property(lambda self: self._text)
    style = property(lambda self: self._style)
    tables = property(lambda self: self._tables)       # (grp_start, grp_size, grp_pos, members) on the device, or None
