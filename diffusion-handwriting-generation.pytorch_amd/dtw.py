"""Dynamic time warping between stroke lines (include/dhw.h dhw_dtw): a distance in stroke space itself, which
sees what a rendered image forgets (pen order, speed, lifts, a uniform scaling) and needs no trained network.

``stroke_features`` turns model strokes (dx, dy, pen) into the rows the kernel compares, ``dtw_distance`` gives the distance and
path length of every pair of two sets, and ``nearest_strokes`` the nearest line of a set for every query ("is this sample a
time-warped copy of a training line?").
"""
from __future__ import annotations

import numpy as np

from . import _call

DTW_MAX_N, DTW_MAX_PAIRS, DTW_MAX_L, DTW_MAX_F = 16384, 1 << 26, 1024, 4   # csrc/dtw/dtw.h
KINDS = ("positions", "offsets")
WHO = "dynamic time warping"   # in the no-GPU refusal of every function here


def _check_strokes(strokes, lengths, who: str):
    """(strokes as a float32 tensor [B,L,3] on its own device, lengths as an int64 host array [B] or None); ValueError for a shape,
    a length outside [1, L] or a non-finite value in a row below its line's length.  Host inputs are checked on the host."""
    import torch

    x = strokes if isinstance(strokes, torch.Tensor) else torch.as_tensor(np.asarray(strokes))
    if x.dim() != 3 or x.shape[2] != 3 or not x.is_floating_point() or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: strokes must be floating-point [B, L, 3] with B, L >= 1, got {tuple(x.shape)} {x.dtype}")
    B, L = int(x.shape[0]), int(x.shape[1])
    if L > DTW_MAX_L:
        raise ValueError(f"{who}: lines of L = {L} rows: at most {DTW_MAX_L}")
    lens = None
    if lengths is not None:
        lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)
        if lens.shape != (B,) or lens.dtype.kind not in "iu":
            raise ValueError(f"{who}: lengths must hold {B} integers, got shape {lens.shape} {lens.dtype}")
        lens = lens.astype(np.int64)
        if lens.min() < 1 or lens.max() > L:
            raise ValueError(f"{who}: lengths must lie in [1, {L}] (got {int(lens.min())} .. {int(lens.max())})")
    x = x.detach().to(torch.float32)
    used = x if lens is None else x[torch.arange(L, device=x.device)[None, :] < torch.from_numpy(lens).to(x.device)[:, None]]
    if not bool(torch.isfinite(used).all()):
        raise ValueError(f"{who}: strokes hold a non-finite value (NaN or infinite)")
    return x, lens


def _check_kind(kind, pen_weight, who: str):
    if kind not in KINDS:
        raise ValueError(f"{who}: kind = {kind!r} must be one of {', '.join(KINDS)}")
    if not _call.is_number(pen_weight) or not np.isfinite(pen_weight) or pen_weight < 0:
        raise ValueError(f"{who}: pen_weight = {pen_weight!r} must be a finite number >= 0")


def _features(x, kind: str, pen_weight, dev):
    """The checked strokes `x` -> features f32 [B,L,3] on `dev` (torch element-wise ops and one prefix sum: preparation, not the hot path)."""
    import torch

    x = x.to(dev)
    out = torch.empty_like(x)
    if kind == "offsets":
        out[..., :2] = x[..., :2]
    else:
        pos = torch.cumsum(torch.nan_to_num(x[..., :2].double(), nan=0.0, posinf=0.0, neginf=0.0), dim=1)   # (rows past a length may hold anything)
        out[..., :2] = (pos - pos[:, :1]).float()
    out[..., 2] = float(np.float32(np.sqrt(np.float64(pen_weight)))) * (torch.round(x[..., 2]) != 0).float()
    return out


def stroke_features(strokes, lengths=None, kind: str = "positions", pen_weight: float = 1.0):
    """Model strokes [B,L,3] = (dx, dy, pen) -> the rows ``dtw_distance`` compares, float32 [B,L,3] on the device.

    Channels 0 and 1: ``kind="offsets"`` keeps (dx, dy), which compares pen velocity; ``kind="positions"`` gives pos[i] - pos[0],
    the prefix sums taken in float64 and rounded once, which compares the trajectory itself and so sees a uniform scaling.
    Channel 2 is sqrt(pen_weight) (rint(pen) != 0): a pen lift matched to a row without one costs ``pen_weight``.  Rows at or
    past a line's length are carried along unread.  ValueError for non-finite strokes and lengths outside [1, L]."""
    _check_kind(kind, pen_weight, "stroke_features")
    x, _ = _check_strokes(strokes, lengths, "stroke_features")
    return _features(x, kind, pen_weight, _call.pick_device(WHO, like=x))


def _aligned(t):
    """t, or a copy of it when its first byte is not 16-byte aligned (a slice of a larger tensor)."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def _chunks(n: int, step: int):
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def _check_chunk(chunk):
    if chunk is not None and not (_call.is_int(chunk) and 1 <= chunk <= DTW_MAX_N):
        raise ValueError(f"_chunk = {chunk!r} must be an integer in [1, {DTW_MAX_N}]")


def _steps(M: int, N: int, chunk):
    """Lines per call on each side: within the entry's limits (16384 lines a side, 2^26 pairs), or `chunk` when given."""
    if chunk is not None:
        return int(chunk), int(chunk)
    cn = min(N, DTW_MAX_N)
    return min(M, DTW_MAX_N, DTW_MAX_PAIRS // cn), cn


def _check_sets(a, b, lengths_a, lengths_b, kind, pen_weight, who):
    """The host rules of both sets -> (strokes a, lens a, strokes b, lens b, same); ``b`` None: ``a`` against itself."""
    _check_kind(kind, pen_weight, who)
    xa, la = _check_strokes(a, lengths_a, who)
    if b is None:
        if lengths_b is not None:
            raise ValueError(f"{who}: lengths of the second set were given without the set")
        return xa, la, xa, la, True
    return (xa, la) + _check_strokes(b, lengths_b, who) + (False,)


def _stage(c, xa, la, xb, lb, same, kind, pen_weight):
    """The checked sets on the call's device: (features a, lens a, features b, lens b); lens are int32 tensors or None."""
    import torch

    fa = _features(xa, kind, pen_weight, c.dev).contiguous()
    fb = fa if same else _features(xb, kind, pen_weight, c.dev).contiguous()
    da = None if la is None else torch.from_numpy(la.astype(np.int32)).to(c.dev)
    db = da if same else None if lb is None else torch.from_numpy(lb.astype(np.int32)).to(c.dev)
    return fa, da, fb, db


def _run(c, fa, la, fb, lb, normalize, skip_diag, dist, steps, near, idx):
    """One dhw_dtw call on the stream of `c`; the tensors are contiguous and 16-byte aligned."""
    M, La, N, Lb = int(fa.shape[0]), int(fa.shape[1]), int(fb.shape[0]), int(fb.shape[1])
    ws, need = c.workspace("dtw", "dhw_dtw_workspace_bytes", M, N, La, Lb, 3)
    c.run("dhw_dtw", fa.data_ptr(), c.ptr(la), M, La, fb.data_ptr(), c.ptr(lb), N, Lb, 3, int(bool(normalize)), int(bool(skip_diag)),
          c.ptr(dist), c.ptr(steps), c.ptr(near), c.ptr(idx), c.ptr(ws), need)


def dtw_distance(a, b=None, lengths_a=None, lengths_b=None, kind: str = "positions", pen_weight: float = 1.0, normalize: bool = True, _chunk=None):
    """DTW between every line of ``a`` [M,La,3] and every line of ``b`` [N,Lb,3] (``b=None``: ``a`` against itself), model strokes
    with optional lengths: (dist float32 [M,N], steps int32 [M,N]) on the device.  dist is the summed squared feature distance
    along the best warping path (``stroke_features``), divided by the path's number of cells ``steps`` when ``normalize``.  Sets
    beyond one call's limits (16384 lines a side, 2^26 pairs) are computed in blocks; ``_chunk`` (tests) forces blocks of that
    many lines a side.  A pair's bits do not depend on the blocks.  One workspace is cached per device: calls on one device must
    be ordered on one stream."""
    import torch

    _check_chunk(_chunk)
    xa, la, xb, lb, same = _check_sets(a, b, lengths_a, lengths_b, kind, pen_weight, "dtw_distance")
    with _call.open(WHO, like=xa) as c:
        fa, la, fb, lb = _stage(c, xa, la, xb, lb, same, kind, pen_weight)
        M, N = int(fa.shape[0]), int(fb.shape[0])
        cm, cn = _steps(M, N, _chunk)
        dist, steps = c.empty((M, N)), c.empty((M, N), torch.int32)
        for plo, phi in _chunks(M, cm):
            for qlo, qhi in _chunks(N, cn):
                whole = qlo == 0 and qhi == N
                d = dist[plo:phi] if whole else torch.empty((phi - plo, qhi - qlo), dtype=torch.float32, device=c.dev)   # (a block's own:
                k = steps[plo:phi] if whole else torch.empty((phi - plo, qhi - qlo), dtype=torch.int32, device=c.dev)    # not kept by c)
                da, ka = _aligned(d), _aligned(k)
                _run(c, _aligned(fa[plo:phi]), None if la is None else _aligned(la[plo:phi]), _aligned(fb[qlo:qhi]),
                     None if lb is None else _aligned(lb[qlo:qhi]), normalize, False, da, ka, None, None)
                if not whole or da is not d:
                    dist[plo:phi, qlo:qhi] = da
                    steps[plo:phi, qlo:qhi] = ka
    return dist, steps


def nearest_strokes(queries, refs=None, lengths_q=None, lengths_r=None, kind: str = "positions", pen_weight: float = 1.0, normalize: bool = True,
                    _chunk=None):
    """For every line of ``queries`` the nearest line of ``refs`` under ``dtw_distance``: (dist float32 [M], index int32 [M]; the
    smallest index on a tie) on the device.  ``refs=None``: the nearest *other* line of ``queries`` itself.  A distance near 0 to a
    training line is a time-warped copy of it.  The reference set is walked in blocks and the results merged, the smaller index
    kept on a tie."""
    import torch

    _check_chunk(_chunk)
    xa, la, xb, lb, same = _check_sets(queries, refs, lengths_q, lengths_r, kind, pen_weight, "nearest_strokes")
    with _call.open(WHO, like=xa) as c:
        fa, la, fb, lb = _stage(c, xa, la, xb, lb, same, kind, pen_weight)
        M, N = int(fa.shape[0]), int(fb.shape[0])
        if same and M < 2:
            raise ValueError("nearest_strokes: the nearest other line needs at least 2 lines")
        cm, cn = _steps(M, N, _chunk)
        if same:
            cm = cn = min(cm, cn)   # the same blocks on both sides: the diagonal lies in the blocks with equal bounds
        best = torch.full((M,), float("inf"), dtype=torch.float32, device=c.dev)
        best_idx = torch.full((M,), -1, dtype=torch.int32, device=c.dev)
        for plo, phi in _chunks(M, cm):
            for qlo, qhi in _chunks(N, cn):
                near = torch.empty(phi - plo, dtype=torch.float32, device=c.dev)
                idx = torch.empty(phi - plo, dtype=torch.int32, device=c.dev)
                _run(c, _aligned(fa[plo:phi]), None if la is None else _aligned(la[plo:phi]), _aligned(fb[qlo:qhi]),
                     None if lb is None else _aligned(lb[qlo:qhi]), normalize, same and (plo, phi) == (qlo, qhi), None, None, near, idx)
                better = near < best[plo:phi]     # blocks ascending and a strict comparison: the smaller index stays on a tie
                best[plo:phi] = torch.where(better, near, best[plo:phi])
                best_idx[plo:phi] = torch.where(better, idx + qlo, best_idx[plo:phi])
    return best, best_idx
