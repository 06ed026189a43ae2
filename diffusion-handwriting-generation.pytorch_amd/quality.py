"""Sample quality: the Fréchet distance between real and generated lines in the StyleExtractor's feature space.

A line is rendered (``render_strokes``), turned into [14,1280] style features (``StyleExtractor``) and pooled over the 14
positions; ``FeatureStats`` keeps the running sum and Gram matrix of those vectors in double precision on the GPU
(include/dhw.h dhw_moments_update), and ``frechet_distance`` compares two such statistics on the host in numpy float64.
"""
from __future__ import annotations

import ctypes as C
import time
import warnings

import numpy as np

MOMENTS_MAX_N, MOMENTS_MAX_S, MOMENTS_MIN_D, MOMENTS_MAX_D = 16384, 64, 16, 2048   # csrc/moments/moments.h
_workspaces = {}   # device index -> workspace tensors of dhw_moments_update (vis._workspace)


class FeatureStats:
    """Count, sum and Gram matrix of D-dimensional feature vectors, accumulated batch by batch in float64 on the GPU.

    The state lives on the host until the first ``update`` (so ``load`` / ``save`` / ``mean`` / ``cov`` need no device) and on
    ``device`` from then on, as one f64 buffer [D + D*D] = (sum, gram)."""

    chunk = MOMENTS_MAX_N   # samples per dhw_moments_update call (at most MOMENTS_MAX_N)

    def __init__(self, D: int = 1280, device=None):
        if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or D < MOMENTS_MIN_D or D > MOMENTS_MAX_D or D % 16:
            raise ValueError(f"D = {D!r} must be a multiple of 16 in [{MOMENTS_MIN_D}, {MOMENTS_MAX_D}]")
        self.D = int(D)
        self.device = device
        self.count = 0
        self._host = np.zeros(self.D + self.D * self.D, np.float64)
        self._dev = None

    @classmethod
    def from_state(cls, count: int, sum, gram, device=None) -> "FeatureStats":
        """Statistics from a count, a sum [D] and a Gram matrix [D,D] (what ``save`` writes)."""
        s, g = np.asarray(sum, np.float64), np.asarray(gram, np.float64)
        if s.ndim != 1 or g.shape != (s.shape[0], s.shape[0]):
            raise ValueError(f"sum must be [D] and gram [D, D], got {s.shape} and {g.shape}")
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 0:
            raise ValueError(f"count = {count!r} must be a non-negative integer")
        st = cls(s.shape[0], device)
        st.count = int(count)
        st._host[:st.D], st._host[st.D:] = s, g.reshape(-1)
        return st

    # ------------------------------------------------------------ accumulation (GPU)
    def update(self, features) -> "FeatureStats":
        """Add ``features``, [N,S,D] (pooled over S) or [N,D], a tensor on any device or an array."""
        import torch

        x = features if isinstance(features, torch.Tensor) else torch.as_tensor(np.asarray(features))
        if x.dim() == 2:
            x = x.unsqueeze(1)
        if x.dim() != 3 or x.shape[2] != self.D or not x.is_floating_point():
            raise ValueError(f"features must be floating-point [N, S, {self.D}] or [N, {self.D}], got {tuple(x.shape)} {x.dtype}")
        N, S = int(x.shape[0]), int(x.shape[1])
        if not 1 <= S <= MOMENTS_MAX_S:
            raise ValueError(f"features hold S = {S} positions per sample, must be in [1, {MOMENTS_MAX_S}]")
        if N == 0:
            return self
        if not torch.cuda.is_available():
            raise RuntimeError("FeatureStats.update needs an MI355X (HIP device): there is no CPU path in this package")
        from . import _lib
        from .vis import _workspace

        if self._dev is None:
            dev = torch.device(self.device) if self.device is not None else (x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device()))
            self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
            self._dev = torch.from_numpy(self._host).to(self.device)
            self._host = None
        dev, D, l = self.device, self.D, _lib.lib()
        step = max(1, min(int(self.chunk), MOMENTS_MAX_N, (2 ** 31 - 1) // (S * D)))
        with torch.cuda.device(dev):
            x = x.detach().to(dev, torch.float32).contiguous()
            st = torch.cuda.current_stream(dev)
            for lo in range(0, N, step):
                n = min(step, N - lo)
                need = int(l.dhw_moments_workspace_bytes(n, S, D))
                ws = _workspace(_workspaces, dev, need)
                _lib.check(l.dhw_moments_update(x[lo:lo + n].data_ptr(), n, S, D, self._dev.data_ptr(), self._dev[D:].data_ptr(), ws.data_ptr(),
                                                need, C.c_void_p(st.cuda_stream)))
            x.record_stream(st)
        self.count += N
        return self

    # ------------------------------------------------------------ reading
    def _state(self):
        """(sum [D], gram [D,D]) as numpy float64: one device read."""
        a = self._host if self._dev is None else self._dev.cpu().numpy()
        return a[:self.D], a[self.D:].reshape(self.D, self.D)

    def _finite_state(self, least: int):
        if self.count < least:
            raise ValueError(f"FeatureStats holds {self.count} samples, fewer than {least}")
        s, g = self._state()
        if not (np.isfinite(s).all() and np.isfinite(g).all()):
            raise ValueError("FeatureStats holds a non-finite state: a feature was NaN or infinite")
        return s, g

    def mean(self) -> np.ndarray:
        return self._finite_state(1)[0] / self.count

    def moments(self):
        """(mean [D], unbiased covariance [D,D]) from one device read."""
        s, g = self._finite_state(2)
        m = s / self.count
        c = (g - self.count * np.outer(m, m)) / (self.count - 1)
        return m, (c + c.T) * 0.5

    def cov(self) -> np.ndarray:
        return self.moments()[1]

    def save(self, path) -> None:
        s, g = self._state()
        with open(path, "wb") as f:   # (an open file: np.savez appends no suffix)
            np.savez(f, count=np.int64(self.count), sum=s, gram=g)

    @classmethod
    def load(cls, path, device=None) -> "FeatureStats":
        with np.load(path) as z:
            return cls.from_state(int(z["count"]), z["sum"], z["gram"], device)


def _mean_cov(x):
    if isinstance(x, FeatureStats):
        if x.count <= x.D:
            warnings.warn(f"frechet_distance: {x.count} samples for D = {x.D} features: the covariance is rank-deficient and the "
                          "distance is biased (use more samples than dimensions)")
        return x.moments()
    m, c = x
    m, c = np.asarray(m, np.float64), np.asarray(c, np.float64)
    if m.ndim != 1 or c.shape != (m.shape[0], m.shape[0]):
        raise ValueError(f"a (mean, cov) pair must be ([D], [D, D]), got {m.shape} and {c.shape}")
    return m, c


def frechet_distance(a, b) -> float:
    """|mu_a - mu_b|^2 + tr C_a + tr C_b - 2 tr (C_a^1/2 C_b C_a^1/2)^1/2 between two ``FeatureStats`` or two (mean, cov) pairs,
    on the host in float64.  Both square roots come from symmetric eigen-decompositions with the eigenvalues clipped at 0: no
    inverse and no general matrix square root, so a rank-deficient covariance is legal."""
    (ma, ca), (mb, cb) = _mean_cov(a), _mean_cov(b)
    if ma.shape != mb.shape:
        raise ValueError(f"the two statistics have {ma.shape[0]} and {mb.shape[0]} dimensions")
    w, v = np.linalg.eigh((ca + ca.T) * 0.5)
    root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = root @ ((cb + cb.T) * 0.5) @ root
    lam = np.linalg.eigvalsh((m + m.T) * 0.5)
    d = ma - mb
    return float(d @ d + np.trace(ca) + np.trace(cb) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def line_features(strokes, extractor, lengths=None, batch: int = 32):
    """Strokes [N,L,3] -> style features [N,14,1280] on the device: ``render_strokes`` then ``extractor``, ``batch`` lines at a time."""
    import torch

    from .vis import render_strokes
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"batch = {batch!r} must be a positive integer")
    N = int(strokes.shape[0])
    if lengths is not None and len(lengths) != N:
        raise ValueError(f"lengths must hold {N} entries")
    out = []
    for lo in range(0, N, batch):
        images, _ = render_strokes(strokes[lo:lo + batch], None if lengths is None else lengths[lo:lo + batch])
        out.append(extractor(images))
    return torch.cat(out) if len(out) != 1 else out[0]


_SAMPLE_KW = {"T", "diffusion_mode", "guidance"}
_DDIM_KW = {"T", "steps", "levels", "guidance"}


def _sampler_of(sampler: dict):
    """Which sampler the keywords select: ``sample_ddim`` when steps / levels is among them, else ``sample``; TypeError for a
    keyword that sampler does not take."""
    ddim = "steps" in sampler or "levels" in sampler
    unknown = sorted(set(sampler) - (_DDIM_KW if ddim else _SAMPLE_KW))
    if unknown:
        raise TypeError(f"sample_quality: unknown sampler keyword(s) {', '.join(unknown)} for {'sample_ddim' if ddim else 'sample'} "
                        f"(known: {', '.join(sorted(_DDIM_KW if ddim else _SAMPLE_KW))})")
    return ddim


def sample_quality(model, data, extractor, n=None, batch: int = 32, seed: int = 0, real=None, timings=None, **sampler):
    """Fréchet distance between the lines of a data set and lines the model samples for the same rows.

    ``data``: the dict ``train.py --val`` reads, {"strokes" [N,L,3], "text" [N,Lt], "style" [N,S,1280]}.  The first ``n`` rows
    (default all) are used.  Real statistics come from ``data["strokes"]``, or from ``real`` (a ``FeatureStats``, e.g. loaded from
    a file) when given.  Generated lines come from ``sample`` (keywords T, diffusion_mode, guidance), or from ``sample_ddim`` when
    ``steps=`` or ``levels=`` is among the keywords, with the rows' text and style at L = data["strokes"].shape[1], ``batch`` rows
    per call and ``first_sample`` = the row index, so the result does not depend on ``batch``.  ``timings`` (a dict): filled with
    the seconds spent in sampling, rendering + features, moments and the host eigen-decompositions (synchronises per stage).
    Returns (fd, real_stats, generated_stats)."""
    ddim = _sampler_of(sampler)
    for k in ("strokes", "text", "style"):
        if k not in data:
            raise ValueError(f"data must hold 'strokes', 'text' and 'style' (missing {k!r})")
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"batch = {batch!r} must be a positive integer")
    total = int(data["strokes"].shape[0])
    n = total if n is None else n
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= n <= total:
        raise ValueError(f"n = {n!r} must be an integer in [2, {total}] (the rows of data)")
    if real is not None and not isinstance(real, FeatureStats):
        raise ValueError("real must be a FeatureStats")
    import torch

    from .inference import sample, sample_ddim
    dev = extractor.device
    L = int(data["strokes"].shape[1])
    t = dict(sample=0.0, features=0.0, moments=0.0, eig=0.0)

    def tick():
        if timings is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    if real is None:
        real = FeatureStats(1280, dev)
        for lo in range(0, n, batch):
            t0 = tick()
            f = line_features(torch.as_tensor(data["strokes"][lo:min(lo + batch, n)]), extractor, batch=batch)
            t1 = tick()
            real.update(f)
            t2 = tick()
            t["features"], t["moments"] = t["features"] + t1 - t0, t["moments"] + t2 - t1
    gen = FeatureStats(1280, dev)
    draw = sample_ddim if ddim else sample
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        t0 = tick()
        lines = draw(model, torch.as_tensor(data["text"][lo:hi]).to(dev), torch.as_tensor(data["style"][lo:hi]).to(dev), L=L, seed=seed,
                     first_sample=lo, **sampler)
        t1 = tick()
        f = line_features(lines, extractor, batch=batch)
        t2 = tick()
        gen.update(f)
        t3 = tick()
        t["sample"], t["features"], t["moments"] = t["sample"] + t1 - t0, t["features"] + t2 - t1, t["moments"] + t3 - t2
    t0 = time.perf_counter()
    fd = frechet_distance(real, gen)
    t["eig"] = time.perf_counter() - t0
    if timings is not None:
        timings.update(t)
    return fd, real, gen
