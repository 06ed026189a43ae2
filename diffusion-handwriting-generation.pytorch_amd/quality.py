"""Sample quality: the Fréchet distance between real and generated lines in the StyleExtractor's feature space.

A line is rendered (``render_strokes``), turned into [14,1280] style features (``StyleExtractor``) and pooled over the 14
positions; ``FeatureStats`` keeps the running sum and Gram matrix of those vectors in double precision on the GPU
(include/dhw.h dhw_moments_update), and ``frechet_distance`` compares two such statistics on the host in numpy float64.

``FeatureSet`` keeps the pooled vectors themselves, in float64 on the GPU; ``knn_radius``, ``nearest``, ``precision_recall``
(precision / recall, density / coverage) and ``kernel_distance`` (KID) are functions of the pairwise inner products of two such
sets (include/dhw.h dhw_pairs_*), and ``sample_metrics`` is ``sample_quality`` with all of them.
"""
from __future__ import annotations

import time
import warnings

import numpy as np

from . import _call

MOMENTS_MAX_N, MOMENTS_MAX_S, MOMENTS_MIN_D, MOMENTS_MAX_D = 16384, 64, 16, 2048   # csrc/moments/moments.h
PAIRS_MAX_N, PAIRS_MAX_K = 16384, 8                                               # csrc/pairs/pairs.h


def _check_D(D) -> int:
    if not _call.is_int(D) or D < MOMENTS_MIN_D or D > MOMENTS_MAX_D or D % 16:
        raise ValueError(f"D = {D!r} must be a multiple of 16 in [{MOMENTS_MIN_D}, {MOMENTS_MAX_D}]")
    return int(D)


def _check_features(features, D: int):
    """What ``FeatureStats.update`` and ``FeatureSet.update`` take -> (the features as a tensor [N,S,D] where they were, N, S)."""
    import torch

    x = features if isinstance(features, torch.Tensor) else torch.as_tensor(np.asarray(features))
    if x.dim() == 2:
        x = x.unsqueeze(1)
    if x.dim() != 3 or x.shape[2] != D or not x.is_floating_point():
        raise ValueError(f"features must be floating-point [N, S, {D}] or [N, {D}], got {tuple(x.shape)} {x.dtype}")
    N, S = int(x.shape[0]), int(x.shape[1])
    if not 1 <= S <= MOMENTS_MAX_S:
        raise ValueError(f"features hold S = {S} positions per sample, must be in [1, {MOMENTS_MAX_S}]")
    return x, N, S


class FeatureStats:
    """Count, sum and Gram matrix of D-dimensional feature vectors, accumulated batch by batch in float64 on the GPU.

    The state lives on the host until the first ``update`` (so ``load`` / ``save`` / ``mean`` / ``cov`` need no device) and on
    ``device`` from then on, as one f64 buffer [D + D*D] = (sum, gram)."""

    chunk = MOMENTS_MAX_N   # samples per dhw_moments_update call (at most MOMENTS_MAX_N)

    def __init__(self, D: int = 1280, device=None):
        self.D = _check_D(D)
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
        if not _call.is_int(count) or count < 0:
            raise ValueError(f"count = {count!r} must be a non-negative integer")
        st = cls(s.shape[0], device)
        st.count = int(count)
        st._host[:st.D], st._host[st.D:] = s, g.reshape(-1)
        return st

    # ------------------------------------------------------------ accumulation (GPU)
    def update(self, features) -> "FeatureStats":
        """Add ``features``, [N,S,D] (pooled over S) or [N,D], a tensor on any device or an array."""
        import torch

        x, N, S = _check_features(features, self.D)
        if N == 0:
            return self
        with _call.open("FeatureStats.update", like=x, device=self.device, record=True) as c:   # (record: x may be the caller's own)
            if self._dev is None:
                self.device = c.dev
                self._dev = torch.from_numpy(self._host).to(c.dev)
                self._host = None
            D = self.D
            step = max(1, min(int(self.chunk), MOMENTS_MAX_N, (2 ** 31 - 1) // (S * D)))
            x = c.to(x.detach())
            for lo in range(0, N, step):
                n = min(step, N - lo)
                ws, need = c.workspace("moments", "dhw_moments_workspace_bytes", n, S, D)
                c.run("dhw_moments_update", x[lo:lo + n].data_ptr(), n, S, D, self._dev.data_ptr(), self._dev[D:].data_ptr(), c.ptr(ws), need)
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


# ---------------------------------------------------------------- sets of pooled vectors and their pairwise statistics (§38)
class FeatureSet:
    """The pooled D-dimensional feature vectors themselves, at most 16384 rows, in float64 on the GPU.

    Rows read by ``load`` / ``from_rows`` stay on the host until a device is needed (``update`` or one of the pairwise functions),
    so ``load`` / ``save`` / ``count`` / ``data`` need no device."""

    def __init__(self, D: int = 1280, device=None):
        self.D = _check_D(D)
        self.device = device
        self.count = 0
        self._host = np.zeros((0, self.D), np.float64)
        self._dev = None   # f64 [capacity, D], the first `count` rows in use

    @classmethod
    def from_rows(cls, rows, device=None) -> "FeatureSet":
        """A set from pooled rows f64 [N,D] (what ``save`` writes)."""
        r = np.ascontiguousarray(rows, np.float64)
        if r.ndim != 2:
            raise ValueError(f"rows must be [N, D], got {r.shape}")
        if r.shape[0] > PAIRS_MAX_N:
            raise ValueError(f"a FeatureSet holds at most {PAIRS_MAX_N} rows (got {r.shape[0]})")
        if not np.isfinite(r).all():
            raise ValueError("rows hold a non-finite value")
        st = cls(r.shape[1], device)
        st._host, st.count = r.copy(), int(r.shape[0])
        return st

    def _on_device(self):
        """The device buffer, created from the host rows at the first need of a device."""
        if self._dev is None:
            import torch

            self.device = _call.pick_device("FeatureSet", device=self.device)
            self._dev = torch.empty((max(256, self.count), self.D), dtype=torch.float64, device=self.device)
            self._dev[:self.count] = torch.from_numpy(self._host)
            self._host = None
        return self._dev

    def _reserve(self, rows: int):
        import torch

        buf = self._on_device()
        if buf.shape[0] < rows:
            cap = buf.shape[0]
            while cap < rows:
                cap *= 2
            new = torch.empty((min(cap, PAIRS_MAX_N), self.D), dtype=torch.float64, device=self.device)
            new[:self.count] = buf[:self.count]
            self._dev = new
        return self._dev

    def update(self, features) -> "FeatureSet":
        """Append ``features``, [N,S,D] (pooled over S as ``FeatureStats.update`` pools) or [N,D], a tensor on any device or an array."""
        import torch

        x, N, S = _check_features(features, self.D)
        if N == 0:
            return self
        if self.count + N > PAIRS_MAX_N:
            raise ValueError(f"a FeatureSet holds at most {PAIRS_MAX_N} rows (holds {self.count}, got {N} more)")
        x = x.detach().to(torch.float32)
        if not x.is_cuda and not bool(torch.isfinite(x).all()):
            raise ValueError("features hold a non-finite value (NaN or infinite)")
        with _call.open("FeatureSet.update", like=x, device=self.device, record=True) as c:   # (record: x may be the caller's own)
            if self._dev is None:
                self.device = c.dev
                self._on_device()
            given_on_device, D = x.is_cuda, self.D
            step = max(1, min(MOMENTS_MAX_N, (2 ** 31 - 1) // (S * D)))
            x = c.to(x)
            if given_on_device and not bool(torch.isfinite(x).all()):
                raise ValueError("features hold a non-finite value (NaN or infinite)")
            buf = self._reserve(self.count + N)
            for lo in range(0, N, step):
                n = min(step, N - lo)
                c.run("dhw_pairs_pool", x[lo:lo + n].data_ptr(), n, S, D, buf[self.count + lo:].data_ptr())
        self.count += N
        return self

    @property
    def data(self):
        """The rows, a float64 tensor [count, D]: on the device once one was needed, else on the host."""
        import torch

        return torch.from_numpy(self._host) if self._dev is None else self._dev[:self.count]

    def rows(self) -> np.ndarray:
        return self._host.copy() if self._dev is None else self._dev[:self.count].cpu().numpy()

    def save(self, path) -> None:
        with open(path, "wb") as f:
            np.savez(f, rows=self.rows())

    @classmethod
    def load(cls, path, device=None) -> "FeatureSet":
        with np.load(path) as z:
            return cls.from_rows(z["rows"], device)


def _check_k(k, rows: int):
    if not _call.is_int(k) or not 1 <= k <= PAIRS_MAX_K:
        raise ValueError(f"k = {k!r} must be an integer in [1, {PAIRS_MAX_K}]")
    if k >= rows:
        raise ValueError(f"k = {k} needs more than {k} rows in the set (it holds {rows})")


def _check_sets(*sets, least: int = 1):
    for s in sets:
        if not isinstance(s, FeatureSet):
            raise ValueError(f"expected a FeatureSet, got {type(s).__name__}")
        if s.count < least:
            raise ValueError(f"a FeatureSet holds {s.count} rows, fewer than {least}")
    if len({s.D for s in sets}) != 1:
        raise ValueError(f"the sets have different dimensions: {', '.join(str(s.D) for s in sets)}")


def _pairs(first, *others):
    """(device, rows of every set on that device): the sets are brought to the first one's device.  The pairwise entries share
    one cached workspace per device: calls on one device must be ordered on one stream."""
    import torch

    x = first._on_device()[:first.count]
    dev = first.device
    rows = [x]
    for s in others:
        if s._dev is None and s.device is None:
            s.device = dev
        r = s._on_device()[:s.count]
        if s.device != dev:
            raise ValueError(f"the sets live on different devices: {dev} and {s.device}")
        rows.append(r)
    assert all(r.is_contiguous() and r.dtype == torch.float64 for r in rows)
    return dev, rows


def knn_radius(s: FeatureSet, k: int = 3):
    """Squared distance of every row to its k-th nearest other row of the same set: a float64 device tensor [count].  The row
    itself is left out by index, so a duplicated row has radius 0 at k = 1."""
    import torch

    _check_sets(s)
    _check_k(k, s.count)
    dev, (x,) = _pairs(s)
    N, D = s.count, s.D
    with _call.open("FeatureSet", device=dev) as c:
        out = c.empty(N, torch.float64)
        ws, need = c.workspace("pairs", "dhw_pairs_workspace_bytes", N, N, D)
        c.run("dhw_pairs_knn", x.data_ptr(), N, D, int(k), out.data_ptr(), c.ptr(ws), need)
    return out


def _cover(queries: FeatureSet, ref: FeatureSet, radius2=None):
    """(count [M] int32 or None, nearest2 [M] float64, nearest_idx [M] int32) of dhw_pairs_cover, device tensors."""
    import torch

    dev, (q, r) = _pairs(queries, ref)
    M, N, D = queries.count, ref.count, ref.D
    with _call.open("FeatureSet", device=dev) as c:
        near, idx = c.empty(M, torch.float64), c.empty(M, torch.int32)
        count = c.empty(M, torch.int32, wanted=radius2 is not None)
        ws, need = c.workspace("pairs", "dhw_pairs_workspace_bytes", M, N, D)
        c.run("dhw_pairs_cover", q.data_ptr(), M, r.data_ptr(), N, D, c.ptr(radius2), c.ptr(count), near.data_ptr(), idx.data_ptr(), c.ptr(ws), need)
    return count, near, idx


def nearest(queries: FeatureSet, ref: FeatureSet):
    """For every row of ``queries`` the nearest row of ``ref``: (squared distance float64 [M], index int32 [M]; the smallest index
    on a tie), device tensors.  A distance of 0 to a training line is a copy of it."""
    _check_sets(queries, ref)
    _, near, idx = _cover(queries, ref)
    return near, idx


def precision_recall(real: FeatureSet, gen: FeatureSet, k: int = 3) -> dict:
    """{"precision", "recall", "density", "coverage"} of the generated set against the real one with k-nearest-neighbour balls
    (Kynkäänniemi et al. 2019; Naeem et al. 2020): precision = the share of generated rows inside some real row's ball, density =
    the mean number of real balls a generated row lies in, over k; recall = precision with the roles swapped; coverage = the share
    of real rows whose nearest generated row lies inside their own ball."""
    _check_sets(real, gen)
    _check_k(k, real.count)
    _check_k(k, gen.count)
    r_real, r_gen = knn_radius(real, k), knn_radius(gen, k)
    in_real, _, _ = _cover(gen, real, r_real)
    in_gen, near_gen, _ = _cover(real, gen, r_gen)
    m, n = real.count, gen.count   # (integer counts over integer sizes: one rounding per number)
    return {"precision": int((in_real > 0).sum()) / n, "recall": int((in_gen > 0).sum()) / m, "density": int(in_real.sum()) / (k * n),
            "coverage": int((near_gen <= r_real).sum()) / m}


def _polysum(x: FeatureSet, y: FeatureSet, skip_diag: bool) -> float:
    import torch

    dev, (a, b) = _pairs(x, y)
    with _call.open("FeatureSet", device=dev) as c:
        out = c.empty(2, torch.float64)
        ws, need = c.workspace("pairs", "dhw_pairs_workspace_bytes", x.count, y.count, x.D)
        c.run("dhw_pairs_polysum", a.data_ptr(), x.count, b.data_ptr(), y.count, x.D, int(skip_diag), out.data_ptr(), c.ptr(ws), need)
        return float(out[0])


def kernel_distance(real: FeatureSet, gen: FeatureSet) -> float:
    """The kernel distance (KID): the unbiased estimate of MMD^2 with k(x, y) = (x.y / D + 1)^3,
    sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (n (n - 1)) - 2 sum_{i, j} k(x_i, y_j) / (m n).
    Unbiased at any set size (it can be slightly negative) and free of eigen-decompositions."""
    _check_sets(real, gen, least=2)
    m, n, d3 = real.count, gen.count, float(real.D) ** 3
    xx, yy, xy = _polysum(real, real, True), _polysum(gen, gen, True), _polysum(real, gen, False)
    return (xx / (m * (m - 1)) + yy / (n * (n - 1)) - 2.0 * xy / (m * n)) / d3


def line_features(strokes, extractor, lengths=None, batch: int = 32):
    """Strokes [N,L,3] -> style features [N,14,1280] on the device: ``render_strokes`` then ``extractor``, ``batch`` lines at a time."""
    import torch

    from .vis import render_strokes
    if not _call.is_int(batch) or batch < 1:
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
_DDIM_KW = {"T", "steps", "levels", "guidance", "order"}


def _sampler_of(sampler: dict, who: str = "sample_quality"):
    """Which sampler the keywords select: ``sample_ddim`` when steps / levels is among them, else ``sample``; TypeError for a
    keyword that sampler does not take."""
    ddim = "steps" in sampler or "levels" in sampler
    unknown = sorted(set(sampler) - (_DDIM_KW if ddim else _SAMPLE_KW))
    if unknown:
        raise TypeError(f"{who}: unknown sampler keyword(s) {', '.join(unknown)} for {'sample_ddim' if ddim else 'sample'} "
                        f"(known: {', '.join(sorted(_DDIM_KW if ddim else _SAMPLE_KW))})")
    return ddim


def _evaluate(who, model, data, extractor, n, batch, seed, real, real_set, with_sets, timings, sampler, keep=None):
    """The one loop behind ``sample_quality`` and ``sample_metrics``: the first ``n`` rows of ``data``, ``batch`` at a time, real
    lines rendered and generated lines drawn with ``first_sample`` = the row index; every batch of features feeds a
    ``FeatureStats`` and, ``with_sets``, a ``FeatureSet``.  ``real`` / ``real_set``: given statistics / rows of the real lines
    (None: computed).  ``keep`` (a list): the generated strokes of every batch are appended to it.  Returns (fd, real, gen,
    real_set, gen_set)."""
    ddim = _sampler_of(sampler, who)
    for k in ("strokes", "text", "style"):
        if k not in data:
            raise ValueError(f"data must hold 'strokes', 'text' and 'style' (missing {k!r})")
    if not _call.is_int(batch) or batch < 1:
        raise ValueError(f"batch = {batch!r} must be a positive integer")
    total = int(data["strokes"].shape[0])
    n = total if n is None else n
    if not _call.is_int(n) or not 2 <= n <= total:
        raise ValueError(f"n = {n!r} must be an integer in [2, {total}] (the rows of data)")
    if real is not None and not isinstance(real, FeatureStats):
        raise ValueError("real must be a FeatureStats")
    if with_sets:
        if n > PAIRS_MAX_N:
            raise ValueError(f"n = {n} lines: a FeatureSet holds at most {PAIRS_MAX_N}")
        if real_set is not None and not isinstance(real_set, FeatureSet):
            raise ValueError("real must be a FeatureSet or a (FeatureStats, FeatureSet) pair")
    import torch

    from .inference import sample, sample_ddim
    dev = extractor.device
    L = int(data["strokes"].shape[1])
    t = dict(sample=0.0, features=0.0, moments=0.0, eig=0.0)

    def tick():
        if timings is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    if with_sets and real_set is not None and real is None:   # statistics of the given rows
        rows = real_set.rows()                                # (on the host in float64: update() would round the rows to float32)
        real = FeatureStats.from_state(real_set.count, rows.sum(0), rows.T @ rows, dev)
    fill_real, fill_set = real is None, with_sets and real_set is None
    if fill_real:
        real = FeatureStats(1280, dev)
    if fill_set:
        real_set = FeatureSet(1280, dev)
    if fill_real or fill_set:
        for lo in range(0, n, batch):
            t0 = tick()
            f = line_features(torch.as_tensor(data["strokes"][lo:min(lo + batch, n)]), extractor, batch=batch)
            t1 = tick()
            if fill_real:
                real.update(f)
            if fill_set:
                real_set.update(f)
            t2 = tick()
            t["features"], t["moments"] = t["features"] + t1 - t0, t["moments"] + t2 - t1
    gen = FeatureStats(1280, dev)
    gen_set = FeatureSet(1280, dev) if with_sets else None
    draw = sample_ddim if ddim else sample
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        t0 = tick()
        lines = draw(model, torch.as_tensor(data["text"][lo:hi]).to(dev), torch.as_tensor(data["style"][lo:hi]).to(dev), L=L, seed=seed,
                     first_sample=lo, **sampler)
        t1 = tick()
        if keep is not None:
            keep.append(lines)
        f = line_features(lines, extractor, batch=batch)
        t2 = tick()
        gen.update(f)
        if with_sets:
            gen_set.update(f)
        t3 = tick()
        t["sample"], t["features"], t["moments"] = t["sample"] + t1 - t0, t["features"] + t2 - t1, t["moments"] + t3 - t2
    t0 = time.perf_counter()
    fd = frechet_distance(real, gen)
    t["eig"] = time.perf_counter() - t0
    if timings is not None:
        timings.update(t)
    return fd, real, gen, real_set, gen_set


def sample_quality(model, data, extractor, n=None, batch: int = 32, seed: int = 0, real=None, timings=None, **sampler):
    """Fréchet distance between the lines of a data set and lines the model samples for the same rows.

    ``data``: the dict ``train.py --val`` reads, {"strokes" [N,L,3], "text" [N,Lt], "style" [N,S,1280]}.  The first ``n`` rows
    (default all) are used.  Real statistics come from ``data["strokes"]``, or from ``real`` (a ``FeatureStats``, e.g. loaded from
    a file) when given.  Generated lines come from ``sample`` (keywords T, diffusion_mode, guidance), or from ``sample_ddim`` when
    ``steps=`` or ``levels=`` is among the keywords (then also ``order=``, its solver order), with the rows' text and style at L = data["strokes"].shape[1], ``batch`` rows
    per call and ``first_sample`` = the row index, so the result does not depend on ``batch``.  ``timings`` (a dict): filled with
    the seconds spent in sampling, rendering + features, moments and the host eigen-decompositions (synchronises per stage).
    Returns (fd, real_stats, generated_stats)."""
    return _evaluate("sample_quality", model, data, extractor, n, batch, seed, real, None, False, timings, sampler)[:3]


def sample_metrics(model, data, extractor, n=None, batch: int = 32, seed: int = 0, k: int = 3, real=None, timings=None, dtw: bool = False, **sampler):
    """``sample_quality`` with every metric: the same rows, sampler keywords and ``first_sample`` (one loop serves both), the
    features of each batch kept as statistics and as rows.  ``real``: a ``FeatureSet`` of the real lines (its statistics are
    computed from its rows) or a (``FeatureStats``, ``FeatureSet``) pair, used as given; None: both come from ``data["strokes"]``.
    At most 16384 lines.  Returns {"fd", "precision", "recall", "density", "coverage", "kid", "k", "n", "real_stats", "gen_stats",
    "real_set", "gen_set"}; "fd" is ``sample_quality``'s value, bit for bit.

    ``dtw=True`` also keeps the real and the generated strokes and adds the stroke-space distances of DESIGN.md §39 (normalised
    ``dtw_distance`` with its default features): "dtw_paired", the mean distance between generated row r and real row r;
    "dtw_nearest", the mean over generated rows of the distance to the nearest real line, with the index vector
    "dtw_nearest_idx" (a value near 0: the model copies that line); "dtw_self", the mean over generated rows of the distance to
    the nearest other generated line (a value near 0: the samples collapse onto one another).  Every other key is unchanged."""
    if not _call.is_int(k) or not 1 <= k <= PAIRS_MAX_K:
        raise ValueError(f"k = {k!r} must be an integer in [1, {PAIRS_MAX_K}]")
    stats, rows = real if isinstance(real, tuple) and len(real) == 2 else (None, real)
    if dtw and "strokes" in data:
        from .dtw import DTW_MAX_L
        if int(data["strokes"].shape[1]) > DTW_MAX_L:
            raise ValueError(f"dtw=True: lines of L = {int(data['strokes'].shape[1])} rows: at most {DTW_MAX_L}")
    kept = [] if dtw else None
    fd, real_stats, gen_stats, real_set, gen_set = _evaluate("sample_metrics", model, data, extractor, n, batch, seed, stats, rows, True, timings,
                                                             sampler, kept)
    out = {"fd": fd, **precision_recall(real_set, gen_set, k), "kid": kernel_distance(real_set, gen_set), "k": int(k), "n": gen_set.count,
           "real_stats": real_stats, "gen_stats": gen_stats, "real_set": real_set, "gen_set": gen_set}
    if dtw:
        out.update(_dtw_metrics(kept, data["strokes"], gen_set.count, batch))
    return out


def _dtw_metrics(kept, real_strokes, n: int, batch: int) -> dict:
    """The stroke-space keys of ``sample_metrics``: generated strokes `kept` (one tensor per batch) against the first n real lines.
    The paired distances are the diagonal of the generated x real matrix, computed in diagonal blocks of `batch` lines (a pair's
    bits do not depend on the block it is computed in)."""
    import torch

    from .dtw import dtw_distance, nearest_strokes
    gen = torch.cat(kept) if len(kept) != 1 else kept[0]
    real = torch.as_tensor(real_strokes[:n]).to(gen.device)
    paired = torch.cat([dtw_distance(gen[lo:lo + batch], real[lo:lo + batch])[0].diagonal() for lo in range(0, n, batch)])
    near, idx = nearest_strokes(gen, real)
    self_near, _ = nearest_strokes(gen)
    mean = lambda t: float(t.cpu().numpy().astype(np.float64).mean())   # noqa: E731
    return {"dtw_paired": mean(paired), "dtw_nearest": mean(near), "dtw_nearest_idx": idx, "dtw_self": mean(self_near)}
