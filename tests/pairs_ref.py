"""The numpy float64 statements of dhw_pairs_* (include/dhw.h) and of dhg_amd.precision_recall / kernel_distance,
for the tests of both.  Distances are taken in the direct form sum (x - y)^2, not the expanded form the kernel uses."""
import numpy as np

U = 2.0 ** -53   # unit roundoff of float64


def pool(feat):
    """feat f32 [N,S,D] -> p f64 [N,D] = (sum_s (double)feat[n][s][d]) / S, s ascending."""
    f = np.asarray(feat)
    assert f.ndim == 3
    acc = f[:, 0].astype(np.float64)
    for s in range(1, f.shape[1]):
        acc = acc + f[:, s].astype(np.float64)
    return acc / np.float64(f.shape[1])


def d2(x, y):
    """[M,N] squared distances, direct form, row by row (no M x N x D array)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    for i in range(x.shape[0]):
        diff = y - x[i]
        out[i] = (diff * diff).sum(1)
    return out


def radius(x, k):
    """radius2[i] = the k-th smallest of { d2(x_i, x_j) : j != i }, j excluded by index."""
    d = d2(x, x)
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, k - 1]


def cover(q, ref, radius2=None):
    """(count [M] or None, nearest2 [M], nearest_idx [M]: the smallest index attaining the minimum)."""
    d = d2(q, ref)
    count = None if radius2 is None else (d <= np.asarray(radius2)[None, :]).sum(1).astype(np.int32)
    return count, d.min(1), d.argmin(1).astype(np.int32)


def polysum(x, y, skip_diag=False):
    """sum_{i,j} (x_i . y_j + D)^3, without i == j when skip_diag."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    t = x @ y.T + x.shape[1]
    c = t * t * t
    if skip_diag:
        assert x.shape[0] == y.shape[0]
        np.fill_diagonal(c, 0.0)
    return float(c.sum())


def polysum_bound(x, y):
    """(3 D + M N + 16) 2^-53 sum_ij (sum_d |x_id y_jd| + D)^3: a D-term inner product, cubed (three times its relative error), and
    an M N-term sum in any order."""
    x, y = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(y, np.float64))
    M, N, D = x.shape[0], y.shape[0], x.shape[1]
    t = x @ y.T + D
    return (3 * D + M * N + 16) * U * float((t * t * t).sum())


def pair_bound(x, y):
    """b_ij = (D + 8) 2^-53 . 2 (sq_i + sq_j), [M,N]: the expanded form's error against the direct form."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    sx, sy = (x * x).sum(1), (y * y).sum(1)
    return (x.shape[1] + 8) * U * 2.0 * (sx[:, None] + sy[None, :])


def metrics(real, gen, k):
    """precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) with k-NN balls."""
    r_real, r_gen = radius(real, k), radius(gen, k)
    in_real, _, _ = cover(gen, real, r_real)
    in_gen, near_gen, _ = cover(real, gen, r_gen)
    m, n = len(real), len(gen)
    return {"precision": int((in_real > 0).sum()) / n, "recall": int((in_gen > 0).sum()) / m, "density": int(in_real.sum()) / (k * n),
            "coverage": int((near_gen <= r_real).sum()) / m}


def kid(real, gen):
    """Unbiased MMD^2 with k(x, y) = (x . y / D + 1)^3."""
    real, gen = np.asarray(real, np.float64), np.asarray(gen, np.float64)
    m, n, D = real.shape[0], gen.shape[0], real.shape[1]
    def cube(a, b):
        t = a @ b.T / D + 1
        return t * t * t

    kxx, kyy, kxy = cube(real, real), cube(gen, gen), cube(real, gen)
    return float((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (n * (n - 1)) - 2 * kxy.sum() / (m * n))
