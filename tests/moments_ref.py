"""The numpy float64 statement of dhw_moments_update (include/dhw.h) and of dhg_amd.frechet_distance, for the
tests of both."""
import numpy as np

U = 2.0 ** -53   # unit roundoff of float64


def pool(feat):
    """feat f32 [N,S,D] -> p f64 [N,D] = (sum_s (double)feat[n][s][d]) / S, s ascending from feat[n][0][d]."""
    f = np.asarray(feat)
    assert f.ndim == 3
    acc = f[:, 0].astype(np.float64)
    for s in range(1, f.shape[1]):
        acc = acc + f[:, s].astype(np.float64)
    return acc / np.float64(f.shape[1])


def update(feat, sum=None, gram=None):
    """(sum [D], gram [D,D]) after one update of the given state (zeros when None) with feat [N,S,D], n ascending."""
    p = pool(feat)
    D = p.shape[1]
    s = np.zeros(D) if sum is None else np.array(sum, np.float64)
    g = np.zeros((D, D)) if gram is None else np.array(gram, np.float64)
    for n in range(p.shape[0]):
        s += p[n]
        g += np.outer(p[n], p[n])
    return s, g


def bounds(feat):
    """The elementwise error bounds of one update from a zero state: (N + S + 4) 2^-53 sum_n |p_ni| (sum) and (N + S + 4) 2^-53
    sum_n |p_ni| |p_nj| (gram): an n-term recursive sum of (fused) products, the S-term pooling sum, its division and the
    conversions."""
    N, S, _ = np.asarray(feat).shape
    a = np.abs(pool(feat))
    return (N + S + 4) * U * a.sum(0), (N + S + 4) * U * (a.T @ a)


def exact_update(feat_int, S):
    """Exact int64 (sum S, gram S^2) numerators of small-integer features [N,S,D]: sum = q / S and gram = q2 / S^2 exactly when
    S is a power of two."""
    f = np.asarray(feat_int).astype(np.int64)
    q = f.sum(1)
    return q.sum(0), q.T @ q


def mean_cov(x):
    """np.mean / unbiased np.cov of samples x [N,D] in float64."""
    x = np.asarray(x, np.float64)
    return x.mean(0), np.cov(x, rowvar=False)


def frechet_distance(ma, ca, mb, cb):
    """|ma - mb|^2 + tr ca + tr cb - 2 sum_k sqrt(max(lambda_k, 0)), lambda = eigvalsh(sym(ca^1/2 cb ca^1/2)), ca^1/2 from eigh
    with the eigenvalues clipped at 0."""
    w, v = np.linalg.eigh((ca + ca.T) / 2)
    root = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    m = root @ ((cb + cb.T) / 2) @ root
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    d = ma - mb
    return float(d @ d + np.trace(ca) + np.trace(cb) - 2 * np.sqrt(np.clip(lam, 0, None)).sum())
