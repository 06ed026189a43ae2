"""The numpy float32 statement of dhw_dtw's pair rules (include/dhw.h), twice: `dtw_loop`, a plain double loop,
and `dtw_diag`, the same cells one anti-diagonal at a time (fast enough for 1024 x 1024), for the tests of the entry and of
dhg_amd.stroke_features / dtw_distance / nearest_strokes.  Every operation is one float32 operation in the rules' order."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)
ORDER = ("diag", "up", "left")   # rule 5: the first of these that attains the minimum is the predecessor


def cost(x, y):
    """c = sum_f (x_f - y_f)^2 over the last axis: difference, product and sum over f ascending, each rounded to float32."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    d = x[..., 0] - y[..., 0]
    c = d * d
    for f in range(1, x.shape[-1]):
        d = x[..., f] - y[..., f]
        c = c + d * d
    return c


def dtw_loop(a, b, order=ORDER):
    """(D(n-1,m-1) float32, K(n-1,m-1) int) of a [n,F] against b [m,F] by rules 2 to 6; `order`: the tie order of rule 5."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    n, m = a.shape[0], b.shape[0]
    D = np.full((n, m), INF, F32)
    K = np.zeros((n, m), np.int32)
    for i in range(n):
        for j in range(m):
            c = cost(a[i], b[j])
            if i == 0 and j == 0:
                D[0, 0], K[0, 0] = c, 1
                continue
            pred = {}
            if i > 0 and j > 0:
                pred["diag"] = (D[i - 1, j - 1], K[i - 1, j - 1])
            if i > 0:
                pred["up"] = (D[i - 1, j], K[i - 1, j])
            if j > 0:
                pred["left"] = (D[i, j - 1], K[i, j - 1])
            best = None
            for name in order:
                if name in pred and (best is None or pred[name][0] < best[0]):
                    best = pred[name]
            D[i, j], K[i, j] = F32(c + best[0]), best[1] + 1
    return D[n - 1, m - 1], int(K[n - 1, m - 1])


def dtw_diag(a, b):
    """The same result with the cells of one anti-diagonal d = i + j computed at once; a predecessor that does not exist is
    (+inf, 0), which never wins against one that does while the values are finite."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    n, m = a.shape[0], b.shape[0]
    # slot i + 1 holds row i, slot 0 is the row above the matrix
    d1, k1 = np.full(n + 1, INF, F32), np.zeros(n + 1, np.int32)   # the diagonal d - 1
    d2, k2 = d1.copy(), k1.copy()                                   # the diagonal d - 2
    d1[1], k1[1] = cost(a[0], b[0]), 1
    for d in range(1, n + m - 1):
        lo, hi = max(0, d - m + 1), min(n - 1, d)
        i = np.arange(lo, hi + 1)
        c = cost(a[i], b[d - i])
        best, kb = d2[i].copy(), k2[i].copy()          # diagonal: D(i-1, j-1)
        up, ku = d1[i], k1[i]                          # D(i-1, j)
        w = up < best
        best[w], kb[w] = up[w], ku[w]
        left, kl = d1[i + 1], k1[i + 1]                # D(i, j-1)
        w = left < best
        best[w], kb[w] = left[w], kl[w]
        nd, nk = np.full(n + 1, INF, F32), np.zeros(n + 1, np.int32)
        nd[i + 1], nk[i + 1] = c + best, kb + 1
        d2, k2, d1, k1 = d1, k1, nd, nk
    return d1[n], int(k1[n])


def dtw_batch(a, lens_a, b, lens_b, normalize=False, pair=dtw_diag):
    """(dist [M,N] float32, steps [M,N] int32) of a [M,La,F] against b [N,Lb,F]; lens None: the full length.  Rule 7: a length
    outside [1, L] gives +inf and 0.  Rule 6: the normalised distance is one float32 division."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    M, N = a.shape[0], b.shape[0]
    la = np.full(M, a.shape[1]) if lens_a is None else np.asarray(lens_a)
    lb = np.full(N, b.shape[1]) if lens_b is None else np.asarray(lens_b)
    dist, steps = np.full((M, N), INF, F32), np.zeros((M, N), np.int32)
    for p in range(M):
        for q in range(N):
            if 1 <= la[p] <= a.shape[1] and 1 <= lb[q] <= b.shape[1]:
                d, k = pair(a[p, :la[p]], b[q, :lb[q]])
                dist[p, q], steps[p, q] = (F32(d) / F32(k) if normalize else d), k
    return dist, steps


def nearest(dist, skip_diag=False):
    """Rule 8: (smallest dist over q [M] float32, smallest q attaining it [M] int32; +inf and -1 when no pair is finite)."""
    d = np.array(dist, F32)
    if skip_diag:
        np.fill_diagonal(d, INF)
    idx = d.argmin(1).astype(np.int32)
    best = d.min(1)
    idx[~np.isfinite(best)] = -1
    return best, idx


def features(strokes, kind="positions", pen_weight=1.0):
    """dhg_amd.stroke_features in numpy: (dx, dy) or pos[i] - pos[0] with float64 prefix sums rounded once, and
    sqrt(pen_weight) (rint(pen) != 0)."""
    s = np.asarray(strokes, F32)
    out = np.empty(s.shape, F32)
    if kind == "offsets":
        out[..., :2] = s[..., :2]
    else:
        pos = np.cumsum(s[..., :2].astype(np.float64), axis=-2)
        out[..., :2] = (pos - pos[..., :1, :]).astype(F32)
    out[..., 2] = F32(np.sqrt(np.float64(pen_weight))) * (np.rint(s[..., 2]) != 0).astype(F32)
    return out
