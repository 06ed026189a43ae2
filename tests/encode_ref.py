"""CPU statement of the stroke encoder's rules (include/dhw.h dhw_encode, rules 1-9) in float64 numpy, written from the rules.
The merge order is the stable (v, j) order of rule 4."""
import numpy as np


def final_rows(n: int, rounds: int) -> int:
    """Rule 5: the row count after `rounds` rounds, a function of n and rounds alone."""
    M = n - 1
    for _ in range(rounds):
        M -= M // 5
    return M


def _normalise(d):
    """Rule 3; False when the std is 0 or not finite (nothing is divided then)."""
    v = d.reshape(-1)
    mean = v.sum() / v.size
    s = np.sqrt(((v - mean) ** 2).sum() / v.size)
    if not (s > 0) or not np.isfinite(s):
        return False
    d /= s
    return True


def pair_keys(d):
    """v_j of rule 4 for the pairs (2j, 2j+1), j < M // 2."""
    P = len(d) // 2
    a, b = d[0:2 * P:2], d[1:2 * P:2]
    norm = lambda x: np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
    return norm(a) + norm(b) - norm(a + b)


def encode_rows(points, rounds: int = 3, gaps=None):
    """Rules 1-4 on one line's n >= 2 points [n,3]: (rows float64 [M,3] = (dx, dy, pen), ok).  ok False is status bit 2: the
    rows then only have the right count.  `gaps` (a list) receives, per round, (v_(k+1) - v_(k) in sorted order or inf,
    the number of exact-zero v, k)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(p)
    M = n - 1
    d = np.stack([p[1:, 0] - p[:-1, 0], -(p[1:, 1] - p[:-1, 1])], axis=1)
    pen = np.roll((p[1:, 2] != 0).astype(np.float64), 1)
    ok = bool(np.isfinite(p).all()) and _normalise(d)
    for _ in range(rounds):
        k = M // 5
        if not ok:
            M -= k
            continue
        v = pair_keys(d)
        order = np.lexsort((np.arange(len(v)), v))   # by v, then by j
        if gaps is not None:
            sv = v[order]
            gaps.append((float(sv[k] - sv[k - 1]) if 0 < k < len(sv) else float("inf"), int((v == 0).sum()), k))
        ind = order[:k]
        d[2 * ind] += d[2 * ind + 1]
        pen[2 * ind] = (pen[2 * ind] + pen[2 * ind + 1] > 0)
        d = np.delete(d, 2 * ind + 1, axis=0)
        pen = np.delete(pen, 2 * ind + 1)
        M -= k
        ok = _normalise(d)
    if not ok:
        return np.zeros((M, 3)), False
    return np.concatenate([d, pen[:, None]], axis=1), True


def encode_ref(points, n=None, N=None, L: int = 480, rounds: int = 3, max_abs: float = 15.0):
    """One line by rules 1-9: (strokes float32 [L,3], length, status).  n defaults to len(points), N to n."""
    points = np.asarray(points)
    n = len(points) if n is None else int(n)
    N = n if N is None else N
    pad = np.zeros((L, 3), np.float32)
    pad[:, 2] = 1
    if n < 2 or n > N:
        return pad, 0, 1
    rows, ok = encode_rows(points[:n], rounds)
    M = len(rows)
    assert M == final_rows(n, rounds)
    status = 0 if ok else 2
    if M > L:
        status |= 4
    if ok and np.abs(rows[:, :2]).max() > np.float64(np.float32(max_abs)):
        status |= 8
    if status == 0:
        pad[:M] = rows.astype(np.float32)
    return pad, M, status


def encode_batch_ref(lines, L: int, rounds: int = 3, max_abs: float = 15.0):
    out = [encode_ref(p, L=L, rounds=rounds, max_abs=max_abs) for p in lines]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int32)
