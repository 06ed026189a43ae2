"""The batch draw of a training update, stated in numpy (include/dhw_train.h dhw_train_batch_draw): Philox4x32-10 on Python
integers, then the mappings of its four output words in np.float32 — one correctly rounded operation at a time, which is what
the kernel's unfused fp32 arithmetic computes, so the floats are comparable bit for bit."""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words -> 4 words (Random123's Philox4x32 with 10 rounds; the key is bumped after every round)."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, index, N, B, abar, tables=None):
    """-> (idx int64 [B], style_src int64 [B], alphas f32 [B], sigma f32 [B], interval int64 [B]) of draw number ``index``.
    abar: the schedule's cumulative products [T]; tables: (grp_start, grp_size, grp_pos, members) or None."""
    abar = np.asarray(abar, np.float32)
    T = len(abar)
    idx, src, iv = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    alphas, sigma = np.zeros(B, np.float32), np.zeros(B, np.float32)
    for b in range(B):
        stream = (int(index) * B + b) & 0xFFFFFFFFFFFFFFFF
        w0, w1, w2, w3 = philox4x32_10((stream & M32, stream >> 32, 0, 0), (int(seed) & M32, (int(seed) >> 32) & M32))
        n = (w0 * N) >> 32
        i = (w1 * (T - 1)) >> 32
        u = (np.float32(w2 >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
        a = np.float32(np.float32(u * np.float32(abar[i + 1] - abar[i])) + abar[i])
        s = n
        if tables is not None:
            start, size, pos, members = tables
            g = int(size[n])
            if g > 1:
                r = (w3 * (g - 1)) >> 32
                s = int(members[int(start[n]) + r + (1 if r >= int(pos[n]) else 0)])
        idx[b], src[b], iv[b], alphas[b], sigma[b] = n, s, i, a, np.sqrt(a)
    return idx, src, alphas, sigma, iv
