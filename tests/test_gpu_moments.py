"""Feature moments on the GPU (include/dhw.h dhw_moments_update, dhg_amd.FeatureStats) against tests/moments_ref.py.

Exact data: features are small integers in [-7, 7] with S in {1, 2}, so every pooled value is a multiple of 1/2, every product
a multiple of 1/4 below 2^6 and every sum far below 2^53: sum and gram are exactly representable at every step, in any order,
and must equal the int64 result bit for bit.  The columns are drawn from different ranges (no p[n][i] == p[n][j] pattern, no
symmetric operand), so a swapped row / column map of the matrix instruction, or the f32 form's row formula, cannot pass.

Real-valued data, bound derived and not measured: gram[i][j] is an N-term recursive sum of (fused) products of pooled values,
each pooled value an S-term sum, one division and S exact conversions, so |gram - ref| <= (N + S + 4) 2^-53 sum_n |p_ni| |p_nj|
elementwise (Higham, Accuracy and Stability, §3.1 with gamma_k ~ k u), likewise |sum - ref| <= (N + S + 4) 2^-53 sum_n |p_ni|."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, quality

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moments_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 32            # canary doubles on each side of sum, gram and the workspace
CANARY = -1234.5
EXTRA_ROWS = 3        # NaN rows behind row N of feat: never read


def int_features(N, S, D, seed):
    """Integers in [-7, 7], column d drawn from [-(d % 8), (5 d + 3) % 8]: every column has its own range."""
    g = np.random.Generator(np.random.PCG64([seed, N, S, D]))
    d = np.arange(D)
    return g.integers(-(d % 8), (5 * d + 3) % 8 + 1, size=(N, S, D)).astype(np.float32)


def real_features(N, S, D, seed):
    g = np.random.Generator(np.random.PCG64([seed, N, S, D]))
    return np.clip(g.normal(1.5, 1.5, size=(N, S, D)), 0, 6).astype(np.float32)


def raw_update(feat, state=None, calls=1):
    """dhw_moments_update on feat [N,S,D] (host) from `state` = (sum, gram) or zeros; sum, gram and the workspace lie in one
    buffer between canaries, feat has NaN rows behind row N.  Returns (sum, gram) as numpy after checking the canaries."""
    N, S, D = feat.shape
    l = _lib.lib()
    need = int(l.dhw_moments_workspace_bytes(N, S, D))
    assert need == N * D * 8
    sizes = [D, D * D, N * D]
    offs, o = [], GUARD
    for n in sizes:
        offs.append(o)
        o += n + GUARD
    host = np.full(o, CANARY)
    host[offs[0]:offs[0] + D] = 0 if state is None else state[0]
    host[offs[1]:offs[1] + D * D] = 0 if state is None else np.asarray(state[1]).reshape(-1)
    buf = torch.from_numpy(host).cuda()
    padded = np.full((N + EXTRA_ROWS, S, D), np.nan, np.float32)
    padded[:N] = feat
    x = torch.from_numpy(padded).cuda()
    for _ in range(calls):
        _lib.check(l.dhw_moments_update(x.data_ptr(), N, S, D, buf[offs[0]:].data_ptr(), buf[offs[1]:].data_ptr(), buf[offs[2]:].data_ptr(), need,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    keep = np.ones(o, bool)
    for off, n in zip(offs, sizes):
        keep[off:off + n] = False
    assert (out[keep] == CANARY).all(), "a canary next to sum, gram or the workspace was overwritten"
    assert np.array_equal(out[offs[2]:offs[2] + N * D].reshape(N, D), moments_ref.pool(feat))   # the pooled matrix, bit for bit
    return out[offs[0]:offs[0] + D].copy(), out[offs[1]:offs[1] + D * D].reshape(D, D).copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def exact(feat):
    S = feat.shape[1]
    q, q2 = moments_ref.exact_update(feat, S)
    return q.astype(np.float64) / S, q2.astype(np.float64) / (S * S)


EXACT_CASES = [(N, S, 48) for N in (1, 3, 4, 5, 67) for S in (1, 2)] + [(2, 1, 16), (2, 2, 16), (37, 2, 1280)]


@pytest.mark.parametrize("N,S,D", EXACT_CASES)
def test_exact_data_bit_for_bit(N, S, D):
    feat = int_features(N, S, D, 1)
    s, g = raw_update(feat)
    ws, wg = exact(feat)
    assert same_bits(s, ws), np.argwhere(s != ws)[:8]
    assert same_bits(g, wg), np.argwhere(g != wg)[:8]
    assert same_bits(g, g.T)


def test_two_updates_equal_one_update_of_all_rows():
    feat = int_features(72, 2, 48, 2)
    first = raw_update(feat[:5])
    s2, g2 = raw_update(feat[5:], state=first)
    s1, g1 = raw_update(feat)
    assert same_bits(s1, s2) and same_bits(g1, g2) and same_bits(g2, g2.T)
    ws, wg = exact(feat)
    assert same_bits(s2, ws) and same_bits(g2, wg)


REAL = {}


def real_case(D):
    """Features, float64 reference and bounds of the real-valued case at D: computed once, shared, never changed."""
    if D not in REAL:
        feat = real_features(67, 14, D, 3)
        REAL[D] = (feat, moments_ref.update(feat), moments_ref.bounds(feat))
        for a in REAL[D][1] + REAL[D][2]:
            a.setflags(write=False)
    return REAL[D]


def worst(got, ref, bound):
    return float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("D", [48, 1280])
def test_real_valued_data_within_the_derived_bound(D):
    feat, (rs, rg), (bs, bg) = real_case(D)
    assert feat.min() == 0 and feat.max() == 6 and (bs > 0).all() and (bg > 0).all()
    s, g = raw_update(feat)
    es, eg = worst(s, rs, bs), worst(g, rg, bg)
    print(f"D = {D}: largest error / bound: sum {es:.3e}, gram {eg:.3e}")
    assert es <= 1 and eg <= 1
    assert same_bits(g, g.T)
    s2, g2 = raw_update(feat)
    assert same_bits(s, s2) and same_bits(g, g2)          # the same call on the same state: the same bits


def stats_state(st):
    s, g = st._state()
    return s.copy(), g.copy()


def test_feature_stats_takes_pooled_and_unpooled_inputs():
    feat = real_features(21, 1, 48, 4)
    a = dhg_amd.FeatureStats(48).update(torch.from_numpy(feat[:, 0]))          # [N,D], from the host
    b = dhg_amd.FeatureStats(48).update(torch.from_numpy(feat).cuda())         # [N,1,D], on the device
    assert a.count == b.count == 21 and a.device.type == "cuda"
    for x, y in zip(stats_state(a), stats_state(b)):
        assert same_bits(x, y)
    s, g = raw_update(feat)
    assert same_bits(stats_state(a)[0], s) and same_bits(stats_state(a)[1], g)
    m, c = moments_ref.mean_cov(feat[:, 0])
    assert np.abs(a.mean() - m).max() <= 1e-12 * np.abs(m).max() and np.abs(a.cov() - c).max() <= 1e-12 * np.abs(c).max()
    with pytest.raises(ValueError, match="non-finite"):
        dhg_amd.FeatureStats(48).update(np.full((2, 48), np.nan, np.float32)).cov()


def test_feature_stats_in_chunks(monkeypatch):
    monkeypatch.setattr(quality.FeatureStats, "chunk", 5)
    feat = int_features(67, 2, 48, 5)
    st = dhg_amd.FeatureStats(48)
    st.update(feat[:30]).update(feat[30:])
    ws, wg = exact(feat)
    s, g = stats_state(st)
    assert st.count == 67 and same_bits(s, ws) and same_bits(g, wg) and same_bits(g, g.T)
    feat, (rs, rg), (bs, bg) = real_case(48)
    s, g = stats_state(dhg_amd.FeatureStats(48).update(feat))
    es, eg = worst(s, rs, bs), worst(g, rg, bg)
    print(f"chunks of 5: largest error / bound: sum {es:.3e}, gram {eg:.3e}")
    assert es <= 1 and eg <= 1 and same_bits(g, g.T)
