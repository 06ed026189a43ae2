"""tests/train_ops_ref.py — the float64 references the GPU tests of the training ops compare against — pinned without a GPU: every
hand-written backward equals torch.autograd.grad of the matching torch operator on float64 leaves to 1e-12 relative, at two small
shapes each, and the keep-mask reference has its fixed points."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_ref as R  # noqa: E402


def _leaf(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64, requires_grad=True)


def _same(a, b, what=""):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), (what, float((a - b).abs().max()))


def _grads(y, leaves, dy):
    return torch.autograd.grad(y, leaves, dy, retain_graph=True)


@pytest.mark.parametrize("n", [5, 37])
def test_unary_and_flat_ops(n):
    g = torch.Generator().manual_seed(n)
    x, dy, prev = _leaf(g, n), torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    for kind, op in ((0, F.silu), (1, torch.sigmoid)):
        y = op(x)
        _same(R.unary(kind, x), y, kind)
        (dx,) = _grads(y, (x,), dy)
        _same(R.unary_bwd(kind, dy, x if kind == 0 else y), dx, kind)
        _same(R.unary_bwd(kind, dy, x if kind == 0 else y, prev), prev + dx, kind)
    b, m = _leaf(g, n), (torch.rand(n, generator=g) > 0.3).double()
    _same(R.add(x, b), x + b)
    _same(R.add(x, None, prev), prev + x)
    _same(R.add(x, b, prev), prev + x + b)
    _same(R.mask_mul(x, m, 1.25), x * m * 1.25)
    (dx,) = _grads(x * m * 1.25, (x,), dy)
    _same(R.mask_mul(dy, m, 1.25, prev), prev + dx)          # (dropout is its own adjoint)


@pytest.mark.parametrize("B,L,C", [(1, 1, 1), (3, 5, 7)])
def test_film_and_film_act(B, L, C):
    g = torch.Generator().manual_seed(10 * B + C)
    x, ga, be, ad = _leaf(g, B, L, C), _leaf(g, B, C), _leaf(g, B, C), _leaf(g, B, L, C)
    dy = torch.randn(B, L, C, generator=g, dtype=torch.float64)
    px, pg, pb = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, L, C), (B, C), (B, C)))
    y = x * ga[:, None] + be[:, None]
    _same(R.film(x, ga, be), y)
    _same(R.add_rows(x, ad[0]), x + ad[0][None])
    dx, dg, db = _grads(y, (x, ga, be), dy)
    for got, want in zip(R.film_bwd(dy, x, ga), (dx, dg, db)):
        _same(got, want)
    for got, want in zip(R.film_bwd(dy, x, ga, px, pg, pb), (px + dx, pg + dg, pb + db)):
        _same(got, want)
    for act in (0, 1):
        for addend in (None, ad):
            y = F.silu(x * ga[:, None] + be[:, None]) if act else x * ga[:, None] + be[:, None]
            y = y if addend is None else y + addend
            _same(R.film_act(x, ga, be, act, addend), y, (act, addend is None))
            dx, dg, db = _grads(y, (x, ga, be), dy)
            for got, want in zip(R.film_act_bwd(dy, x, ga, be, act, px, pg, pb), (px + dx, pg + dg, pb + db)):
                _same(got, want, act)
            if addend is not None:
                _same(_grads(y, (ad,), dy)[0], dy)            # the addend's gradient is dy: no entry computes it


@pytest.mark.parametrize("B,L,C", [(1, 2, 3), (3, 4, 9)])
def test_layernorm_and_ln_film(B, L, C):
    g = torch.Generator().manual_seed(100 * B + C)
    x, ga, be, ad = _leaf(g, B, L, C), _leaf(g, B, C), _leaf(g, B, C), _leaf(g, B, L, C)
    pe = torch.randn(L, C, generator=g, dtype=torch.float64)
    dy, px = (torch.randn(B, L, C, generator=g, dtype=torch.float64) for _ in range(2))
    pg, pb = (torch.randn(B, C, generator=g, dtype=torch.float64) for _ in range(2))
    yn = F.layer_norm(x, (C,), eps=1e-6)
    y, mean, rstd = R.layernorm(x)
    _same(y, yn)
    _same(mean, x.mean(-1))
    _same(rstd, 1 / torch.sqrt(x.var(-1, unbiased=False) + 1e-6))
    (dx,) = _grads(yn, (x,), dy)
    _same(R.layernorm_bwd(dy, y, rstd), dx)
    _same(R.layernorm_bwd(dy, y, rstd, px), px + dx)
    for addend in (None, ad):
        t = F.layer_norm(x, (C,), eps=1e-6) * ga[:, None] + be[:, None]
        t = t if addend is None else t + addend
        y, act, yp, mean, rstd = R.ln_film(x, ga, be, addend, pe)
        _same(y, t)
        _same(act, F.silu(t))
        _same(yp, t + pe[None])
        assert R.ln_film(x, ga, be, addend)[2] is None
        dx, dg, db = _grads(t, (x, ga, be), dy)
        for got, want in zip(R.ln_film_bwd(dy, x, mean, rstd, ga, px, pg, pb), (px + dx, pg + dg, pb + db)):
            _same(got, want)
        for got, want in zip(R.ln_film_bwd(dy, x, mean, rstd, ga), (dx, dg, db)):
            _same(got, want)


@pytest.mark.parametrize("B,Rr,cols,scale", [(2, 3, 5, 1.0), (3, 4, 70, 0.125)])
def test_softmax(B, Rr, cols, scale):
    g = torch.Generator().manual_seed(cols)
    s = torch.randn(B, Rr, cols, generator=g)
    mask = torch.zeros(B, cols)
    for b in range(B):
        mask[b, cols - b - 1:] = 1
    mask[0, 1:] = 1                                             # one sample keeps a single key
    dp = torch.randn(B, Rr, cols, generator=g, dtype=torch.float64)
    for m in (None, mask):
        z = R.softmax_logits(s, m, scale)
        assert z.dtype == torch.float32
        zl = z.double().requires_grad_(True)
        p = F.softmax(zl, -1)
        _same(R.softmax(s, m, scale), p)
        if m is not None:
            assert bool((R.softmax(s, m, scale)[m[:, None].expand(B, Rr, cols) == 1] == 0).all())
        (dz,) = _grads(p, (zl,), dp)
        _same(R.softmax_bwd(dp, p, scale), dz * scale)           # d logits / d s = scale


@pytest.mark.parametrize("rows,C", [(2, 1), (6, 5)])
def test_resample(rows, C):
    g = torch.Generator().manual_seed(rows)
    cl = lambda t: t.t()[None]              # noqa: E731  rows C-last -> [1, C, rows]
    back = lambda t: t[0].t()               # noqa: E731
    x = _leaf(g, rows, C)
    prev_h, prev_d = (torch.randn(n, C, generator=g, dtype=torch.float64) for n in (rows // 2, rows * 2))
    y0 = back(F.avg_pool1d(cl(x), 2))
    y2 = back(F.interpolate(cl(x), scale_factor=2, mode="nearest"))
    _same(R.resample(0, x), y0)
    _same(R.resample(2, x), y2)
    _same(R.resample(0, x, prev_h), prev_h + y0)
    _same(R.resample(2, x, prev_d), prev_d + y2)
    dy0, dy2 = torch.randn_like(y0), torch.randn_like(y2)
    prev = torch.randn(rows, C, generator=g, dtype=torch.float64)
    _same(R.resample(1, dy0), _grads(y0, (x,), dy0)[0])
    _same(R.resample(3, dy2), _grads(y2, (x,), dy2)[0])
    _same(R.resample(1, dy0, prev), prev + _grads(y0, (x,), dy0)[0])
    _same(R.resample(3, dy2, prev), prev + _grads(y2, (x,), dy2)[0])


@pytest.mark.parametrize("V,rows,C", [(1, 1, 1), (7, 12, 5)])
def test_embedding_and_colsum(V, rows, C):
    g = torch.Generator().manual_seed(V)
    table = _leaf(g, V, C)
    ids = torch.randint(0, V, (rows,), generator=g)
    dy, prev = torch.randn(rows, C, generator=g, dtype=torch.float64), torch.randn(V, C, generator=g, dtype=torch.float64)
    y = F.embedding(ids, table)
    _same(R.embedding(ids, table), y)
    _same(R.embedding_bwd(ids, dy, prev), prev + _grads(y, (table,), dy)[0])
    b = _leaf(g, C)
    (db,) = _grads(table.detach()[ids] + b[None], (b,), dy)     # a bias gradient is the column sum of dy
    _same(R.colsum(dy), db)
    _same(R.colsum(dy, prev[0]), prev[0] + db)


@pytest.mark.parametrize("B,total", [(1, 1), (5, 9)])
def test_film_table(B, total):
    g = torch.Generator().manual_seed(total)
    n = 40 * total + 16
    perm = torch.randperm(total, generator=g)
    woff, boff = 40 * perm + 4, 40 * perm + 37                  # rows in permuted order with gaps, biases scattered between them
    flat, sigma = _leaf(g, n), _leaf(g, B, 32)
    W, b = flat[woff[:, None] + torch.arange(32)[None]], flat[boff]
    y = sigma @ W.t() + b
    _same(R.film_table(sigma, flat, woff, boff), y)
    dy = torch.randn(B, total, generator=g, dtype=torch.float64)
    pf, ps = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(B, 32, generator=g, dtype=torch.float64)
    dflat, dsig = _grads(y, (flat, sigma), dy)
    gf, gs = R.film_table_bwd(dy, sigma, flat, woff, boff, pf, ps)
    _same(gf, pf + dflat)
    _same(gs, ps + dsig)
    used = torch.zeros(n, dtype=torch.bool)
    used[(woff[:, None] + torch.arange(32)[None]).reshape(-1)] = True
    used[boff] = True
    assert torch.equal(gf[~used], pf[~used])                    # slots no woff / boff names come back as they were


@pytest.mark.parametrize("B,L", [(1, 3), (3, 10)])
def test_loss(B, L):
    g = torch.Generator().manual_seed(L)
    eps, pen = torch.randn(B, L, 2, generator=g, dtype=torch.float64), (torch.rand(B, L, generator=g) > 0.5).float()
    score = _leaf(g, B, L, 2)
    pp = (0.05 + 0.9 * torch.rand(B, L, generator=g, dtype=torch.float64)).requires_grad_(True)
    a = torch.rand(B, 1, generator=g, dtype=torch.float64)
    y = torch.clamp(pen, min=1e-7, max=1 - 1e-7).double()
    s = ((eps - score) ** 2).sum(-1).mean()
    q = (F.binary_cross_entropy(pp, y, reduction="none").mean(1) * a.squeeze(-1)).mean()
    out3, ds, dp = R.loss(eps, score, pen, pp, a)
    _same(out3, torch.stack([s + q, s, q]))
    want_s, want_p = _grads(s + q, (score, pp), torch.ones((), dtype=torch.float64))
    _same(ds, want_s)
    _same(dp, want_p)
    # the clamps, where autograd of log has no finite answer: log at -100, the gradient's denominator at 1e-12
    edge = torch.tensor([[0.0, 1.0, 1e-30]], dtype=torch.float64)
    o, _, d = R.loss(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2), torch.tensor([[1.0, 0.0, 1.0]]), edge, torch.ones(1))
    y1 = float(np.float32(1) - np.float32(1e-7))
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(d).all())
    assert abs(float(d[0, 0]) - (0.0 - y1) / 1e-12 / 3) <= 1e-12 * y1 / 1e-12 / 3
    assert abs(float(o[2]) - (100.0 * y1 + 100.0 * (1 - 1e-7) - y1 * np.log(1e-30)) / 3) <= 1e-9


def test_keep_mask_fixed_points():
    B, per = 3, 12
    assert R.keep_mask(7, 5, B, per, 0.0, 3).tolist() == [1.0] * (B * per)
    a, b = R.keep_mask(7, 5, B, per, 0.3, 3), R.keep_mask(7, 5, B, per, 0.3, 3)
    assert a.dtype == np.float32 and np.array_equal(a, b) and set(a.tolist()) <= {0.0, 1.0}
    assert R.keep_words(7, 16, 2, 3) == R.keep_words(7, 16, 2, 3)
    # another seed, stream, block or site gives other words
    base = R.keep_words(7, 16, 2, 3)
    for other in (R.keep_words(8, 16, 2, 3), R.keep_words(7, 17, 2, 3), R.keep_words(7, 16, 1, 3), R.keep_words(7, 16, 2, 4), R.keep_words(7, 16 + (1 << 32), 2, 3)):
        assert other != base
    # sample b of draw d at B samples is stream d * B + b: draw 5 at B = 4 is draws 10 and 11 at B = 2
    whole = R.keep_mask(7, 5, 4, per, 0.3, 2)
    halves = np.concatenate([R.keep_mask(7, 10, 2, per, 0.3, 2), R.keep_mask(7, 11, 2, per, 0.3, 2)])
    assert np.array_equal(whole, halves)
    # the rule itself on one block: u = ((w >> 8) + 0.5) 2^-24 in float32, kept where u >= p
    w = R.keep_words(7, 5 * B + 1, 2, 3)
    u = [(np.float32(x >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24) for x in w]
    for p in (0.3, 0.9):
        m = R.keep_mask(7, 5, B, per, p, 3)
        assert m[per + 8:per + 12].tolist() == [1.0 if x >= np.float32(p) else 0.0 for x in u]
