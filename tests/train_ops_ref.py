"""The generic operations of the training step (include/dhw_train.h dhw_op_* / dhw_train_loss / the keep masks) stated in float64
on the CPU, one plain function per operation, from the formulas in that header and the reference lines it cites — not from the
kernels.  Inputs are torch CPU tensors of any float type; every result is float64 unless noted.

Accumulating outputs: every backward that takes ``accumulate`` and every ``+=`` output takes the buffer's PREVIOUS content
(``prev`` / ``dgamma`` / ``dbeta`` / ... ; None = the call overwrites, or the buffer held zeros) and returns its FINAL content."""
import numpy as np
import torch

from batch_ref import M32, philox4x32_10

LN_EPS = 1e-6   # nn.LayerNorm(C, eps=1e-6, elementwise_affine=False)


def _d(t):
    return t.detach().to(torch.float64)


def _plus(prev, v):
    return v if prev is None else _d(prev) + v


def _silu(x):
    return x * torch.sigmoid(x)


def _dsilu(x):   # d SiLU / dx = s (1 + x (1 - s))
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


# ---- flat passes ---------------------------------------------------------------------------------------------------------
def unary(kind, x):
    """kind 0: SiLU, 1: sigmoid"""
    x = _d(x)
    return _silu(x) if kind == 0 else torch.sigmoid(x)


def unary_bwd(kind, dy, x_or_y, prev=None):
    """kind 0 takes the forward INPUT x, kind 1 the forward OUTPUT y"""
    dy, t = _d(dy), _d(x_or_y)
    return _plus(prev, dy * _dsilu(t) if kind == 0 else dy * t * (1 - t))


def add(a, b=None, prev=None):
    return _plus(prev, _d(a) if b is None else _d(a) + _d(b))


def add_rows(x, table):
    """x [B, L, C] + table [L, C]"""
    return _d(x) + _d(table)[None]


def mask_mul(x, mask, scale, prev=None):
    return _plus(prev, _d(x) * _d(mask) * float(scale))


def colsum(dy, prev=None):
    """db[c] += sum over rows of dy [rows, C]"""
    return _plus(prev, _d(dy).sum(0))


# ---- FiLM (conditioning.py:20-26): per-sample rows gamma / beta [B, C] on x [B, L, C] -----------------------------------
def film(x, gamma, beta):
    return _d(x) * _d(gamma)[:, None] + _d(beta)[:, None]


def film_bwd(dy, x, gamma, prev=None, dgamma=None, dbeta=None):
    """-> dx (+)= dy gamma, dgamma += sum_l dy x, dbeta += sum_l dy"""
    dy, x = _d(dy), _d(x)
    return _plus(prev, dy * _d(gamma)[:, None]), _plus(dgamma, (dy * x).sum(1)), _plus(dbeta, dy.sum(1))


def film_act(x, gamma, beta, act, addend=None):
    """y = act ? SiLU(x gamma + beta) : x gamma + beta, then + addend"""
    a = film(x, gamma, beta)
    if act:
        a = _silu(a)
    return a if addend is None else a + _d(addend)


def film_act_bwd(dy, x, gamma, beta, act, prev=None, dgamma=None, dbeta=None):
    """d' = act ? dy SiLU'(x gamma + beta) : dy, then as film_bwd on d' (the addend's gradient is dy itself)"""
    d = _d(dy)
    if act:
        d = d * _dsilu(film(x, gamma, beta))
    return film_bwd(d, x, gamma, prev, dgamma, dbeta)


# ---- LayerNorm (model.py:25) and LayerNorm -> FiLM ------------------------------------------------------------------------
def layernorm(x):
    """rows of x [..., C] -> (y, mean, rstd); biased variance, eps 1e-6, no affine"""
    x = _d(x)
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(((x - mean[..., None]) ** 2).mean(-1) + LN_EPS)
    return (x - mean[..., None]) * rstd[..., None], mean, rstd


def layernorm_bwd(dy, y, rstd, prev=None):
    """dx (+)= rstd (dy - mean(dy) - y mean(dy y)) with y the normalised rows"""
    dy, y = _d(dy), _d(y)
    v = _d(rstd)[..., None] * (dy - dy.mean(-1, keepdim=True) - y * (dy * y).mean(-1, keepdim=True))
    return _plus(prev, v)


def ln_film(x, gamma, beta, addend=None, pe=None):
    """x [B, L, C], gamma / beta [B, C], addend [B, L, C], pe [L, C] -> (y, SiLU(y), y + pe[l] or None, mean [B, L], rstd [B, L])"""
    xn, mean, rstd = layernorm(x)
    y = xn * _d(gamma)[:, None] + _d(beta)[:, None]
    if addend is not None:
        y = y + _d(addend)
    return y, _silu(y), (None if pe is None else y + _d(pe)[None]), mean, rstd


def ln_film_bwd(dy, x, mean, rstd, gamma, prev=None, dgamma=None, dbeta=None):
    """With the forward's saved mean / rstd [B, L]: xn = (x - mean) rstd, dn = dy gamma,
    dx (+)= rstd (dn - mean(dn) - xn mean(dn xn)), dgamma += sum_l dy xn, dbeta += sum_l dy"""
    dy = _d(dy)
    xn = (_d(x) - _d(mean)[..., None]) * _d(rstd)[..., None]
    dn = dy * _d(gamma)[:, None]
    dx = _d(rstd)[..., None] * (dn - dn.mean(-1, keepdim=True) - xn * (dn * xn).mean(-1, keepdim=True))
    return _plus(prev, dx), _plus(dgamma, (dy * xn).sum(1)), _plus(dbeta, dy.sum(1))


# ---- softmax (attention.py:16-22) -----------------------------------------------------------------------------------------
def softmax_logits(s, mask, scale):
    """s [B, R, cols] fp32, mask [B, cols] fp32 or None -> the logits s * scale + mask * -1e9 as the header writes them, in float32
    one rounded operation at a time: the fp32 add is what makes a masked key's logit exactly -1e9 and its probability exactly 0."""
    z = s.detach().to(torch.float32) * torch.tensor(scale, dtype=torch.float32)
    if mask is not None:
        z = z + (mask.detach().to(torch.float32) * torch.tensor(-1e9, dtype=torch.float32))[:, None]
    return z


def softmax(s, mask, scale):
    z = _d(softmax_logits(s, mask, scale))
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd(dp, p, scale):
    """dS = scale P (dP - sum_key dP P)"""
    dp, p = _d(dp), _d(p)
    return float(scale) * p * (dp - (dp * p).sum(-1, keepdim=True))


# ---- AvgPool1d(2) / nearest x2 Upsample over rows and their adjoints ------------------------------------------------------
def resample(mode, x, prev=None):
    """x [rows_in, C].  0: pool forward, 1: pool backward, 2: upsample forward, 3: upsample backward"""
    x = _d(x)
    if mode == 0:
        v = 0.5 * (x[0::2] + x[1::2])
    elif mode == 1:
        v = 0.5 * x.repeat_interleave(2, 0)
    elif mode == 2:
        v = x.repeat_interleave(2, 0)
    else:
        v = x[0::2] + x[1::2]
    return _plus(prev, v)


# ---- nn.Embedding ---------------------------------------------------------------------------------------------------------
def embedding(ids, table):
    return _d(table)[ids.reshape(-1).long()]


def embedding_bwd(ids, dy, dtable):
    """dtable [V, C] += scatter of dy [rows, C]"""
    out = _d(dtable).clone()
    out.index_add_(0, ids.reshape(-1).long(), _d(dy))
    return out


# ---- every FiLM Linear as one table over the flat parameter buffer --------------------------------------------------------
def film_table(sigma, flat, woff, boff):
    """film[b][j] = flat[boff[j]] + sum_k sigma[b][k] flat[woff[j] + k]"""
    flat = _d(flat)
    W = flat[woff.long()[:, None] + torch.arange(32)[None]]          # [total, 32]
    return _d(sigma) @ W.t() + flat[boff.long()][None]


def film_table_bwd(dfilm, sigma, flat, woff, boff, grad_flat, dsigma):
    """-> (grad_flat, dsigma): grad_flat[woff[j] + k] += sum_b dfilm[b][j] sigma[b][k], grad_flat[boff[j]] += sum_b dfilm[b][j],
    dsigma[b][k] += sum_j dfilm[b][j] flat[woff[j] + k]"""
    dfilm, flat = _d(dfilm), _d(flat)
    rows = woff.long()[:, None] + torch.arange(32)[None]
    g = _d(grad_flat).clone()
    g.index_put_((rows.reshape(-1),), (dfilm.t() @ _d(sigma)).reshape(-1), accumulate=True)
    g.index_put_((boff.long(),), dfilm.sum(0), accumulate=True)
    return g, _d(dsigma) + dfilm @ flat[rows]


# ---- the loss (loss.py:5-37) and its gradients ----------------------------------------------------------------------------
def loss(eps, score_pred, pen, pen_pred, alphas):
    """eps / score_pred [B, L, 2], pen / pen_pred [B, L], alphas [B] -> (out3 = [loss, score_loss, pen_lifts_loss], d loss / d
    score_pred, d loss / d pen_pred).  The target is clamped in float32 as loss.py does; binary_cross_entropy clamps its logs at
    -100 and the denominator of its gradient at 1e-12."""
    B, L = pen.shape
    diff = _d(eps) - _d(score_pred)
    score = (diff ** 2).sum(-1).mean()
    y = _d(torch.clamp(pen.detach().to(torch.float32), min=1e-7, max=1 - 1e-7))
    pp, a = _d(pen_pred), _d(alphas).reshape(B)
    lp = torch.clamp(torch.log(pp), min=-100.0)
    lq = torch.clamp(torch.log(1 - pp), min=-100.0)
    bce = -(y * lp + (1 - y) * lq)
    pen_loss = (bce.mean(1) * a).mean()
    d_score = -2.0 * diff / (B * L)
    d_pen = (pp - y) / torch.clamp(pp * (1 - pp), min=1e-12) * a[:, None] / (B * L)
    return torch.stack([score + pen_loss, score, pen_loss]), d_score, d_pen


# ---- Dropout keep masks from the counter-based generator ------------------------------------------------------------------
def keep_words(seed, stream, block, w3):
    """The four Philox4x32-10 words of (stream, block of 4 elements, w3) under key = seed"""
    stream = int(stream) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((stream & M32, stream >> 32, block, w3), (int(seed) & M32, (int(seed) >> 32) & M32))


def keep_mask(seed, index, B, per_sample, p, w3):
    """-> float32 [B * per_sample], 1 = kept.  Sample b of draw ``index`` is stream index * B + b; element e of a sample takes word
    e % 4 of block e // 4; w3 = 2 for the style mask of dhw_train_draw, the site number (>= 3) for dhw_op_keep_mask.  The keep rule
    ((w >> 8) + 0.5) 2^-24 >= p is evaluated in float32, one operation at a time."""
    assert per_sample % 4 == 0
    out = np.zeros(B * per_sample, np.float32)
    p32 = np.float32(p)
    for b in range(B):
        for blk in range(per_sample // 4):
            w = keep_words(seed, int(index) * B + b, blk, w3)
            for k in range(4):
                u = (np.float32(w[k] >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
                out[b * per_sample + 4 * blk + k] = 1.0 if u >= p32 else 0.0
    return out
