"""The rules of include/dhw.h for dhw_guided_ddim_sample / dhw_guided_sample and of include/dhw_train.h for
dhw_train_cond_drop, in torch and numpy on the CPU.  A helper, not a test.

Guided sampling is the unguided reference with another denoiser: ``ddim_ref.sample`` (its ``update``) and
``cond_ref.cond_sample`` (its scheduler step) are called as they are, with a ``forward`` that asks the real denoiser
(``forward(sd, x, text, sigma, style) -> (eps, pen)``, the tests pass ``oracle.ref_cpu.forward``) TWICE — under the real and
under the guidance condition — and returns the combined eps with the conditional pen.  Every arithmetic step is one float32
torch operation.  ``lengths`` are handled by running each sample alone at ``L = lengths[b]``.  ``perturb`` (optional, ddim_ref's
hook) is applied to the ``(eps, pen)`` of BOTH branches, before they are combined.

Conditioning dropout is batch_ref's Philox block with the counter (stream, 1, 0)."""
import numpy as np
import torch

import batch_ref
import cond_ref
import ddim_ref


def combine(e_c, e_u, w):
    """e = e_c + (w - 1) (e_c - e_u), the scalar and three float32 operations per element; w == 0 selects e_u (include/dhw.h)."""
    w = torch.as_tensor(w, dtype=torch.float32)
    g = w - torch.tensor(1.0)
    d = e_c - e_u
    m = g * d
    e = e_c + m
    return torch.where(w == 0, e_u, e)


def guided_forward(forward, utext, ustyle, scale, perturb=None):
    """-> forward'(sd, x, text, sigma, style) = (combine(e_c, e_u, scale), q_c); scale: float32 [B] (broadcast over rows)."""
    w = torch.as_tensor(scale, dtype=torch.float32).reshape(-1, 1, 1)

    def f(sd, x, text, sigma, style):
        e_c, q_c = forward(sd, x, text, sigma, style)
        e_u, q_u = forward(sd, x, utext, sigma, ustyle)
        if perturb is not None:
            e_c, q_c = perturb(e_c, q_c)
            e_u, q_u = perturb(e_u, q_u)
        return combine(e_c, e_u, w), q_c
    return f


def _scales(scale, B):
    s = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
    return s.expand(B).clone() if s.numel() == 1 else s


def sample_ddim(forward, sd, text, style, utext, ustyle, scale, levels, T, latent, lengths=None, perturb=None):
    """-> [B,L,3] = (x(S), conditional pen of the last call), 0 past lengths[b]."""
    B, L = latent.shape[:2]
    w = _scales(scale, B)
    if lengths is None:
        return ddim_ref.sample(guided_forward(forward, utext, ustyle, w, perturb), sd, text, style, levels, T, latent)
    out = torch.zeros((B, L, 3))
    for b, n in enumerate(lengths):
        f = guided_forward(forward, utext[b:b + 1], ustyle[b:b + 1], w[b:b + 1], perturb)
        out[b, :n] = ddim_ref.sample(f, sd, text[b:b + 1], style[b:b + 1], levels, T, latent[b:b + 1, :n])[0]
    return out


def sample(forward, sd, text, style, utext, ustyle, scale, L, noise, T, mode="new", lengths=None, perturb=None):
    """The guided ancestral loop with external noise [T+1,B,L,2] -> [B,L,3], 0 past lengths[b]."""
    B = text.shape[0]
    w = _scales(scale, B)
    if lengths is None:
        return cond_ref.cond_sample(guided_forward(forward, utext, ustyle, w, perturb), sd, text, style, L, noise, T=T, mode=mode)
    out = torch.zeros((B, L, 3))
    for b, n in enumerate(lengths):
        f = guided_forward(forward, utext[b:b + 1], ustyle[b:b + 1], w[b:b + 1], perturb)
        out[b, :n] = cond_ref.cond_sample(f, sd, text[b:b + 1], style[b:b + 1], n, noise[:, b:b + 1, :n].contiguous(), T=T, mode=mode)[0]
    return out


# ---------------------------------------------------------------- conditioning dropout
def drop_words(seed, index, B):
    """The four Philox output words of every sample of draw ``index``: counter (lo, hi of the stream index * B + b, 1, 0)."""
    out = []
    for b in range(B):
        stream = (int(index) * B + b) & 0xFFFFFFFFFFFFFFFF
        out.append(batch_ref.philox4x32_10((stream & batch_ref.M32, stream >> 32, 1, 0), (int(seed) & batch_ref.M32, (int(seed) >> 32) & batch_ref.M32)))
    return out


def cond_drop(seed, index, B, p):
    """-> dropped int32 [B]: u = ((w0 >> 8) + 0.5) 2^-24 in float32, dropped iff u < float32(p)."""
    p = np.float32(p)
    u = [(np.float32(w[0] >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24) for w in drop_words(seed, index, B)]
    return np.array([1 if x < p else 0 for x in u], np.int32)


def apply_drop(dropped, ids, mask, style):
    """(ids int64 [B,Lt], mask f32 [B,Lt], style f32 [B,S,1280]) with the dropped samples set to the null condition (copies)."""
    ids, mask, style = np.array(ids, np.int64), np.array(mask, np.float32), np.array(style, np.float32)
    for b in np.nonzero(np.asarray(dropped))[0]:
        ids[b] = 0
        ids[b, 0] = 1
        mask[b] = 1.0
        mask[b, 0] = 0.0
        style[b] = 0.0
    return ids, mask, style
