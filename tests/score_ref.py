"""The scoring rules of include/dhw.h (dhw_score, rules 1-4) in torch on the CPU, with explicit noise.  A helper, not a test:
the denoiser is a callable ``forward(sd, x, text, sigma, style) -> (eps, pen)`` (the tests pass ``oracle.ref_cpu.forward``).
``lengths`` are handled by scoring each sample alone at ``L = lengths[b]``, which is what rule 6 promises of a batch."""
import numpy as np
import torch

from oracle import ref_cpu


def schedule(T):
    """abar as an fp32 numpy array: cumprod(1 - beta), beta = 0.02 + exp(linspace(ln 1e-5, ln 0.4, T))."""
    return ref_cpu.get_alpha_set(ref_cpu.get_beta_set(T)).numpy().astype(np.float32)


def bce(q, pen):
    """-(t max(log q, -100) + (1 - t) max(log(1 - q), -100)), t = clamp(pen, 1e-7, 1 - 1e-7): rule 4, element-wise."""
    t = torch.clamp(pen, min=1e-7, max=1 - 1e-7)
    return -(t * torch.clamp(torch.log(q), min=-100.0) + (1 - t) * torch.clamp(torch.log(1 - q), min=-100.0))


def score_terms(forward, sd, strokes, text, style, abar_i, z):
    """One level, uniform length: (out [B,2], details) with details = dict(z, eps, pen, q) for a test's own bounds."""
    B = strokes.shape[0]
    a = torch.full((B, 1), float(abar_i))
    x_t = ref_cpu.perturb(strokes[..., :2], z, a)
    with torch.no_grad():
        eps, q = forward(sd, x_t, text, torch.sqrt(a).reshape(B, 1, 1), style)
    s = ((z - eps) ** 2).sum(dim=-1).mean(dim=1)
    p = float(abar_i) * bce(q, strokes[..., 2]).mean(dim=1)
    return torch.stack((s, p), dim=1), dict(z=z, eps=eps, pen=strokes[..., 2], q=q, abar=float(abar_i))


def score(forward, sd, strokes, text, style, levels, T, noise, lengths=None, details=None):
    """-> [B,K,2].  noise [K,B,L,2]; ``details`` (optional list) receives one dict per (k, b) or per k (uniform)."""
    abar = schedule(T)
    B, L = strokes.shape[:2]
    out = torch.zeros((B, len(levels), 2))
    for k, i in enumerate(levels):
        if lengths is None:
            o, d = score_terms(forward, sd, strokes, text, style, abar[i], noise[k])
            out[:, k] = o
            if details is not None:
                details.append(d)
        else:
            for b, n in enumerate(lengths):
                o, d = score_terms(forward, sd, strokes[b:b + 1, :n], text[b:b + 1], style[b:b + 1], abar[i], noise[k, b:b + 1, :n])
                out[b, k] = o[0]
                if details is not None:
                    details.append(d)
    return out
