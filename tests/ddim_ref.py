"""The rules of include/dhw.h for dhw_ddim_sample / dhw_ddim_invert in torch on the CPU.  A helper, not a test: the denoiser is
a callable ``forward(sd, x, text, sigma, style) -> (eps, pen)`` (the tests pass ``oracle.ref_cpu.forward``).  Every arithmetic
step is one float32 torch operation, so each rounds on its own, as the kernel's do.  ``lengths`` are handled by running
each sample alone at ``L = lengths[b]``, which is what the header promises of a batch.  ``perturb`` (optional) is applied to
every ``(eps, pen)`` the denoiser returns: the GPU tests use it to measure how far a denoiser error of known size moves the
result."""
import numpy as np
import torch

from oracle import ref_cpu


def schedule(T):
    """abar as an fp32 numpy array: cumprod(1 - beta), beta = 0.02 + exp(linspace(ln 1e-5, ln 0.4, T))."""
    return ref_cpu.get_alpha_set(ref_cpu.get_beta_set(T)).numpy().astype(np.float32)


def coefs(levels, T, abar=None):
    """[(A_j, B_j)] for j = 0..S as numpy float32 scalars: sqrt(a_j), sqrt(1 - a_j); entry S is the clean end (1, 0)."""
    abar = schedule(T) if abar is None else np.asarray(abar, np.float32)
    one = np.float32(1.0)
    return [(np.sqrt(abar[i]), np.sqrt(one - abar[i])) for i in levels] + [(one, np.float32(0.0))]


def update(base, e, c0, c1, c2, c3):
    """U(base, e; c0, c1, c2, c3) = c2 * ((base - c1 * e) / c0) + c3 * e, five float32 operations."""
    c0, c1, c2, c3 = (torch.tensor(float(c), dtype=torch.float32) for c in (c0, c1, c2, c3))
    m = c1 * e
    d = base - m
    x0 = d / c0
    s = c2 * x0
    n = c3 * e
    return s + n


def _call(forward, sd, x, text, style, sigma, perturb):
    B = x.shape[0]
    with torch.no_grad():
        e, q = forward(sd, x, text, torch.full((B, 1, 1), float(sigma)), style)
    if perturb is not None:
        e, q = perturb(e, q)
    return e, q


def _sample_uniform(forward, sd, text, style, levels, T, latent, perturb):
    c = coefs(levels, T)
    x = latent.to(torch.float32).clone()
    q = None
    for j in range(len(levels)):
        e, q = _call(forward, sd, x, text, style, c[j][0], perturb)
        x = update(x, e, c[j][0], c[j][1], c[j + 1][0], c[j + 1][1])
    return torch.cat((x, q.reshape(x.shape[0], x.shape[1], 1)), dim=2)


def _invert_uniform(forward, sd, strokes, text, style, levels, T, iters, perturb):
    c = coefs(levels, T)
    y = strokes[..., :2].to(torch.float32).clone()
    for j in range(len(levels) - 1, -1, -1):
        w = y
        for _ in range(iters):
            e, _q = _call(forward, sd, w, text, style, c[j][0], perturb)
            w = update(y, e, c[j + 1][0], c[j + 1][1], c[j][0], c[j][1])
        y = w
    return y


def sample(forward, sd, text, style, levels, T, latent, lengths=None, perturb=None):
    """-> [B,L,3] = (x(S), pen of the last call), 0 past lengths[b]."""
    if lengths is None:
        return _sample_uniform(forward, sd, text, style, levels, T, latent, perturb)
    B, L = latent.shape[:2]
    out = torch.zeros((B, L, 3))
    for b, n in enumerate(lengths):
        out[b, :n] = _sample_uniform(forward, sd, text[b:b + 1], style[b:b + 1], levels, T, latent[b:b + 1, :n], perturb)[0]
    return out


def invert(forward, sd, strokes, text, style, levels, T, iters=1, lengths=None, perturb=None):
    """-> the latent [B,L,2], 0 past lengths[b]."""
    if lengths is None:
        return _invert_uniform(forward, sd, strokes, text, style, levels, T, iters, perturb)
    B, L = strokes.shape[:2]
    out = torch.zeros((B, L, 2))
    for b, n in enumerate(lengths):
        out[b, :n] = _invert_uniform(forward, sd, strokes[b:b + 1, :n], text[b:b + 1], style[b:b + 1], levels, T, iters, perturb)[0]
    return out


def sign_perturb(tol_eps, tol_pen, seed):
    """perturb(eps, pen) adding +-tol_eps to every eps element and +-tol_pen to every pen element, signs from one seeded generator."""
    g = torch.Generator().manual_seed(seed)

    def f(e, q):
        se = torch.randint(0, 2, e.shape, generator=g).to(torch.float32) * 2 - 1
        sq = torch.randint(0, 2, q.shape, generator=g).to(torch.float32) * 2 - 1
        return e + tol_eps * se, q + tol_pen * sq
    return f
