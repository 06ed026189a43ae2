"""The rules of include/dhw.h for dhw_dpm_sample / dhw_dpm_coefs (second-order multistep sampling) in torch and
numpy on the CPU, generic over the dtype.  A helper, not a test.

``dtype=torch.float32`` is the library's statement: A_j, B_j are ddim_ref's float32 pairs, the second-order coefficients are
computed in Python floats (double: ``math.log`` / ``math.expm1``) from those float32 values and rounded once to float32, and
every arithmetic step of the update is one float32 torch operation, so each rounds on its own, as the kernel's do.
``dtype=torch.float64`` is the same rule with every number a double (the schedule too): what the float32 statement is measured
against.  The denoiser is a callable ``forward(sd, x, text, sigma, style) -> (eps, pen)``: ``oracle.ref_cpu.forward`` as in
ddim_ref.py, ``guide_ref.guided_forward`` of it for a guided call, or an analytic one (``gaussian_denoiser``).  ``lengths`` are
handled by running each sample alone at ``L = lengths[b]``.  ``perturb`` is ddim_ref's hook."""
import math

import numpy as np
import torch

import ddim_ref


def schedule64(T):
    """abar in float64: cumprod(1 - beta), beta = 0.02 + exp(linspace(ln 1e-5, ln 0.4, T))."""
    beta = 0.02 + np.exp(np.linspace(np.log(1e-5), np.log(0.4), T))
    return np.cumprod(1.0 - beta)


def levels_ab(levels, T, dtype=torch.float32, abar=None):
    """[(A_j, B_j)] j = 0..S as Python floats holding values of ``dtype``; entry S is the clean end (1, 0)."""
    if dtype == torch.float32:
        return [(float(a), float(b)) for a, b in ddim_ref.coefs(levels, T, abar=abar)]
    abar = schedule64(T) if abar is None else np.asarray(abar, np.float64)
    return [(math.sqrt(abar[i]), math.sqrt(1.0 - abar[i])) for i in levels] + [(1.0, 0.0)]


def second_order(ab, j):
    """(k0, k1, c4, c5) of step j (0 < j < S - 1) in double from the table's A, B."""
    lam = [math.log(a / b) for a, b in ab[j - 1:j + 2]]
    h = lam[2] - lam[1]
    r = (lam[1] - lam[0]) / h
    k1 = 1.0 / (2.0 * r)
    return 1.0 + k1, k1, ab[j + 1][1] / ab[j][1], -ab[j + 1][0] * math.expm1(-h)


def table(levels, T, order, dtype=torch.float32, abar=None):
    """S rows (kind, c0, c1, c2, c3, k0, k1, c4, c5) as Python floats holding values of ``dtype``: dhw_dpm_coefs' layout."""
    ab = levels_ab(levels, T, dtype, abar)
    S = len(levels)
    rows = []
    for j in range(S):
        row = [1.0, ab[j][0], ab[j][1], ab[j + 1][0], ab[j + 1][1], 0.0, 0.0, 0.0, 0.0]
        if order == 2 and 0 < j < S - 1:
            row[0] = 2.0
            row[5:] = second_order(ab, j)
            if dtype == torch.float32:
                row[5:] = [float(np.float32(v)) for v in row[5:]]   # each rounded once
        rows.append(row)
    return rows


def step(x, e, hist, row, dtype=torch.float32):
    """One step on tensors of ``dtype`` -> (x', x0): nine operations for kind 2, U's five (and x0's three) for kind 1."""
    kind, c0, c1, c2, c3, k0, k1, c4, c5 = (torch.tensor(v, dtype=dtype) for v in row)
    m = c1 * e
    d = x - m
    x0 = d / c0
    if row[0] == 2.0:
        p = k0 * x0
        q = k1 * hist
        D = p - q
        s = c4 * x
        n = c5 * D
        return s + n, x0
    s = c2 * x0
    n = c3 * e
    return s + n, x0


def _sample_uniform(forward, sd, text, style, rows, latent, perturb, dtype):
    x = latent.to(dtype).clone()
    hist, q = None, None
    for row in rows:
        B = x.shape[0]
        with torch.no_grad():
            e, q = forward(sd, x, text, torch.full((B, 1, 1), row[1], dtype=dtype), style)
        if perturb is not None:
            e, q = perturb(e, q)
        x, hist = step(x, e, hist, row, dtype)
    return torch.cat((x, q.reshape(x.shape[0], x.shape[1], 1).to(dtype)), dim=2)


def sample(forward, sd, text, style, levels, T, latent, order=2, lengths=None, perturb=None, dtype=torch.float32, abar=None):
    """-> [B,L,3] = (x(S), pen of the last call), 0 past lengths[b]."""
    rows = table(levels, T, order, dtype, abar)
    if lengths is None:
        return _sample_uniform(forward, sd, text, style, rows, latent, perturb, dtype)
    B, L = latent.shape[:2]
    out = torch.zeros((B, L, 3), dtype=dtype)
    for b, n in enumerate(lengths):
        out[b, :n] = _sample_uniform(forward, sd, text[b:b + 1], style[b:b + 1], rows, latent[b:b + 1, :n], perturb, dtype)[0]
    return out


# ---------------------------------------------------------------- a problem with a known answer
def gaussian_denoiser(mu, s):
    """The exact denoiser of 1-D Gaussian data N(mu, s^2): at level (A, B = sqrt(1 - A^2)) x is N(A mu, A^2 s^2 + B^2) and
    E[eps | x] = B (x - A mu) / (A^2 s^2 + B^2).  The probability-flow solution from x = A mu + sqrt(A^2 s^2 + B^2) z is
    mu + s z at the clean end.  Computes in x's dtype; the pen is 0."""
    def f(sd, x, text, sigma, style):
        A = sigma.to(x.dtype)
        B2 = 1.0 - A * A
        e = torch.sqrt(B2) * (x - A * mu) / (A * A * s * s + B2)
        return e, torch.zeros(x.shape[:2], dtype=x.dtype)
    return f


def gaussian_problem(levels, T, n=4096, mu=0.7, s=0.5, seed=0):
    """(start [1,n/2,2] float64 at level 0 of ``levels``, exact [1,n/2,2]) for n draws z from default_rng(seed): n starts of the
    1-D problem, laid out as the two coordinates of n/2 stroke rows."""
    z = torch.from_numpy(np.random.default_rng(seed).standard_normal(n).reshape(1, n // 2, 2))
    A, B = levels_ab(levels, T, torch.float64)[0]
    return A * mu + math.sqrt(A * A * s * s + B * B) * z, mu + s * z
