"""The conditioned reverse loop of include/dhw.h (dhw_sample_cond, rules 1-4) in torch on the CPU, for uniform lengths and
external noise.  A helper, not a test: the denoiser is a callable ``forward(sd, x, text, sigma, style) -> (eps, pen)``
(the tests pass ``oracle.ref_cpu.forward``).  The scheduler step is written in the operation order of ``heads_finish``
(csrc/heads_core.h) with fp32 scalar coefficients, one rounding per operation."""
import numpy as np
import torch


def schedule(T):
    """(beta, abar) as fp32 numpy arrays: 0.02 + exp(linspace(ln 1e-5, ln 0.4, T)) and its cumprod(1 - beta)."""
    from oracle import ref_cpu
    beta = ref_cpu.get_beta_set(T)
    return beta.numpy().astype(np.float32), ref_cpu.get_alpha_set(beta).numpy().astype(np.float32)


def a_next_of(abar, i):
    return abar[i - 1] if i > 1 else np.float32(1.0)


def noised(known_xy, z, abar_level):
    """fadd(fmul(sqrtf(abar), known_xy), fmul(sqrtf(1 - abar), z)) in fp32."""
    a = np.float32(abar_level)
    ka, kb = float(np.sqrt(a)), float(np.sqrt(np.float32(1.0) - a))
    return known_xy * ka + z * kb


def cond_sample(forward, sd, text, style, L, noise, T=60, mode="new", known=None, keep=None, t_start=None, cond_noise=None):
    """-> out [B,L,3].  noise [T+1,B,L,2], cond_noise [T,B,L,2] (needed iff keep is given), known [B,L,3], keep bool [B,L]."""
    beta, abar = schedule(T)
    t_start = T if t_start is None else t_start
    B = text.shape[0]
    kept = keep.bool() if keep is not None else torch.zeros((B, L), dtype=torch.bool)
    x = noise[0].clone()
    if known is not None:
        seeded = torch.ones_like(kept) if t_start < T else kept
        x = torch.where(seeded[..., None], noised(known[..., :2], x, abar[t_start - 1]), x)
    pen = None
    one = np.float32(1.0)
    with torch.no_grad():
        for k in range(T - t_start, T):
            i = T - 1 - k
            a, b = abar[i], beta[i]
            a_next = a_next_of(abar, i)
            sigma = torch.full((B, 1, 1), float(np.sqrt(a)))
            eps, pen = forward(sd, x, text, sigma, style)
            z = noise[1 + k]
            k0 = float(np.sqrt(one - a))
            if mode == "new":
                k1, k2 = float(np.sqrt(one - b)), float(np.sqrt(one - a_next))
                x = (x - k0 * eps) / k1
                x = x + z * k2
            else:
                k1, k2, k3 = float(one / np.sqrt(one - b)), float(np.sqrt(b)), float(b)
                x = k1 * (x - (k3 * eps) / k0)
                if i != 0:
                    x = x + k2 * z
            if keep is not None:
                x = torch.where(kept[..., None], noised(known[..., :2], cond_noise[k], a_next), x)
    out = torch.cat((x, pen.unsqueeze(2)), dim=2)
    if keep is not None:
        out = torch.where(kept[..., None], known, out)
    return out
