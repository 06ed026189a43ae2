"""Float64 statements of what dhw_train_adam_ema_dev computes (include/dhw_train.h), for the tests of the fused optimizer pass:
the clipped Adam step of dhw_train_adam_dev and the EMA line.  Both take the scalars as the DEVICE holds them — rounded to fp32 —
and evaluate every operation in float64; numpy only."""
import numpy as np


def f32(x):
    """A scalar or array rounded to fp32 and widened again: the value the device reads."""
    return np.asarray(x, np.float32).astype(np.float64)


def adam_step(p, g, m, v, hyper):
    """One update of flat buffers p, g, m, v (any float arrays, taken as float64) under hyper[9] = {lr, beta1, beta2, eps,
    weight_decay, 1 - beta1^t, 1 - beta2^t, max_norm (<= 0: no clipping), grad_scale} -> (p', m', v', sqnorm): the global-norm clip
    min(1, max_norm / (||grad_scale g|| + 1e-6)), L2 weight decay folded into the gradient, bias-corrected moments.  sqnorm is the
    squared norm of g itself, as the entry leaves it."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, bc1, bc2, max_norm, gs = (float(h) for h in f32(hyper))
    sqnorm = float(np.sum(g * g))
    clip = gs
    if max_norm > 0:
        clip = gs * min(1.0, max_norm / (np.sqrt(sqnorm) * gs + float(f32(1e-6))))
    gi = g * clip + wd * p
    m2 = b1 * m + (1.0 - b1) * gi
    v2 = b2 * v + (1.0 - b2) * gi * gi
    p2 = p - lr / bc1 * m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps)
    return p2, m2, v2, sqnorm


def ema_line(ema, p_new, ema_hyper):
    """ema' = decay ema + omd p' with ema_hyper = {decay, omd} as the device holds them (each rounded to fp32 on its own)."""
    decay, omd = (float(h) for h in f32(ema_hyper))
    return decay * np.asarray(ema, np.float64) + omd * np.asarray(p_new, np.float64)


def ema_decay_at(t, decay):
    """The warm-up rule, restated: min(decay, (1 + t) / (10 + t))."""
    return min(decay, (1 + t) / (10 + t))
