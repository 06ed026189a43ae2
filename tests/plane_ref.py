"""The all-steps text plane of dhw_sample in float64.  TEST INFRASTRUCTURE ONLY (tests/test_gpu_text_plane.py, tests/test_text_ref_cpu.py).

dhw_sample evaluates the sigma-dependent text side - TextStyleEncoder and every EncoderLayer's text keys / values - for all steps of
the schedule at once, in chunks of up to 64 steps, one (step, prompt) PAIR per slot of the plane (csrc/sampler/sample.cpp:206-221):
  * the chunk that starts at iteration c (counted from the first iteration that runs) writes slot k * Bs + b with step
    first + c + k of prompt b, k < min(64, steps left): every chunk writes from slot 0 on, so after the call the slots the last,
    shorter chunk did not reach still hold the chunk before it;
  * step s reads schedule index i = T - 1 - s: sigma = sqrtf(abar[i]) in float32 (sample.cpp:429), FiLM row i of the T-row table
    (the launch passes row i of its first step and a NEGATIVE row stride, film_div = Bs pairs per row).
The schedule is the project's Python statement of it (tests/ddim_ref.py schedule(), tied to tests/golden/sched.npz by
tests/test_oracle_golden.py), never read back from the library.
"""
import numpy as np
import torch

import block_ref as R
import ddim_ref

CHUNK = 64   # plane_chunk (csrc/sampler/plane_tag.h)


def plane_slots(T, Bs, first=0):
    """[(step, schedule index, prompt)] per pair slot, as a call of T steps that runs iterations [first, T) leaves the plane of a
    workspace with Bs prompts: min(64, T - first) * Bs slots."""
    run = T - first
    slots = [None] * (min(CHUNK, run) * Bs)
    for c in range(0, run, CHUNK):
        for k in range(min(CHUNK, run - c)):
            step = first + c + k
            for b in range(Bs):
                slots[k * Bs + b] = (step, T - 1 - step, b)
    return slots


def sigmas(T):
    """sigma per schedule index as the library feeds its sigma MLP: float32 sqrt of the float32 abar."""
    return np.sqrt(ddim_ref.schedule(T).astype(np.float32)).astype(np.float32)


def plane_reference(W, text, style, T, slots, rnd=R.exact, text_out=None, mut=None):
    """{"text_style_model": [pairs, Lt, 384], "<layer>.k1" / "<layer>.v1": [pairs, Lt, d]} in float64 for the given slots
    ((step, schedule index, prompt) triples of plane_slots).  text [B, Lt] int64, style [B, S, 1280] float32.
    text_out: what the layers' text halves read - the device's own text_out plane for the same slots (each block from the inputs its
    launch read) - or None: the reference's own.
    mut (WRONG variants, CPU tests): {"film_next": True} a pair reads the FiLM row of the next step (schedule index i - 1, where
    there is one); {"film_mirror": True} the FiLM row stride has the wrong sign: the k-th step of a chunk reads index i + 2 k, k rows
    on the other side of the chunk's first row (where the table has one); {"prompt_next": True} a pair reads prompt (b + 1) % B; {"swap_pairs": True} the k1 blocks of slots 2 j and
    2 j + 1 change places (the two pairs of a two-pair workgroup)."""
    m = mut or {}
    B = text.shape[0]
    sg = sigmas(T)
    idx = [max(i - 1, 0) if m.get("film_next") else i for _, i, _ in slots]
    if m.get("film_mirror"):
        idx = [min(i + 2 * (n // B), T - 1) for n, (_, i, _) in enumerate(slots)]   # (slot n is the (n // Bs)-th step of its chunk)
    pr = [(b + 1) % B if m.get("prompt_next") else b for _, _, b in slots]
    sig = R.sigma_ffn(W, torch.from_numpy(sg[idx].astype(np.float64)))
    tx, sv = torch.as_tensor(text)[pr], torch.as_tensor(style)[pr]
    out = {"text_style_model": R.text_style_encoder(W, tx, sv, sig, rnd).out}
    src = out["text_style_model"] if text_out is None else text_out
    nl = W.num_layers()
    for l in ["enc3", "enc5"] + [f"att_layers.{i}" for i in range(nl)]:
        k1, v1 = R.text_half(W, l, src, sig, rnd)
        if m.get("swap_pairs"):
            p = torch.arange(len(slots)) ^ 1
            p[p >= len(slots)] = len(slots) - 1
            k1 = k1[p]
        out[l + ".k1"], out[l + ".v1"] = k1, v1
    return out
