"""The reverse-diffusion sampler: ``sample`` is the body of the reference's ``infer``
loop (reference inference.py:80-96) for a whole prompt batch; ``infer`` wraps it with
the tokenizer and the stroke-length heuristic (inference.py:65-78)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .model import DiffusionModel, attention_layer_index, check_lengths, check_token_ids  # noqa: F401 (check_token_ids: re-exported)
from .tokenizer import Tokenizer, stroke_length


def get_beta_set(T: int = 60) -> torch.Tensor:
    """beta_i = 0.02 + exp(linspace(ln 1e-5, ln 0.4, T)) (reference utils/nn.py:19-39); host-only."""
    return torch.from_numpy(_lib.schedule(T)[0])


def get_alpha_set(T: int = 60) -> torch.Tensor:
    """abar = cumprod(1 - beta) (reference inference.py:81)."""
    return torch.from_numpy(_lib.schedule(T)[1])


def _check_int(name: str, v, lo: int | None = None, hi: int | None = None, why: str | None = None, hi_text: str | None = None) -> int:
    """The one "a real integer in [lo, hi]" check.  ``why``: the caller's own wording for any failure (``name = v why``);
    ``hi_text``: how the caller names the upper bound in the range message."""
    is_int = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))
    in_range = is_int and (lo is None or v >= lo) and (hi is None or v <= hi)
    if why is not None and not in_range:
        raise ValueError(f"{name} = {v!r} {why}")
    if not is_int:
        raise ValueError(f"{name} = {v!r} is not an integer")
    if not in_range:
        raise ValueError(f"{name} = {v} must lie in [{lo}, {hi_text or hi}]" if hi is not None else f"{name} = {v} must be at least {lo}")
    return int(v)


def _check_strokes(strokes, name: str = "strokes"):
    """The [B,L,3] floating-point rule of every entry that reads existing strokes; returns (B, L)."""
    if not isinstance(strokes, torch.Tensor) or not strokes.dtype.is_floating_point:
        raise ValueError(f"{name} must be a floating-point tensor [B,L,3]")
    if strokes.dim() != 3 or strokes.shape[2] != 3:
        raise ValueError(f"{name} must be [B,L,3], got {tuple(strokes.shape)}")
    return int(strokes.shape[0]), int(strokes.shape[1])


# ---------------------------------------------------------------- classifier-free guidance (include/dhw.h dhw_guided_*)
MAX_GUIDANCE = 64.0


def null_condition(B: int, Lt: int, S: int = 14):
    """The condition guided sampling extrapolates away from and conditioning dropout trains (include/dhw_train.h
    dhw_train_cond_drop): ``text`` int64 [B,Lt] with every row ``[1, 0, 0, ...]`` — ``Tokenizer().encode("")``, the end token,
    then padding (not an all-padding row) — and ``style`` f32 [B,S,1280] of zeros."""
    B, Lt, S = _check_int("B", B, 1), _check_int("Lt", Lt, 1), _check_int("S", S, 1)
    ids = Tokenizer().encode("")
    if len(ids) > Lt:
        raise ValueError(f"Lt = {Lt} is shorter than the empty prompt's {len(ids)} token(s)")
    text = torch.zeros((B, Lt), dtype=torch.int64)
    text[:, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    return text, torch.zeros((B, S, 1280), dtype=torch.float32)


def _guided_kw(guidance, candidates: int, B: int | None = None) -> dict:
    """What a front end passes on for its ``guidance`` argument: nothing for None (the unguided calls stay as they are, argument
    for argument); refused next to best-of-N, whose candidates are scored as unguided samples."""
    if guidance is None:
        return {}
    if candidates > 1:
        raise ValueError("guidance cannot be combined with candidates > 1 (best-of-N ranks unguided samples by score)")
    if B is not None:
        _check_guidance(guidance, B)
    return {"guidance": guidance}


def _check_guidance(guidance, B: int) -> list:
    """``guidance`` (a real number, or B of them as a sequence or tensor) -> B floats, each finite and in [0, MAX_GUIDANCE]."""
    if isinstance(guidance, torch.Tensor):
        guidance = guidance.detach().cpu().tolist()
    if isinstance(guidance, np.ndarray):
        guidance = guidance.tolist()
    is_num = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))   # noqa: E731
    if is_num(guidance):
        seq = [guidance] * B
    else:
        try:
            seq = list(guidance)
        except TypeError:
            raise ValueError(f"guidance must be a number or a sequence of B = {B} numbers, got {type(guidance).__name__}") from None
        if len(seq) != B:
            raise ValueError(f"guidance has {len(seq)} entries, B = {B} are needed")
    for b, v in enumerate(seq):
        if not is_num(v):
            raise ValueError(f"guidance[{b}] = {v!r} is not a number")
        if not (0.0 <= float(np.float32(v)) <= MAX_GUIDANCE):    # (a NaN fails the range test)
            raise ValueError(f"guidance[{b}] = {v!r} must be finite and lie in [0, {MAX_GUIDANCE:g}]")
    return [float(np.float32(v)) for v in seq]


def _guided_pair(text, style_vector, uncond_text, uncond_style):
    """The 2B-row condition of a guided call, checked on the host: rows [0, B) the real condition, rows [B, 2B) the guidance
    condition (each half of ``null_condition`` unless given) -> (text2 int64 [2B,Lt], style2 f32 [2B,S,1280])."""
    B, Lt = text.shape
    if not isinstance(style_vector, torch.Tensor) or style_vector.dim() != 3 or style_vector.shape[0] != B or style_vector.shape[2] != 1280:
        raise ValueError(f"style_vector must be a tensor [B = {B}, S, 1280]")
    if text.dtype.is_floating_point or text.dtype == torch.bool:
        raise ValueError("text must be an integer tensor [B, Lt]")
    S = int(style_vector.shape[1])
    nt, ns = null_condition(B, Lt, S)
    if uncond_text is not None:
        if not isinstance(uncond_text, torch.Tensor) or uncond_text.dtype.is_floating_point or uncond_text.dtype == torch.bool:
            raise ValueError("uncond_text must be an integer tensor [B, Lt]")
        if tuple(uncond_text.shape) != (B, Lt):
            raise ValueError(f"uncond_text must be [B,Lt] = {(B, Lt)}, got {tuple(uncond_text.shape)}")
        nt = uncond_text
    if uncond_style is not None:
        if not isinstance(uncond_style, torch.Tensor) or not uncond_style.dtype.is_floating_point:
            raise ValueError("uncond_style must be a floating-point tensor [B,S,1280]")
        if tuple(uncond_style.shape) != (B, S, 1280):
            raise ValueError(f"uncond_style must be [B,S,1280] = {(B, S, 1280)}, got {tuple(uncond_style.shape)}")
        ns = uncond_style
    dev = next((t.device for t in (text, style_vector, nt, ns) if t.is_cuda), text.device)
    text2 = torch.cat((text.to(dev, torch.int64), nt.to(dev, torch.int64)), dim=0)
    style2 = torch.cat((style_vector.to(dev, torch.float32), ns.to(dev, torch.float32)), dim=0)
    return text2, style2


def _scale_array(scale):
    return (C.c_float * len(scale))(*scale)


def sample(model: DiffusionModel, text: torch.Tensor, style_vector: torch.Tensor, L: int | None = None, T: int = 60,
           diffusion_mode: str = "new", noise: torch.Tensor | None = None, seed: int = 0,
           first_sample: int = 0, lengths=None, known: torch.Tensor | None = None, keep: torch.Tensor | None = None,
           t_start: int | None = None, cond_noise: torch.Tensor | None = None, guidance=None, uncond_text: torch.Tensor | None = None,
           uncond_style: torch.Tensor | None = None) -> torch.Tensor:
    """Reverse-sample a batch.  text int [B,Lt] (0 = pad), style_vector [B,S,1280] -> [B,L,3] = (dx, dy, pen).

    ``lengths`` (optional, B ints, multiples of 8 in [8, L]; ``L`` then defaults to max(lengths)): a ragged batch — prompts
    of different stroke lengths in ONE call.  Row b equals prompt b sampled alone at ``L = lengths[b]`` with
    ``first_sample + b`` (external noise: ``noise[:, b, :lengths[b]]``); rows past lengths[b] are 0.

    ``noise`` (optional, f32 [T+1,B,L,2]): noise[0] = x_T, noise[1+k] = the N(0,1) draw of the k-th loop
    iteration (the reference draws them from torch's global RNG, inference.py:82 / utils/nn.py:86,111).
    Without it the library draws from a counter-based generator keyed by (seed, first_sample + b,
    iteration, position), so any sharding of a prompt batch over GPUs yields the same samples.

    Conditioned sampling (include/dhw.h dhw_sample_cond).  ``known`` f32 [B,L,3] = (dx, dy, pen): strokes
    that exist already.  ``keep`` bool / uint8 [B,L]: rows whose strokes stay exactly as ``known`` gives them (in-painting,
    completion); the model writes the others around them.  ``t_start`` in [1, T] (default T): only the last ``t_start``
    iterations run, from ``known`` noised to that level (restyling: the line keeps its layout, ``style_vector`` decides the
    hand; see ``restyle``).  ``cond_noise`` f32 [T,B,L,2]: the draws that re-noise the kept rows, required exactly when both
    ``noise`` and ``keep`` are given.  Rows of ``known`` that are neither kept nor (``t_start`` < T) seeded are never read.

    Classifier-free guidance (include/dhw.h dhw_guided_sample).  ``guidance``: a scale, or B of them; every step
    asks the denoiser under the real condition and under the guidance condition (``uncond_text`` / ``uncond_style``, each
    defaulting to its half of ``null_condition``; ``uncond_style=style_vector`` guides on the text alone) in ONE forward of 2B
    rows and moves along ``e_c + (guidance - 1) (e_c - e_u)``.  1 is the ordinary sample, 0 the guidance condition's.  The call
    launches eagerly (no graph), draws the same noise as the unguided call, and is refused together with the conditioning
    arguments.  ``None``: today's path, argument for argument.
    """
    if diffusion_mode not in ("new", "standard"):
        raise ValueError("diffusion_mode must be 'new' or 'standard'")
    if guidance is None and (uncond_text is not None or uncond_style is not None):
        raise ValueError("uncond_text / uncond_style belong to a guided call (guidance is None)")
    if guidance is not None:
        given = [k for k, v in (("known", known), ("keep", keep), ("t_start", t_start), ("cond_noise", cond_noise)) if v is not None]
        if given:
            raise ValueError(f"guidance cannot be combined with conditioned sampling ({', '.join(given)})")
        return _sample_guided(model, text, style_vector, L, T, diffusion_mode, noise, seed, first_sample, lengths, guidance, uncond_text, uncond_style)
    B, Lt = text.shape
    lens = None
    if lengths is not None:
        lens = check_lengths(lengths, B, L)
        if L is None:
            L = max(lens)
    if L is None:
        L = stroke_length(Lt)
    if L % 8:
        raise ValueError("L must be a multiple of 8")
    conditioned = known is not None or keep is not None or t_start is not None or cond_noise is not None
    if conditioned:
        t_start = _check_cond(B, L, T, noise, known, keep, t_start, cond_noise)
    with model._device_call("sample", text, (text, style_vector), B, L, style_vector.shape[1]) as c:
        model._apply_teacher()
        t, sv = c.to(text, torch.int64), c.to(style_vector)
        if noise is not None and tuple(noise.shape) != (T + 1, B, L, 2):
            raise ValueError(f"noise must be [T+1,B,L,2] = {(T + 1, B, L, 2)}")
        nz = c.to(noise)
        out = c.empty((B, L, 3))
        head, mode = (t.data_ptr(), sv.data_ptr(), B, L, Lt), 0 if diffusion_mode == "new" else 1
        if conditioned:
            kn, kp, cz = c.to(known), c.to(keep, torch.uint8), c.to(cond_noise)
            c.run("dhw_sample_cond", *head, c.lens(lens), T, mode, c.ptr(nz), seed, first_sample, c.ptr(kn), c.ptr(kp), t_start, c.ptr(cz),
                  out.data_ptr())
        elif lens is None:
            c.run("dhw_sample", *head, T, mode, c.ptr(nz), seed, first_sample, out.data_ptr())
        else:
            c.run("dhw_sample_ragged", *head, c.lens(lens), T, mode, c.ptr(nz), seed, first_sample, out.data_ptr())
    return out.to(text.device)


def _sample_guided(model, text, style_vector, L, T, diffusion_mode, noise, seed, first_sample, lengths, guidance, uncond_text, uncond_style):
    """``sample(..., guidance=...)``: every rule on the host first, then dhw_guided_sample on a handle that holds 2B rows."""
    if not isinstance(text, torch.Tensor) or text.dim() != 2:
        raise ValueError("text must be an integer tensor [B, Lt]")
    B, Lt = text.shape
    lens = _check_ddim_common(text, style_vector, B, lengths, L)
    L, T, seed, first_sample = _check_eager_common(L, lens, Lt, seed, first_sample, lambda: _check_int("T", T, 1, 2 ** 29))
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or not noise.dtype.is_floating_point:
            raise ValueError("noise must be a floating-point tensor [T+1,B,L,2]")
        if tuple(noise.shape) != (T + 1, B, L, 2):
            raise ValueError(f"noise must be [T+1,B,L,2] = {(T + 1, B, L, 2)}")
    scale = _check_guidance(guidance, B)
    text2, style2 = _guided_pair(text, style_vector, uncond_text, uncond_style)
    with model._device_call("guide", text2, (text2, style2) if noise is None else (text2, style2, noise), 2 * B, L, style2.shape[1]) as c:
        t, sv, nz = c.to(text2, torch.int64), c.to(style2), c.to(noise)
        out = c.empty((B, L, 3))
        c.run("dhw_guided_sample", t.data_ptr(), sv.data_ptr(), B, L, Lt, c.lens(lens), T, 0 if diffusion_mode == "new" else 1, _scale_array(scale),
              c.ptr(nz), seed, first_sample, out.data_ptr())
    return out.to(text.device)


def _check_cond(B: int, L: int, T: int, noise, known, keep, t_start, cond_noise) -> int:
    """The conditioning arguments of ``sample``, checked on the host before any device is touched; returns t_start."""
    t_start = _check_int("t_start", T if t_start is None else t_start, 1, T, hi_text=f"T = {T}")
    if known is not None:
        if not isinstance(known, torch.Tensor) or not known.dtype.is_floating_point:
            raise ValueError("known must be a floating-point tensor [B,L,3]")
        if tuple(known.shape) != (B, L, 3):
            raise ValueError(f"known must be [B,L,3] = {(B, L, 3)}, got {tuple(known.shape)}")
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError("keep must be a bool or uint8 tensor [B,L]")
        if tuple(keep.shape) != (B, L):
            raise ValueError(f"keep must be [B,L] = {(B, L)}, got {tuple(keep.shape)}")
        if known is None:
            raise ValueError("keep needs known: the strokes of the kept rows")
    if known is None and t_start != T:
        raise ValueError(f"t_start = {t_start} < T = {T} needs known: the line to start from")
    if cond_noise is not None:
        if not isinstance(cond_noise, torch.Tensor) or not cond_noise.dtype.is_floating_point:
            raise ValueError("cond_noise must be a floating-point tensor [T,B,L,2]")
        if tuple(cond_noise.shape) != (T, B, L, 2):
            raise ValueError(f"cond_noise must be [T,B,L,2] = {(T, B, L, 2)}, got {tuple(cond_noise.shape)}")
        if noise is None or keep is None:
            raise ValueError("cond_noise belongs to calls with external noise and a keep mask (" + ("noise" if noise is None else "keep") + " is missing)")
    elif noise is not None and keep is not None:
        raise ValueError("cond_noise is required when both noise and keep are given ([T,B,L,2])")
    return t_start


def restyle(strokes: torch.Tensor, text: torch.Tensor, style_vector: torch.Tensor, model: DiffusionModel, lengths=None,
            strength: float = 0.5, keep: torch.Tensor | None = None, **sample_kwargs) -> torch.Tensor:
    """Rewrite an existing line in another hand: ``strokes`` [B,L,3] (sampled earlier, or pen data) are noised
    ``strength`` of the way up the schedule, ``t_start = clamp(round(strength * T), 1, T)``, and denoised under
    ``style_vector``.  A small strength keeps the layout and changes details; 1 keeps nothing but the kept rows.  ``keep``
    [B,L] pins rows exactly; the other keywords are ``sample``'s (T, diffusion_mode, seed, ...).  Returns [B,L,3]."""
    if not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"strength = {strength!r} must lie in [0, 1]")
    _check_strokes(strokes)
    T = int(sample_kwargs.pop("T", 60))
    t_start = min(T, max(1, int(round(float(strength) * T))))
    return sample(model, text, style_vector, L=int(strokes.shape[1]), T=T, lengths=lengths, known=strokes, keep=keep, t_start=t_start,
                  **sample_kwargs)


def infer(prompt: str, style_vector: torch.Tensor, model: DiffusionModel, diffusion_mode: str = "new", T: int = 60,
          seed: int = 0, steps: int | None = None, guidance=None, order: int | None = None) -> np.ndarray:
    """Single-prompt convenience wrapper with the reference's front end: tokenise, L = 16 per token rounded up
    to a multiple of 8, sample, return the [L,3] stroke array that the reference hands to ``show_strokes``.
    ``steps``: sample deterministically at that many levels instead (``sample_ddim``; ``diffusion_mode`` then plays no part).
    ``guidance``: a classifier-free guidance scale against ``null_condition`` (``sample`` / ``sample_ddim``); None: unguided.
    ``order`` (with ``steps``): ``sample_ddim``'s solver order, 1 or 2."""
    guided = _guided_kw(guidance, 1, 1)
    guided.update(_order_kw(order, steps))
    ids = Tokenizer().encode(prompt)
    text = torch.tensor([ids], dtype=torch.int64)
    if steps is not None:
        out = sample_ddim(model, text, style_vector, L=stroke_length(len(ids)), T=T, levels=ddim_levels(T, steps), seed=seed, **guided)
        return out[0].detach().cpu().numpy()
    out = sample(model, text, style_vector, L=stroke_length(len(ids)), T=T, diffusion_mode=diffusion_mode, seed=seed, **guided)
    return out[0].detach().cpu().numpy()


def default_levels(T: int = 60) -> list:
    """The noise levels ``score`` evaluates when none are given: four schedule indices spread over the schedule,
    ``(2j+1) * T // 8`` (7, 22, 37, 52 at T = 60; duplicates of a short schedule dropped)."""
    return sorted({(2 * j + 1) * T // 8 for j in range(4)})


def _check_levels(levels, T: int) -> list:
    _check_int("T", T, 1, why="must be a positive integer")
    if levels is None:
        return default_levels(T)
    if isinstance(levels, torch.Tensor):
        levels = levels.detach().cpu().tolist()
    try:
        seq = list(levels)
    except TypeError:
        raise ValueError(f"levels must be a sequence of schedule indices, got {type(levels).__name__}") from None
    if not seq:
        raise ValueError("levels is empty: at least one schedule index is needed")
    if len(seq) > T:
        raise ValueError(f"levels has {len(seq)} entries, more than T = {T}")
    for k, v in enumerate(seq):
        if _check_int(f"levels[{k}]", v) < 0 or v >= T:
            raise ValueError(f"levels[{k}] = {v} must lie in [0, T = {T})")
    return [int(v) for v in seq]


def score(model: DiffusionModel, strokes: torch.Tensor, text: torch.Tensor, style_vector: torch.Tensor, lengths=None, levels=None,
          T: int = 60, noise: torch.Tensor | None = None, seed: int = 0, first_sample: int = 0, pen_round: bool = False) -> torch.Tensor:
    """How well existing strokes fit a text and a hand under the model: the denoising objective (the reference's training
    loss, loss.py:29-37) at chosen noise levels (include/dhw.h dhw_score).  Lower is better.

    strokes f32 [B,L,3] = (dx, dy, pen), text int [B,Lt], style_vector [B,S,1280] -> [B,K,2]: per sample and level the mean
    squared error of the predicted noise and the abar-weighted cross-entropy of the predicted pen lifts, both over the
    sample's own ``lengths[b]`` rows (rows past them are never read).  ``levels``: K schedule indices in [0, T), default
    ``default_levels(T)``.  ``noise`` f32 [K,B,L,2]: the perturbing draws; without it the generator draws them keyed by
    (seed, first_sample + b, position, level), so a level's score depends neither on the other levels nor on sharding.
    ``pen_round``: score against ``torch.round(pen)`` (half to even, the renderer's reading of a sampled pen value)."""
    B, L = _check_strokes(strokes)
    if text.dim() != 2 or text.shape[0] != B:
        raise ValueError(f"text must be [B = {B}, Lt], got {tuple(text.shape)}")
    if L < 8 or L % 8:
        raise ValueError(f"strokes: L = {L} must be a multiple of 8, at least 8")
    lens = check_lengths(lengths, B, L) if lengths is not None else None
    lv = _check_levels(levels, T)
    K, Lt = len(lv), text.shape[1]
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or not noise.dtype.is_floating_point:
            raise ValueError("noise must be a floating-point tensor [K,B,L,2]")
        if tuple(noise.shape) != (K, B, L, 2):
            raise ValueError(f"noise must be [K,B,L,2] = {(K, B, L, 2)}, got {tuple(noise.shape)}")
    with model._device_call("score", text, (strokes, text, style_vector), B, L, style_vector.shape[1]) as c:
        s = strokes.to(c.dev, torch.float32)
        s = c.to(torch.cat((s[..., :2], torch.round(s[..., 2:])), dim=2) if pen_round else s)
        t, sv, nz = c.to(text, torch.int64), c.to(style_vector), c.to(noise)
        out = c.empty((K, B, 2))
        c.run("dhw_score", s.data_ptr(), t.data_ptr(), sv.data_ptr(), B, L, Lt, c.lens(lens), T, c.lens(lv), K, c.ptr(nz), seed, first_sample,
              out.data_ptr())
    return out.transpose(0, 1).to(strokes.device)


# ---------------------------------------------------------------- deterministic sampling and inversion (include/dhw.h dhw_ddim_*)
def ddim_levels(T: int = 60, steps: int | None = None) -> list:
    """The schedule indices ``sample_ddim`` / ``invert`` visit: ``steps`` of them (default T), from T-1 down to 0, evenly
    spread: ``levels[j] = ((steps-1-j) * (T-1)) // (steps-1)``; a single step is ``[T-1]``.  60, 4 -> [59, 39, 19, 0]."""
    T = _check_int("T", T, 1, 2 ** 29)
    steps = T if steps is None else _check_int("steps", steps, 1)
    if steps > T:
        raise ValueError(f"steps = {steps} must lie in [1, T = {T}]")
    if steps == 1:
        return [T - 1]
    return [((steps - 1 - j) * (T - 1)) // (steps - 1) for j in range(steps)]


def _check_ddim_levels(levels, steps, T) -> list:
    """``levels`` as given (checked: integers in [0, T), strictly decreasing, at most T) or ``ddim_levels(T, steps)``."""
    if levels is None:
        return ddim_levels(T, steps)
    if steps is not None:
        raise ValueError("pass steps or levels, not both")
    lv = _check_levels(levels, T)
    for j in range(1, len(lv)):
        if lv[j] >= lv[j - 1]:
            raise ValueError(f"levels[{j}] = {lv[j]} is not below levels[{j - 1}] = {lv[j - 1]}: levels must be strictly decreasing")
    return lv


def _check_order(order) -> int:
    """``order`` of ``sample_ddim``: 1 (DDIM) or 2 (second-order multistep)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or int(order) not in (1, 2):
        raise ValueError(f"order = {order!r} must be 1 (DDIM) or 2 (second-order multistep)")
    return int(order)


def _order_kw(order, steps) -> dict:
    """What a front end passes on for its ``order`` argument: nothing for None (the calls stay as they are, argument for
    argument), else {"order": order}, which needs ``steps``."""
    if order is None:
        return {}
    if steps is None:
        raise ValueError("order belongs to deterministic sampling: pass steps as well")
    return {"order": _check_order(order)}


def _ddim_kw(steps, order, guidance, candidates: int, B: int) -> dict:
    """What a file front end passes on for ``steps``, ``order``, ``guidance``, checked in that order; nothing for a None: today's calls."""
    kw = dict(steps=_check_int("steps", steps, 1)) if steps is not None else {}
    kw.update(_order_kw(order, steps))
    kw.update(_guided_kw(guidance, candidates, B))
    return kw


def _check_ddim_common(text, style_vector, B: int, lengths, L):
    if not isinstance(text, torch.Tensor) or text.dim() != 2 or text.shape[0] != B or text.dtype.is_floating_point:
        raise ValueError(f"text must be an integer tensor [B = {B}, Lt], got {tuple(text.shape) if isinstance(text, torch.Tensor) else type(text).__name__}")
    if not isinstance(style_vector, torch.Tensor) or style_vector.dim() != 3 or style_vector.shape[0] != B or style_vector.shape[2] != 1280:
        raise ValueError(f"style_vector must be a tensor [B = {B}, S, 1280]")
    return check_lengths(lengths, B, L) if lengths is not None else None


def _check_eager_common(L, lens, Lt: int, seed, first_sample, levels_check):
    """What ``sample_ddim`` and ``sample(guidance=...)`` check alike, in their order: L (default: the longest length, else
    ``stroke_length(Lt)``; a multiple of 8), the call's own T / levels check, which stands between them, and the generator's
    ranges.  Returns (L, what ``levels_check()`` returned, seed, first_sample)."""
    if L is None:
        L = max(lens) if lens is not None else stroke_length(Lt)
    L = _check_int("L", L, 8)
    if L % 8:
        raise ValueError(f"L = {L} must be a multiple of 8")
    return L, levels_check(), _check_int("seed", seed, 0, 2 ** 64 - 1), _check_int("first_sample", first_sample, -2 ** 63, 2 ** 63 - 1)


def sample_ddim(model: DiffusionModel, text: torch.Tensor, style_vector: torch.Tensor, L: int | None = None, T: int = 60,
                steps: int | None = None, levels=None, latent: torch.Tensor | None = None, seed: int = 0, first_sample: int = 0,
                lengths=None, return_latent: bool = False, guidance=None, uncond_text: torch.Tensor | None = None,
                uncond_style: torch.Tensor | None = None, order: int = 1):
    """Deterministic (DDIM, eta = 0) sampling over a sub-sequence of the schedule (include/dhw.h dhw_ddim_sample): one
    denoiser call per level and no noise after the start, so the line is a function of its start latent alone.

    ``steps``: how many of the T levels to visit (``ddim_levels(T, steps)``; default all), or ``levels``: the schedule indices
    themselves, strictly decreasing.  ``latent`` f32 [B,L,2]: the start (from ``invert``, ``slerp``, or an earlier call's
    ``return_latent=True``); without it the generator draws the x_T ``sample`` would draw for (seed, first_sample + b).
    ``lengths``: a ragged batch, as in ``sample``.  Returns [B,L,3] = (dx, dy, pen of the last call), or (strokes, latent [B,L,2])
    with ``return_latent=True``.  The calls launch eagerly; they leave ``sample``'s cached graphs and generator state alone.

    ``guidance`` (a scale, or B of them; ``uncond_text`` / ``uncond_style`` as in ``sample``): classifier-free guidance
    (include/dhw.h dhw_guided_ddim_sample) over the same levels, from the same latent; ``None`` is today's call.

    ``order``: 1 (today's call) or 2: the second-order multistep solver (DPM-Solver++ 2M; include/dhw.h dhw_dpm_sample /
    dhw_guided_dpm_sample) over the same levels with the same number of denoiser calls; every step between the
    first and the last also uses the previous step's x0 estimate.  It works with ``guidance``, ``lengths``, ``latent`` and
    ``return_latent``; with one or two levels it returns order 1's bits."""
    order = _check_order(order)
    if not isinstance(text, torch.Tensor) or text.dim() != 2:
        raise ValueError("text must be an integer tensor [B, Lt]")
    if guidance is None and (uncond_text is not None or uncond_style is not None):
        raise ValueError("uncond_text / uncond_style belong to a guided call (guidance is None)")
    B, Lt = text.shape
    if latent is not None:
        if not isinstance(latent, torch.Tensor) or not latent.dtype.is_floating_point:
            raise ValueError("latent must be a floating-point tensor [B,L,2]")
        if latent.dim() != 3 or latent.shape[0] != B or latent.shape[2] != 2 or (L is not None and latent.shape[1] != L):
            raise ValueError(f"latent must be [B,L,2] = {(B, L if L is not None else 'L', 2)}, got {tuple(latent.shape)}")
        L = int(latent.shape[1])
    lens = _check_ddim_common(text, style_vector, B, lengths, L)
    L, lv, seed, first_sample = _check_eager_common(L, lens, Lt, seed, first_sample, lambda: _check_ddim_levels(levels, steps, T))
    # a guided call: the entry's name, the doubled condition (2B rows on the handle) and the scale array; text2 / style2 are the call's own otherwise
    scale = _check_guidance(guidance, B) if guidance is not None else None
    text2, style2 = _guided_pair(text, style_vector, uncond_text, uncond_style) if scale is not None else (text, style_vector)
    tensors = (text2, style2) if latent is None else (text2, style2, latent)
    with model._device_call("ddim" if scale is None else "guide", text2, tensors, B if scale is None else 2 * B, L, style2.shape[1]) as c:
        t, sv, lat = c.to(text2, torch.int64), c.to(style2), c.to(latent)
        lat_out, out = c.empty((B, L, 2), wanted=return_latent), c.empty((B, L, 3))
        head = (t.data_ptr(), sv.data_ptr(), B, L, Lt, c.lens(lens), T, c.lens(lv), len(lv))
        if order != 1:
            head, ddim, guided = head + (order,), "dhw_dpm_sample", "dhw_guided_dpm_sample"
        else:
            ddim, guided = "dhw_ddim_sample", "dhw_guided_ddim_sample"
        if scale is None:
            c.run(ddim, *head, c.ptr(lat), seed, first_sample, c.ptr(lat_out), out.data_ptr())
        else:
            c.run(guided, *head, _scale_array(scale), c.ptr(lat), seed, first_sample, out.data_ptr(), c.ptr(lat_out))
    return (out.to(text.device), lat_out.to(text.device)) if return_latent else out.to(text.device)


def invert(model: DiffusionModel, strokes: torch.Tensor, text: torch.Tensor, style_vector: torch.Tensor, lengths=None, T: int = 60,
           steps: int | None = None, levels=None, iters: int = 1) -> torch.Tensor:
    """The latent an existing line came from (include/dhw.h dhw_ddim_invert): the deterministic process of ``sample_ddim`` run
    backwards over the same levels, from ``strokes`` [B,L,3] (sampled, or pen data; the pen column is not read) up to x_T.
    ``sample_ddim(latent=invert(x))`` under the same text, style and levels reproduces ``x`` to an error the tests measure;
    under another style or text it rewrites the line reproducibly (``transfer``).  ``iters`` in [1, 8]: fixed-point
    iterations per step (1 = the usual DDIM inversion); the call makes ``len(levels) * iters`` denoiser calls.
    Returns the latent [B,L,2], 0 past ``lengths[b]``.  There is no ``order``: a multistep step uses the step before it, so it
    has no one-step inverse; the inversion is of the first-order process (``sample_ddim(order=1)``)."""
    B, L = _check_strokes(strokes)
    if L < 8 or L % 8:
        raise ValueError(f"strokes: L = {L} must be a multiple of 8, at least 8")
    lens = _check_ddim_common(text, style_vector, B, lengths, L)
    lv = _check_ddim_levels(levels, steps, T)
    iters = _check_int("iters", iters, 1, 8)
    Lt = text.shape[1]
    with model._device_call("ddim", text, (strokes, text, style_vector), B, L, style_vector.shape[1]) as c:
        s, t, sv = c.to(strokes), c.to(text, torch.int64), c.to(style_vector)
        out = c.empty((B, L, 2))
        c.run("dhw_ddim_invert", s.data_ptr(), t.data_ptr(), sv.data_ptr(), B, L, Lt, c.lens(lens), T, c.lens(lv), len(lv), iters, out.data_ptr())
    return out.to(strokes.device)


def transfer(strokes: torch.Tensor, text: torch.Tensor, style_from: torch.Tensor, style_to: torch.Tensor, model: DiffusionModel,
             lengths=None, text_to: torch.Tensor | None = None, **kw) -> torch.Tensor:
    """Rewrite an existing line reproducibly: invert ``strokes`` under ``(text, style_from)``, then ``sample_ddim`` that latent
    under ``(text_to or text, style_to)``.  Keywords: T, steps, levels (both halves), iters (the inversion).  Returns [B,L,3],
    the pen from the last denoiser call.  Unlike ``restyle`` nothing is random and no strength is chosen.  There is no ``order``:
    both halves are the first-order process, because a multistep step has no one-step inverse (``invert``)."""
    iters = kw.pop("iters", 1)
    extra = set(kw) - {"T", "steps", "levels"}
    if extra:
        raise ValueError(f"transfer: unknown keyword(s) {sorted(extra)} (T, steps, levels, iters)")
    if text_to is not None and (not isinstance(text_to, torch.Tensor) or text_to.dim() != 2 or text_to.shape[0] != text.shape[0]):
        raise ValueError("text_to must be an integer tensor [B, Lt']")
    if not isinstance(style_to, torch.Tensor) or style_to.dim() != 3 or style_to.shape[0] != strokes.shape[0] or style_to.shape[2] != 1280:
        raise ValueError(f"style_to must be a tensor [B = {strokes.shape[0]}, S, 1280]")
    latent = invert(model, strokes, text, style_from, lengths=lengths, iters=iters, **kw)
    return sample_ddim(model, text if text_to is None else text_to, style_to, latent=latent, lengths=lengths, **kw)


def slerp(latent_a: torch.Tensor, latent_b: torch.Tensor, w, lengths=None) -> torch.Tensor:
    """Spherical interpolation of two latents [B,L,2], per sample over its own ``lengths[b]`` rows (rows past them are 0):
    ``sin((1-w) t)/sin(t) a + sin(w t)/sin(t) b`` with t the angle between the flattened a and b; nearly parallel latents
    (sin t < 1e-6) are interpolated linearly.  ``w``: a number, or B of them.  Plain torch on the latents' device."""
    for name, x in (("latent_a", latent_a), ("latent_b", latent_b)):
        if not isinstance(x, torch.Tensor) or not x.dtype.is_floating_point or x.dim() != 3 or x.shape[2] != 2:
            raise ValueError(f"{name} must be a floating-point tensor [B,L,2]")
    if latent_a.shape != latent_b.shape:
        raise ValueError(f"latent_a {tuple(latent_a.shape)} and latent_b {tuple(latent_b.shape)} differ in shape")
    B, L, _ = latent_a.shape
    lens = check_lengths(lengths, B, L) if lengths is not None else [L] * B
    wt = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
    if wt.numel() not in (1, B) or not torch.isfinite(wt).all():
        raise ValueError(f"w must be a finite number or {B} of them")
    wt = wt.expand(B).tolist()
    out = torch.zeros_like(latent_a)
    for b, n in enumerate(lens):
        a, c = latent_a[b, :n].float(), latent_b[b, :n].float()
        cos = (a * c).sum() / (a.norm() * c.norm()).clamp_min(1e-30)
        t = torch.acos(cos.clamp(-1.0, 1.0))
        st = torch.sin(t)
        if st.item() < 1e-6:
            r = (1.0 - wt[b]) * a + wt[b] * c
        else:
            r = torch.sin((1.0 - wt[b]) * t) / st * a + torch.sin(wt[b] * t) / st * c
        out[b, :n] = r.to(out.dtype)
    return out


# ---------------------------------------------------------------- attention maps and alignment (include/dhw.h dhw_attention)
def _check_attention_args(model: DiffusionModel, strokes, text, sigma, style_vector, lengths, layer):
    """Every argument of ``attention``, checked on the host before any device is touched; returns (lens or None, layer index)."""
    if not isinstance(strokes, torch.Tensor) or not strokes.dtype.is_floating_point:
        raise ValueError("strokes must be a floating-point tensor [B,L,2]")
    if not isinstance(sigma, torch.Tensor) or not isinstance(style_vector, torch.Tensor):
        raise ValueError("sigma and style_vector must be tensors")
    B, L = model._check_forward_inputs(strokes, text, sigma, style_vector)
    if text.dtype.is_floating_point or text.dtype == torch.bool:
        raise ValueError(f"text must hold integer token ids, got {text.dtype}")
    lens = check_lengths(lengths, B, L) if lengths is not None else None
    if model.training or (torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())):
        raise ValueError("attention maps are inference-only (eval() and no gradient recording)")
    return lens, attention_layer_index(layer, model.num_layers)


def attention(model: DiffusionModel, strokes: torch.Tensor, text: torch.Tensor, sigma: torch.Tensor, style_vector: torch.Tensor,
              lengths=None, layer=-1, heads: bool = False):
    """Which text token each stroke row attends to, in one denoiser call (include/dhw.h dhw_attention).

    strokes f32 [B,L,2], text int [B,Lt] (0 = pad), sigma [B] / [B,1] / [B,1,1], style_vector [B,S,1280] ->
    ``(mean [B,Lq,Lt], token [B,Lq] int32)``, and ``probs [B,H,Lq,Lt]`` as a third element with ``heads=True``.  ``layer``:
    an index (0 = enc3 with Lq = L/2, 1 = enc5 with L/4, 2 + i = att_layers.i with L/8; negative from the end, the default -1
    is the last attention layer) or the module's name.  ``mean`` is the mean of the heads' probabilities, ``token`` its first
    argmax.  ``lengths``: a ragged batch, as in ``forward``; rows past a sample's end are 0 / -1."""
    lens, li = _check_attention_args(model, strokes, text, sigma, style_vector, lengths, layer)
    if not isinstance(heads, (bool, np.bool_)):
        raise ValueError(f"heads = {heads!r} must be a bool")
    ret_dev = strokes.device
    _, _, probs, mean, token = model._attention_call(strokes, text, sigma, style_vector, lens, li, bool(heads), True, True)
    out = (mean.to(ret_dev), token.to(ret_dev))
    return out + (probs.to(ret_dev),) if heads else out


def token_spans(token, Lt: int) -> list:
    """Per prompt, per token k < Lt: ``(first_row, last_row + 1)`` of the rows of ``token`` [B,L] that name k, or None for a
    token that never wins.  (A token's rows need not be contiguous: the span is their hull.)"""
    tk = np.asarray(token.detach().cpu() if isinstance(token, torch.Tensor) else token)
    out = []
    for row in tk:
        spans = []
        for k in range(int(Lt)):
            idx = np.flatnonzero(row == k)
            spans.append((int(idx[0]), int(idx[-1]) + 1) if idx.size else None)
        out.append(spans)
    return out


class Alignment:
    """What ``align`` returns: ``mean`` [B,Lq,Lt] (the layer's head-mean attention), ``token`` [B,L] int32 (the winning token
    of every stroke row, -1 past the sample's length), ``spans`` (``token_spans(token, Lt)``), ``lengths`` (list or None),
    ``layer`` (library index)."""

    def __init__(self, mean, token, spans=None, lengths=None, layer=None):
        self.mean, self.token, self.lengths, self.layer = mean, token, lengths, layer
        self.spans = spans if spans is not None else token_spans(token, mean.shape[-1] if mean is not None else int(token.max()) + 1)


def align(model: DiffusionModel, strokes: torch.Tensor, text: torch.Tensor, style_vector: torch.Tensor, lengths=None, level: int = 0,
          T: int = 60, layer=-1) -> Alignment:
    """Where in a line each character sits: the attention map of ``strokes`` [B,L,3] (a sampled line, or pen data) under
    their ``text``.  The denoiser runs once on ``strokes[..., :2]`` as given — no noise is added — at
    ``sigma = sqrt(abar[level])`` of the T-step schedule (level 0: the nearly clean end).  Returns an ``Alignment``."""
    B, L = _check_strokes(strokes)
    T = _check_int("T", T, 1, why="must be a positive integer")
    level = _check_int("level", level, 0, T - 1, why=f"must be an integer in [0, T = {T})")
    xy = strokes[..., :2]
    sigma = torch.full((B,), float(np.sqrt(_lib.schedule(T)[1][level])), dtype=torch.float32)
    lens, li = _check_attention_args(model, xy, text, sigma, style_vector, lengths, layer)
    ret_dev = strokes.device
    _, _, _, mean, token = model._attention_call(xy, text, sigma, style_vector, lens, li, False, True, True)
    mean, token = mean.to(ret_dev), token.to(ret_dev)
    full = token.repeat_interleave(L // token.shape[1], dim=1)   # (rows past a length are -1 already: lengths are multiples of 8)
    return Alignment(mean, full, token_spans(full, text.shape[1]), lens, li)


def align_monotone(alignment: Alignment, text: torch.Tensor) -> Alignment:
    """``alignment`` read monotonically: the same ``mean``, with ``token`` replaced by ``truth.monotone_tokens`` (the best
    non-decreasing token sequence under the map, decoded on the host) repeated to the L stroke rows, and ``spans`` recomputed, so
    that every token's rows are one contiguous span and the spans are in text order.  ``text`` int [B,Lt] (0 = pad): line b has
    as many tokens as it has non-zero ids.  ``align`` picks each row's token on its own; this is the reading to build word and
    character boxes on (``truth.page_truth``)."""
    from .truth import monotone_tokens

    mean, token = alignment.mean, alignment.token
    if not isinstance(mean, torch.Tensor) or mean.dim() != 3 or not isinstance(token, torch.Tensor) or token.dim() != 2:
        raise ValueError("alignment must hold mean [B,Lq,Lt] and token [B,L] tensors")
    B, Lq, Lt = mean.shape
    if not isinstance(text, torch.Tensor) or tuple(text.shape) != (B, Lt) or text.dtype.is_floating_point or text.dtype == torch.bool:
        raise ValueError(f"text must hold integer token ids [B, Lt] = [{B}, {Lt}]")
    L = int(token.shape[1])
    if token.shape[0] != B or L % Lq:
        raise ValueError(f"alignment.token {tuple(token.shape)} does not go with mean {tuple(mean.shape)}")
    n_tokens = [int(v) for v in (text != 0).sum(1).cpu().tolist()]
    if min(n_tokens) < 1:
        raise ValueError("every prompt needs at least one token")
    rep = L // Lq
    rows = None if alignment.lengths is None else [int(n) // rep for n in alignment.lengths]
    full = monotone_tokens(mean, n_tokens, rows).to(token.device).repeat_interleave(rep, dim=1)
    return Alignment(mean, full, token_spans(full, Lt), alignment.lengths, alignment.layer)


def rewrite_mask(alignment: Alignment, tok_lo, tok_hi) -> torch.Tensor:
    """The ``keep`` mask [B,L] (bool) that rewrites tokens [tok_lo, tok_hi) of every line and pins the rest: True inside the
    sample's length where the row's token lies outside the range, False on the rows to rewrite and past the length — ready
    for ``sample(..., known=strokes, keep=mask)``.  ``tok_lo`` / ``tok_hi``: ints, or one per prompt."""
    token = alignment.token
    if not isinstance(token, torch.Tensor) or token.dim() != 2:
        raise ValueError("alignment.token must be a tensor [B,L]")
    B, L = token.shape

    def per_prompt(v, name):
        seq = [v] * B if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) else v
        try:
            seq = list(seq)
        except TypeError:
            raise ValueError(f"{name} = {v!r} must be an integer or one integer per prompt") from None
        if len(seq) != B:
            raise ValueError(f"{name} has {len(seq)} entries, the batch {B}")
        for i, x in enumerate(seq):
            _check_int(f"{name}[{i}]", x)
        return torch.tensor([int(x) for x in seq], dtype=torch.int64, device=token.device)[:, None]

    lo, hi = per_prompt(tok_lo, "tok_lo"), per_prompt(tok_hi, "tok_hi")
    if bool((lo > hi).any()) or bool((lo < 0).any()):
        raise ValueError("tok_lo / tok_hi: every range must satisfy 0 <= tok_lo <= tok_hi")
    tk = token.to(torch.int64)
    inside = torch.ones((B, L), dtype=torch.bool, device=token.device)
    if alignment.lengths is not None:
        lens = torch.tensor([int(n) for n in alignment.lengths], dtype=torch.int64, device=token.device)[:, None]
        inside = torch.arange(L, device=token.device)[None, :] < lens
    return inside & (tk >= 0) & ((tk < lo) | (tk >= hi))


def align_file(prompts, strokes_path, source, config_path: str | None = None, checkpoint_path: str | None = None,
               experiment_path: str | None = None, *, precision: str = "bf16", style_weights: str | None = None, level: int = 0,
               layer=-1):
    """``infer.py --align``: the lines of ``prompts`` as an earlier run wrote them (``strokes_path``: the .npy of ``infer.py
    --save-strokes``) aligned to their text by one ``align`` call.  Returns (the Alignment on the host, the prompts' token
    id lists, the stroke lengths)."""
    model, old, text, sv, lens = _open_lines("align_file", prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, precision,
                                             style_weights)
    al = align(model, old, text, sv, lengths=lens, level=level, layer=layer)
    al.mean, al.token = al.mean.detach().cpu(), al.token.detach().cpu()
    return al, [[int(v) for v in row if int(v) != 0] for row in text.cpu().tolist()], lens


def _encode_batch(who: str, prompts, style_vector):
    """(text int64 [B,Lt] padded with 0, each prompt's own stroke length, style_vector expanded to [B,S,1280])."""
    prompts = list(prompts)
    if not prompts:
        raise ValueError(f"{who}: no prompts")
    tok = Tokenizer()
    ids = [tok.encode(p) for p in prompts]
    if any(len(i) == 0 for i in ids):
        raise ValueError(f"{who}: every prompt needs at least one token")
    B, Lt = len(ids), max(len(i) for i in ids)
    text = torch.zeros((B, Lt), dtype=torch.int64)
    for b, i in enumerate(ids):
        text[b, :len(i)] = torch.tensor(i, dtype=torch.int64)
    lens = [stroke_length(len(i)) for i in ids]
    sv = torch.as_tensor(style_vector)
    if sv.dim() != 3 or sv.shape[0] not in (1, B):
        raise ValueError(f"style_vector must be [1,S,1280] or [B={B},S,1280], got {tuple(sv.shape)}")
    if sv.shape[0] != B:
        sv = sv.expand(B, -1, -1)
    if sv.is_cuda:
        text = text.to(sv.device)
    return text, lens, sv


def infer_batch(prompts, style_vector: torch.Tensor, model: DiffusionModel, diffusion_mode: str = "new", T: int = 60,
                seed: int = 0, first_sample: int = 0, candidates: int = 1, levels=None, steps: int | None = None, guidance=None,
                order: int | None = None) -> list:
    """Many prompts in ONE ragged sampler call: prompt i is tokenised, gets its own ``L_i = stroke_length(n_i)`` and is padded
    with token 0 to the longest prompt.  ``style_vector`` is [1,S,1280] (one writer for every prompt) or [B,S,1280].  Returns a
    list of [L_i, 3] arrays; entry i equals ``sample(model, text_i, style_i, L=L_i, seed=seed, first_sample=first_sample + i)``.

    ``candidates = N > 1`` (best of N): every prompt is sampled N times — candidate j of prompt b is the sample with generator
    index ``first_sample + j*B + b``, so candidate 0 is the line above — and scored by ``score(..., pen_round=True)`` at
    ``levels``; the line returned for a prompt is the candidate with the lowest mean over levels of score term + pen term
    (ties: the lower j).

    ``steps``: every line is sampled deterministically at that many levels (``sample_ddim`` with ``ddim_levels(T, steps)``)
    instead; ``diffusion_mode`` then plays no part.  ``order`` (with ``steps``): ``sample_ddim``'s solver order, 1 or 2.

    ``guidance``: a classifier-free guidance scale, or one per prompt, against ``null_condition`` (each call is then one forward
    of 2B rows per step); refused together with ``candidates > 1``."""
    candidates = _check_candidates(candidates)
    guided = _guided_kw(guidance, candidates)
    solver = _order_kw(order, steps)
    if steps is None:
        def draw(tx, st, ln, first):
            return sample(model, tx, st, L=max(lens), T=T, diffusion_mode=diffusion_mode, seed=seed, first_sample=first, lengths=ln, **guided)
    else:
        ddim = ddim_levels(T, steps)

        def draw(tx, st, ln, first):
            return sample_ddim(model, tx, st, L=max(lens), T=T, levels=ddim, seed=seed, first_sample=first, lengths=ln, **guided, **solver)
    text, lens, sv = _encode_batch("infer_batch", prompts, style_vector)
    B = len(lens)
    if candidates == 1:
        out = draw(text, sv, lens, first_sample)
        out = out.detach().cpu().numpy()
        return [out[b, :lens[b]].copy() for b in range(B)]
    lv = _check_levels(levels, T)
    # whole candidate rounds per call, as many as the model's batch capacity holds: row j*B + b of the stacked batch is
    # candidate j of prompt b.  Every row is its alone run bit for bit, so the split changes nothing.
    per = max(1, max(B, int(model._cap["max_B"])) // B)
    best, best_total = [None] * B, [float("inf")] * B
    for j0 in range(0, candidates, per):
        r = min(per, candidates - j0)
        tx, st, ln = text.repeat(r, 1), sv.repeat(r, 1, 1), lens * r
        first = first_sample + j0 * B
        out = draw(tx, st, ln, first)
        sc = score(model, out, tx, st, lengths=ln, levels=lv, T=T, seed=seed, first_sample=first, pen_round=True)
        total = sc.detach().cpu().double().sum(dim=2).mean(dim=1).tolist()   # (on the host in fp64: the ranking is the same everywhere)
        out = out.detach().cpu().numpy()
        for j in range(r):
            for b in range(B):
                if total[j * B + b] < best_total[b]:
                    best_total[b], best[b] = total[j * B + b], out[j * B + b, :lens[b]].copy()
    if any(x is None for x in best):
        raise RuntimeError("infer_batch: a prompt has no finite candidate score")
    return best


def _check_candidates(candidates) -> int:
    return _check_int("candidates", candidates, 1, why="must be an integer >= 1")


def remove_whitespace(img: np.ndarray, thresh: float) -> np.ndarray:
    """Crop to the rows / columns that hold a pixel darker than `thresh` (reference utils/preprocessing.py:47-62, the
    `remove_middle=False` branch, including its exclusive upper bounds: the last inked row and column are dropped)."""
    rows = np.nonzero(np.amin(img, axis=1) < thresh)[0]
    cols = np.nonzero(np.amin(img, axis=0) < thresh)[0]
    return img[rows[0]:rows[-1], cols[0]:cols[-1]]


def _resize_cubic(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """uint8 bicubic resize with OpenCV's INTER_CUBIC conventions (Keys kernel a = -0.75, pixel centres aligned by
    (dst + 0.5) * scale - 0.5, replicated border, no antialiasing), separable, float accumulation, round + saturate.
    PARITY UNPINNED: cv2 is not importable here, its fixed-point rounding may differ in the last grey level."""
    def taps(n_in, n_out):
        x = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        x0 = np.floor(x).astype(np.int64)
        t = x - x0
        a = -0.75
        w = np.stack([((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a,
                      ((a + 2) * t - (a + 3)) * t * t + 1,
                      ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1,
                      ((a * (2 - t) - 5 * a) * (2 - t) + 8 * a) * (2 - t) - 4 * a], axis=1)
        idx = np.clip(x0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
        return idx, w
    f = img.astype(np.float64)
    idx, w = taps(f.shape[1], out_w)
    f = (f[:, idx] * w[None]).sum(-1)
    idx, w = taps(f.shape[0], out_h)
    f = (f[idx] * w[:, :, None]).sum(1)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def read_img(path, height: int = 96) -> np.ndarray:
    """Load a handwriting image as grey levels, crop the white margins and resize to `height` rows keeping the aspect
    ratio (reference utils/io.py:98-115: cv2.imread(GRAYSCALE) -> remove_whitespace(thresh=127) -> cv2.resize(INTER_CUBIC))."""
    from PIL import Image
    img = np.asarray(Image.open(str(path)).convert("L"))
    img = remove_whitespace(img, thresh=127)
    h, w = img.shape
    return _resize_cubic(img, height * w // h, height)


_IMAGE_SUFFIXES = (".png", ".tif", ".tiff", ".jpg", ".jpeg", ".bmp", ".gif")
_extractors = {}


def load_style(source, style_weights=None) -> torch.Tensor:
    """The writer-style features of a prompt, [1,S,1280].  `source` is what the reference's `infer` takes — the path of a
    handwriting image, run through `read_img(source, 96)` and the StyleExtractor (inference.py:66-70, text_style.py:43-59;
    `style_weights` = a local torchvision MobileNetV2 state_dict file, without it the extractor is random-initialised) —
    or features computed elsewhere: a tensor / array, or a file holding one (.npy, or .pt read with weights_only=True)."""
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        path = str(source)
        if path.lower().endswith(_IMAGE_SUFFIXES):
            from .style_extractor import StyleExtractor
            key = str(style_weights)
            if key not in _extractors:
                _extractors[key] = StyleExtractor(style_weights, precision="fp32")
            return _extractors[key](read_img(path, 96)[None, None, :])
        if path.endswith(".npy"):
            source = np.load(path, allow_pickle=False)
        elif path.endswith((".pt", ".pth")):
            source = torch.load(path, map_location="cpu", weights_only=True)
        else:
            raise ValueError(f"{path}: pass a handwriting image ({', '.join(_IMAGE_SUFFIXES)}) or style features ([S,1280], .npy / .pt)")
    sv = torch.as_tensor(source, dtype=torch.float32)
    if sv.dim() == 2:
        sv = sv[None]
    if sv.dim() != 3 or sv.shape[0] != 1 or sv.shape[2] != 1280:
        raise ValueError(f"style features must be [S,1280] or [1,S,1280], got {tuple(sv.shape)}")
    return sv


RENDERERS = ("matplotlib", "gpu")


def _check_renderer(renderer: str) -> None:
    if renderer not in RENDERERS:
        raise ValueError(f"renderer must be one of {RENDERERS}, got {renderer!r}")


def infer_file(prompt: str, source, config_path: str | None = None, checkpoint_path: str | None = None,
               experiment_path: str | None = None, output: str = "result", diffusion_mode: str = "new", *, precision: str = "bf16",
               seed: int = 0, render: bool = True, style_weights: str | None = None, renderer: str = "matplotlib",
               candidates: int = 1, steps: int | None = None, guidance=None, order: int | None = None) -> np.ndarray:
    """The reference's command-line entry (inference.py:19-27) around this build's sampler: resolve config / checkpoint
    (directly or inside ``experiment_path``), load the model, sample one prompt, write ``./<output>.png`` (``renderer``:
    "matplotlib" = the reference's figure, "gpu" = the 96-row grey line image of ``render_strokes``).
    ``candidates = N > 1``: the best of N samples by ``score`` (``infer_batch``).  ``steps``: deterministic sampling at that
    many levels (``sample_ddim``), ``order`` its solver order.  ``guidance``: a classifier-free guidance scale (``sample``).
    Returns the [L,3] strokes."""
    from .checkpoint import load_model

    _check_renderer(renderer)
    candidates = _check_candidates(candidates)
    ddim = _ddim_kw(steps, order, guidance, candidates, 1)
    config_path, checkpoint_path = _resolve_experiment(config_path, checkpoint_path, experiment_path)
    style = load_style(source, style_weights)
    model = load_model(config_path, checkpoint_path, precision=precision, max_B=2 if guidance is not None else _rounds_capacity(1, candidates),
                       style_rows=style.shape[1])
    if candidates > 1:
        (strokes,) = infer_batch([prompt], style, model, diffusion_mode=diffusion_mode, seed=seed, candidates=candidates, **ddim)
    else:
        strokes = infer(prompt, style, model, diffusion_mode=diffusion_mode, seed=seed, **ddim)
    if render:
        _save_lines([strokes], [output], renderer)
    return strokes


def _rounds_capacity(B: int, candidates: int, limit: int = 64) -> int:
    """Batch capacity for best-of-N over B prompts: as many whole candidate rounds as fit under ``limit`` rows, at least one."""
    return B * max(1, min(candidates, limit // B))


def _resolve_experiment(config_path, checkpoint_path, experiment_path):
    from .checkpoint import find_checkpoint
    if experiment_path:
        from pathlib import Path
        if not config_path:
            config_path = str(Path(experiment_path) / "config.yml")
        if not checkpoint_path:
            ckpt = find_checkpoint(experiment_path)
            checkpoint_path = str(ckpt) if ckpt else None
    if not config_path or not checkpoint_path:
        raise ValueError("Both config_path and checkpoint_path must be provided, either directly or via experiment_path.")
    return config_path, checkpoint_path


def _save_lines(strokes, names, renderer: str) -> None:
    """``./<name>.png`` per line: "gpu" rasterises every line in one ``render_strokes`` call, "matplotlib" draws the reference's figure."""
    from .vis import render_lines_png, show_strokes
    if renderer == "gpu":
        render_lines_png(strokes, names)
    else:
        for s, name in zip(strokes, names):
            show_strokes(s, scale=1, name=name, show_output=False)


def _open_lines(who: str, prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, precision, style_weights):
    """What the front ends that read back saved lines open with -> (model sized for the batch, strokes [B, max L_i, 3], text, style
    [B,S,1280], stroke lengths)."""
    from .checkpoint import load_model
    config_path, checkpoint_path = _resolve_experiment(config_path, checkpoint_path, experiment_path)
    style = load_style(source, style_weights)
    text, lens, sv = _encode_batch(who, list(prompts), style)
    old = _load_strokes(strokes_path, lens)
    model = load_model(config_path, checkpoint_path, precision=precision, max_B=len(lens), style_rows=style.shape[1])
    return model, old, text, sv, lens


def infer_file_batch(prompts, source, config_path: str | None = None, checkpoint_path: str | None = None,
                     experiment_path: str | None = None, output: str = "result", diffusion_mode: str = "new", *,
                     precision: str = "bf16", seed: int = 0, render: bool = True, style_weights: str | None = None,
                     renderer: str = "matplotlib", candidates: int = 1, steps: int | None = None, guidance=None,
                     order: int | None = None) -> list:
    """``infer_file`` for many prompts of one writer: one ragged sampler call (``infer_batch``), ``./<output>_<i>.png`` per
    prompt (``renderer="gpu"``: every line rasterised in one ``render_strokes`` call).  ``candidates = N > 1``: every line is
    the best of N samples by ``score``.  ``steps`` / ``order``: deterministic sampling at that many levels (``sample_ddim``).  ``guidance``: a
    classifier-free guidance scale, or one per prompt (``infer_batch``).  Returns the list of [L_i, 3] strokes."""
    from .checkpoint import load_model

    _check_renderer(renderer)
    candidates = _check_candidates(candidates)
    prompts = list(prompts)
    ddim = _ddim_kw(steps, order, guidance, candidates, max(1, len(prompts)))
    config_path, checkpoint_path = _resolve_experiment(config_path, checkpoint_path, experiment_path)
    style = load_style(source, style_weights)
    model = load_model(config_path, checkpoint_path, precision=precision,
                       max_B=_rounds_capacity(max(1, len(prompts)), candidates) * (2 if guidance is not None else 1), style_rows=style.shape[1])
    strokes = infer_batch(prompts, style, model, diffusion_mode=diffusion_mode, seed=seed, candidates=candidates, **ddim)
    if render:
        _save_lines(strokes, [f"{output}_{i}" for i in range(len(strokes))], renderer)
    return strokes


WRAP_MAX_CHARS = 48   # the model's text cap: the reference's dataset drops lines with len(text) >= max_text_len = 50


def wrap_text(text: str, max_chars: int = 40):
    """Greedy word wrap of a text to lines of at most ``max_chars`` characters -> (lines, slots).

    Every line of ``text`` is wrapped on its own (a newline always ends a line); words are what whitespace separates and are
    joined by one space; a word longer than ``max_chars`` is split hard into pieces of ``max_chars``.  ``slots[i]`` is the
    slot ``render_page`` draws ``lines[i]`` in: consecutive, except that a blank line of the input skips one slot (a
    paragraph gap).  ``max_chars`` in [1, 48]."""
    if not isinstance(text, str):
        raise ValueError(f"text must be a str, got {type(text).__name__}")
    max_chars = _check_int("max_chars", max_chars, 1, WRAP_MAX_CHARS)
    lines, slots, slot = [], [], 0
    for raw in text.split("\n"):
        words = raw.split()
        if not words:
            slot += 1
            continue
        cur = ""
        for w in words:
            if cur and len(cur) + 1 + len(w) <= max_chars:
                cur += " " + w
                continue
            if cur:
                lines.append(cur)
            while len(w) > max_chars:
                lines.append(w[:max_chars])
                w = w[max_chars:]
            cur = w
        lines.append(cur)
        slots.extend(range(slot, slot + len(lines) - len(slots)))
        slot = slots[-1] + 1
    return lines, slots


def _round_size(model: DiffusionModel, guided: bool = False) -> int:
    """Lines per round of ``write_page`` and of the alignment of ``write_page_file``: the model's batch capacity, halved for a
    guided round (one forward of twice its lines)."""
    return max(1, int(model._cap["max_B"]) // (2 if guided else 1))


def write_page(text: str, style_vector: torch.Tensor, model: DiffusionModel, *, max_chars: int = 40, diffusion_mode: str = "new",
               T: int = 60, seed: int = 0, first_sample: int = 0, candidates: int = 1, levels=None, steps: int | None = None,
               guidance=None, order: int | None = None, pages=None, height: int = 1980, width: int = 1400, lines_per_page: int = 20, margin_left: float = 70.0,
               margin_top: float = 70.0, pitch: float = 92.0, line_width: float = 2.0, scale=None):
    """Write a text: ``wrap_text`` to lines, ``infer_batch`` for their strokes, ``render_page`` onto pages at one shared scale.

    ``style_vector`` is [1,S,1280] (one writer).  The lines are sampled in rounds of at most the model's batch capacity
    (``max_B``): the round that starts at line i0 is ``infer_batch(..., first_sample=first_sample + i0 * candidates)``, so with
    ``candidates = 1`` line i uses generator index ``first_sample + i`` however the rounds fall, and the rounds of a best-of-N
    run never share an index.  ``guidance`` (one scale for every line): a guided round is one forward of twice its lines, so the
    rounds are half as long.  ``order`` (with ``steps``): ``sample_ddim``'s solver order.  The sampler arguments are ``infer_batch``'s, the page arguments ``render_page``'s; all are
    checked, with ValueError, before a device is touched.

    Returns (pages f32 [P,1,height,width] on the GPU, the list of [L_i,3] stroke arrays, one per wrapped line)."""
    from .vis import check_page_geometry, render_page

    lines, slots = wrap_text(text, max_chars)
    if not lines:
        raise ValueError("write_page: the text holds no word")
    candidates = _check_candidates(candidates)
    T = _check_int("T", T, 1)
    first_sample = _check_int("first_sample", first_sample, 0)
    if steps is not None:
        ddim_levels(T, steps)
    solver = _order_kw(order, steps)
    if candidates > 1:
        _check_levels(levels, T)
    guided = _guided_kw(guidance, candidates, 1)
    if diffusion_mode not in ("new", "standard"):
        raise ValueError(f"diffusion_mode must be 'new' or 'standard', got {diffusion_mode!r}")
    g = check_page_geometry(pages, height, width, lines_per_page, margin_left, margin_top, pitch, line_width, scale)
    if g["pages"] is None:
        check_page_geometry(slots[-1] // g["lines_per_page"] + 1, height, width, lines_per_page, margin_left, margin_top, pitch, line_width, scale)
    sv = torch.as_tensor(style_vector)
    if sv.dim() != 3 or sv.shape[0] != 1:
        raise ValueError(f"style_vector must be [1,S,1280], got {tuple(sv.shape)}")
    _encode_batch("write_page", lines, sv)   # (an empty or untokenisable line is refused here, before the first round)

    cap = _round_size(model, bool(guided))
    strokes = []
    for i0 in range(0, len(lines), cap):
        strokes += infer_batch(lines[i0:i0 + cap], sv, model, diffusion_mode=diffusion_mode, T=T, seed=seed,
                               first_sample=first_sample + i0 * candidates, candidates=candidates, levels=levels, steps=steps, **guided, **solver)
    out, _, _ = render_page(pad_strokes(strokes), [len(s) for s in strokes], slots, pages=pages, height=height, width=width,
                            lines_per_page=lines_per_page, margin_left=margin_left, margin_top=margin_top, pitch=pitch,
                            line_width=line_width, scale=scale)
    return out, strokes


def write_page_file(text: str, source, config_path: str | None = None, checkpoint_path: str | None = None,
                    experiment_path: str | None = None, output: str = "result", diffusion_mode: str = "new", *,
                    precision: str = "bf16", seed: int = 0, style_weights: str | None = None, candidates: int = 1,
                    steps: int | None = None, guidance=None, order: int | None = None, svg: bool = False, truth: bool = False,
                    truth_level: str = "word", truth_labels: bool = False, **page_kwargs) -> list:
    """``infer.py --page-file``: resolve config / checkpoint as ``infer_file`` does, ``write_page`` the text in the hand of
    ``source`` and save ``./<output>_p<k>.png`` per page (``vis.save_page_png``).  ``svg``: also ``./<output>_p<k>.svg``, the
    same lines as curves (``vector.stroke_paths`` with the same page arguments at its default smoothing and thinning,
    ``vector.save_page_svg``).  ``truth``: also ``./<output>_p<k>.json``, the box, stroke rows and text of every word
    (``truth_level="char"``: character) of the page, and with ``truth_labels`` ``./<output>_p<k>_labels.npy``, which item every
    ink pixel belongs to (``truth.page_truth`` with the very page arguments of the PNG, on one ``align`` + ``align_monotone`` per
    round of lines; ``truth.save_page_truth``).  Returns the list of [L_i,3] strokes."""
    from .checkpoint import load_model
    from .vector import save_page_svg, stroke_paths
    from .vis import save_page_png

    lines, _ = wrap_text(text, page_kwargs.get("max_chars", 40))
    if not lines:
        raise ValueError("write_page_file: the text holds no word")
    if truth_level not in ("word", "char"):
        raise ValueError(f"truth_level must be 'word' or 'char', got {truth_level!r}")
    candidates = _check_candidates(candidates)
    ddim = _ddim_kw(steps, order, guidance, candidates, 1)
    config_path, checkpoint_path = _resolve_experiment(config_path, checkpoint_path, experiment_path)
    style = load_style(source, style_weights)
    model = load_model(config_path, checkpoint_path, precision=precision, max_B=_rounds_capacity(min(len(lines), 64), candidates),
                       style_rows=style.shape[1])
    out, strokes = write_page(text, style, model, diffusion_mode=diffusion_mode, seed=seed, candidates=candidates, **ddim, **page_kwargs)
    out = out.cpu()
    for k in range(out.shape[0]):
        save_page_png(out[k], f"{output}_p{k}")
    if svg or truth:
        _, slots = wrap_text(text, page_kwargs.get("max_chars", 40))
        lens = [len(s) for s in strokes]
        geometry = {k: v for k, v in page_kwargs.items() if k in ("height", "width", "lines_per_page", "margin_left", "margin_top", "pitch", "scale")}
    if svg:
        paths = stroke_paths(pad_strokes(strokes), lens, slots, pages=int(out.shape[0]), **geometry)
        for k in range(paths.pages):
            save_page_svg(paths, k, f"{output}_p{k}", line_width=page_kwargs.get("line_width", 2.0))
    if truth:
        from .truth import page_truth, save_page_truth

        if "line_width" in page_kwargs:
            geometry["line_width"] = page_kwargs["line_width"]
        token = torch.full((len(lines), max(lens)), -1, dtype=torch.int32)
        cap = _round_size(model)
        for i0 in range(0, len(lines), cap):   # one align + align_monotone per round of lines
            txt, _, sv = _encode_batch("write_page_file", lines[i0:i0 + cap], style)
            st = torch.from_numpy(pad_strokes(strokes[i0:i0 + cap]))
            al = align_monotone(align(model, st, txt, sv, lengths=lens[i0:i0 + cap]), txt)
            token[i0:i0 + cap, :al.token.shape[1]] = al.token.cpu()
        rec = page_truth(pad_strokes(strokes), token, lines, lens, slots, level=truth_level, labels=bool(truth_labels), pages=int(out.shape[0]),
                         **geometry)
        for k in range(rec.pages):
            save_page_truth(rec, k, f"{output}_p{k}")
    return strokes


def pad_strokes(strokes_list) -> np.ndarray:
    """A list of [L_i,3] stroke arrays as one f32 [B, max L_i, 3] array, 0 past each line's end: what ``infer.py
    --save-strokes`` writes and ``--restyle`` reads back (line i's length follows from its prompt)."""
    lens = [int(len(s)) for s in strokes_list]
    batch = np.zeros((len(lens), max(lens), 3), np.float32)
    for b, s_ in enumerate(strokes_list):
        batch[b, :lens[b]] = np.asarray(s_, np.float32)
    return batch


def _load_strokes(strokes_path, lens) -> torch.Tensor:
    """The .npy of ``infer.py --save-strokes`` for prompts of stroke lengths ``lens``, cut to [B, max(lens), 3]."""
    old = np.load(str(strokes_path), allow_pickle=False)
    if old.ndim != 3 or old.shape[0] != len(lens) or old.shape[1] < max(lens) or old.shape[2] != 3:
        raise ValueError(f"{strokes_path}: expected strokes [{len(lens)}, >= {max(lens)}, 3] for these prompts, got {tuple(old.shape)}")
    return torch.from_numpy(np.ascontiguousarray(old[:, :max(lens)], dtype=np.float32))


def score_file(prompts, strokes_path, source, config_path: str | None = None, checkpoint_path: str | None = None,
               experiment_path: str | None = None, *, precision: str = "bf16", seed: int = 0, style_weights: str | None = None) -> list:
    """``infer.py --score``: the lines of ``prompts`` as an earlier run wrote them (``strokes_path``: the .npy of ``infer.py
    --save-strokes``) scored against their text and the hand of ``source`` by one ``score(..., pen_round=True)`` call at the
    default levels.  Returns one ``(L_i, score term, pen term, total)`` per line, each averaged over the levels."""
    model, old, text, sv, lens = _open_lines("score_file", prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, precision,
                                             style_weights)
    sc = score(model, old, text, sv, lengths=lens, seed=seed, pen_round=True).mean(dim=1).detach().cpu().tolist()
    return [(lens[b], sc[b][0], sc[b][1], sc[b][0] + sc[b][1]) for b in range(len(lens))]


def restyle_file(prompts, strokes_path, source, config_path: str | None = None, checkpoint_path: str | None = None,
                 experiment_path: str | None = None, output: str = "result", diffusion_mode: str = "new", *, strength: float = 0.5,
                 precision: str = "bf16", seed: int = 0, render: bool = True, style_weights: str | None = None,
                 renderer: str = "matplotlib") -> list:
    """``infer.py --restyle``: the lines of ``prompts`` as an earlier run wrote them (``strokes_path``: the .npy of ``infer.py
    --save-strokes``, [B, >= max L_i, 3]) rewritten in the hand of ``source`` by one ``restyle`` call; ``./<output>_<i>.png``
    per line.  Returns the list of [L_i, 3] strokes."""
    _check_renderer(renderer)
    model, old, text, sv, lens = _open_lines("restyle_file", prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, precision,
                                             style_weights)
    out = restyle(old, text, sv, model, lengths=lens, strength=strength, diffusion_mode=diffusion_mode, seed=seed).detach().cpu().numpy()
    strokes = [out[b, :lens[b]].copy() for b in range(len(lens))]
    if render:
        _save_lines(strokes, [f"{output}_{i}" for i in range(len(strokes))], renderer)
    return strokes
