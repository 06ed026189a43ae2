"""Input side of the "existing line" entry points: raw pen trajectories -> the model's (dx, dy, pen) strokes on the GPU
(include/dhw.h dhw_encode), the IAM-OnDB lineStrokes reader, and training batches in the form train.py --data
reads."""
from __future__ import annotations

import math
import xml.etree.ElementTree as ET

import numpy as np

from . import _call

ENCODE_MAX_B, ENCODE_MAX_N, ENCODE_MAX_L, ENCODE_MAX_ROUNDS = 65535, 4096, 4096, 8   # csrc/encode/encode_host.h


def read_strokes_xml(path) -> np.ndarray:
    """An IAM-OnDB lineStrokes file (<StrokeSet><Stroke><Point x= y= .../>...) -> float32 [n,3] = (x, y, end) in file order (no
    sort by time stamp), end = 1 on the last point of each Stroke.  y grows downward, as the tablet recorded it."""
    stroke_set = ET.parse(path).getroot().find("StrokeSet")
    if stroke_set is None:
        raise ValueError(f"{path}: no StrokeSet element")
    rows = []
    for stroke in stroke_set.findall("Stroke"):
        pts = stroke.findall("Point")
        rows += [(float(p.attrib["x"]), float(p.attrib["y"]), 1.0 if i == len(pts) - 1 else 0.0) for i, p in enumerate(pts)]
    if not rows:
        raise ValueError(f"{path}: the StrokeSet holds no Point")
    return np.asarray(rows, np.float32)


def upper_bound_rows(n: int, rounds: int) -> int:
    """Rows a line of n points has after `rounds` merge rounds: n - 1 shrunk by M - M // 5 each round."""
    M = max(int(n) - 1, 0)
    for _ in range(rounds):
        M -= M // 5
    return M


def padded_lengths(lengths) -> list[int]:
    """Each length rounded up to a multiple of 8, at least 8: the `lengths=` argument of score / align / restyle / invert."""
    host = lengths.tolist() if hasattr(lengths, "tolist") else list(lengths)
    return [max(8, -(-int(v) // 8) * 8) for v in host]


def _as_points(i: int, line) -> np.ndarray:
    """One item of `lines` -> float32 [n,3] with the end flag set on the line's last point."""
    if isinstance(line, (list, tuple)):   # polylines, one per pen-down stroke
        parts = []
        for s, poly in enumerate(line):
            a = np.asarray(poly, np.float32)
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError(f"lines[{i}][{s}] must be an [m, 2] polyline, got {a.shape}")
            if len(a):
                parts.append(np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1))
                parts[-1][-1, 2] = 1.0
        pts = np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)
    else:
        a = line.detach().cpu().numpy() if hasattr(line, "detach") else np.asarray(line)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"lines[{i}] must be an [n, 3] array of (x, y, end) or a list of [m, 2] polylines, got {a.shape}")
        pts = a.astype(np.float32)   # (a copy: the caller's array keeps its last flag)
    if not 2 <= len(pts) <= ENCODE_MAX_N:
        raise ValueError(f"lines[{i}] must hold 2 to {ENCODE_MAX_N} points, got {len(pts)}")
    pts[-1, 2] = 1.0
    return pts


def encode_strokes(lines, L=None, rounds: int = 3, max_abs: float = 15.0, device=None):
    """Encode a batch of raw pen lines on the GPU (include/dhw.h dhw_encode).

    lines: a list; each item is an [n,3] array of (x, y, end) (y downward, end != 0 on the last point of a pen-down stroke) or
    a list of [m,2] polylines, one per pen-down stroke.  The end flag of each polyline's last point and of the line's last
    point is set here.  L: rows of the result; None = the longest line's row bound (n - 1 shrunk `rounds` times), rounded up
    to a multiple of 8.  Returns (strokes f32 [B,L,3], lengths int32 [B], status int32 [B]), all on the GPU; a line whose
    status is not 0 (2 = non-finite or constant input, 4 = longer than L, 8 = an offset above max_abs) is all padding."""
    import torch

    if not isinstance(lines, (list, tuple)) or not lines:
        raise ValueError("lines must be a non-empty list of lines")
    if len(lines) > ENCODE_MAX_B:
        raise ValueError(f"lines must hold at most {ENCODE_MAX_B} lines, got {len(lines)}")
    rounds = _call.check_int("rounds", rounds, 0, ENCODE_MAX_ROUNDS)
    max_abs = _call.check_number("max_abs", max_abs, finite=False)   # (its own message for both rules)
    if not math.isfinite(max_abs) or not max_abs > 0:
        raise ValueError(f"max_abs = {max_abs} must be finite and > 0")
    pts = [_as_points(i, ln) for i, ln in enumerate(lines)]
    if L is None:
        L = max(8, -(-max(upper_bound_rows(len(p), rounds) for p in pts) // 8) * 8)
    L = _call.check_int("L", L, 8, ENCODE_MAX_L)
    with _call.open("encode_strokes", device=device) as c:
        B, N = len(pts), max(len(p) for p in pts)
        host = np.zeros((B, N, 3), np.float32)
        for b, p in enumerate(pts):
            host[b, :len(p)] = p
        points = c.to(torch.from_numpy(host))
        counts = c.to(torch.tensor([len(p) for p in pts], dtype=torch.int32), torch.int32)
        strokes, lengths, status = c.empty((B, L, 3)), c.empty((B,), torch.int32), c.empty((B,), torch.int32)
        ws, need = c.workspace(None, "dhw_encode_workspace_bytes", B, N)
        c.run("dhw_encode", points.data_ptr(), counts.data_ptr(), B, N, L, rounds, max_abs, strokes.data_ptr(), lengths.data_ptr(),
              status.data_ptr(), c.ptr(ws), need)
    return strokes, lengths, status


def make_batches(lines, texts, style, max_seq_len: int = 480, max_text_len: int = 50, writers=None) -> dict:
    """Training samples in the form train.py --data reads: {"strokes" f32 [K,max_seq_len,3], "text" int64 [K,max_text_len],
    "style" f32 [K,14,1280], "kept": the indices of the K samples kept}, on the host.  Lines are encoded by encode_strokes at
    L = max_seq_len, texts tokenised and zero-padded; a sample whose line has a non-zero status or whose
    len(text) >= max_text_len is dropped, as the reference's IAMDataset drops it.  style: [B,14,1280] from load_style /
    StyleExtractor, one per line.  ``writers``: one integer writer id per line; the dict then also holds "writer" (int64 [K], the
    kept lines'), from which train.py --resident takes each sample's style from another line of the same writer."""
    import torch

    from .tokenizer import Tokenizer
    if len(texts) != len(lines):
        raise ValueError(f"texts must hold {len(lines)} entries, got {len(texts)}")
    if any(not isinstance(t, str) for t in texts):
        raise ValueError("texts must be a list of str")
    max_text_len = _call.check_int("max_text_len", max_text_len, 2, 4096)
    style = torch.as_tensor(style)
    if tuple(style.shape) != (len(lines), 14, 1280):
        raise ValueError(f"style must be [{len(lines)}, 14, 1280], got {tuple(style.shape)}")
    if writers is not None:
        w = np.asarray(writers.cpu() if isinstance(writers, torch.Tensor) else writers)
        if w.shape != (len(lines),) or w.dtype.kind not in "iu":
            raise ValueError(f"writers must hold {len(lines)} integer ids, got shape {tuple(w.shape)} dtype {w.dtype}")
    strokes, _, status = encode_strokes(lines, L=max_seq_len)
    status = status.cpu().tolist()
    kept = [i for i, t in enumerate(texts) if status[i] == 0 and len(t) < max_text_len]
    tk = Tokenizer()
    text = torch.zeros((len(kept), max_text_len), dtype=torch.int64)
    for r, i in enumerate(kept):
        ids = tk.encode(texts[i])
        text[r, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
    idx = torch.tensor(kept, dtype=torch.int64)
    out = {"strokes": strokes.cpu()[idx], "text": text, "style": style.detach().cpu().float()[idx], "kept": kept}
    if writers is not None:
        out["writer"] = torch.from_numpy(w.astype(np.int64))[idx]
    return out
