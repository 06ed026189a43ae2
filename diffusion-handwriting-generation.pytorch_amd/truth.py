"""Ground truth for written pages (include/dhw.h dhw_truth): where every word or character of a page sits,
which pixels are its ink and which stroke rows write it.  ``group_boxes`` is the device call, at ``render_page``'s geometry;
``monotone_tokens`` and ``word_map`` turn an attention map and the prompts into the group of every stroke row; ``page_truth``
joins them, ``truth_json`` / ``save_page_truth`` write the result."""
from __future__ import annotations

import json
from dataclasses import dataclass, field

import numpy as np

from . import _call
from .vis import check_page_geometry, check_page_lines, check_page_strokes

TRUTH_MAX_G = 256   # csrc/truth/truth_host.h


@dataclass
class GroupBoxes:
    """What ``group_boxes`` returns.  boxes f32 [N,G,4] = left, top, right, bottom of every group's ink in page pixels, spans
    int32 [N,G,3] = (first drawn row, last drawn row + 1, drawn segments), zeros for a group that draws nothing; labels int32
    [P,1,H,W] (0 = no ink or unassigned ink, else 1 + n G + g) or None; scale f32 [1] (tensors, on the GPU); slots = the slot
    of every line as given (a list, or the int32 device tensor of the call; None: slot n = n); and the geometry of the call."""
    boxes: object
    spans: object
    labels: object
    scale: object
    slots: object
    G: int
    pages: int
    height: int
    width: int
    lines_per_page: int
    margin_left: float
    margin_top: float
    pitch: float
    line_width: float


def _check_groups(groups, N: int, L: int):
    import torch

    g = groups if isinstance(groups, torch.Tensor) else torch.as_tensor(np.asarray(groups))
    if g.dim() != 2 or tuple(g.shape) != (N, L):
        raise ValueError(f"groups must be [N, L] = [{N}, {L}], got {tuple(g.shape)}")
    if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
        raise ValueError(f"groups must hold integers, got {g.dtype}")
    return g


def _check_call(strokes, G, lengths, slots, labels, pages, height, width, lines_per_page, margin_left, margin_top, pitch, line_width, scale):
    """Every rule of ``group_boxes`` but the one on ``groups``, on the host."""
    x, N, L = check_page_strokes(strokes)
    G = _call.check_int("G", G, 1, TRUTH_MAX_G)
    if not isinstance(labels, (bool, np.bool_)):
        raise ValueError(f"labels = {labels!r} must be a bool")
    g = check_page_geometry(pages, height, width, lines_per_page, margin_left, margin_top, pitch, line_width, scale)
    host_lens, host_slots, P = check_page_lines(lengths, slots, N, L, g)
    return x, N, L, G, g, host_lens, host_slots, P


def _device_call(x, groups, N, L, G, g, host_lens, lengths, host_slots, slots, P, labels) -> GroupBoxes:
    import torch

    with _call.open("group_boxes", like=x) as c:
        x = c.to(x.detach())
        lens, slot_t = _call.stage_ints(c, host_lens, lengths), _call.stage_ints(c, host_slots, slots)
        grp = _call.stage_ints(c, None, groups)
        ws, need = c.workspace("truth", "dhw_truth_workspace_bytes", N, L, G)
        boxes, spans, scale_out = c.empty((N, G, 4)), c.empty((N, G, 3), torch.int32), c.empty((1,))
        lab = c.empty((P, 1, g["height"], g["width"]), torch.int32, wanted=bool(labels))
        c.run("dhw_truth", x.data_ptr(), c.ptr(lens), c.ptr(slot_t), grp.data_ptr(), N, L, G, P, g["height"], g["width"], g["lines_per_page"],
              g["margin_left"], g["margin_top"], g["pitch"], g["line_width"], g["scale"], boxes.data_ptr(), spans.data_ptr(), c.ptr(lab),
              scale_out.data_ptr(), c.ptr(ws), need)
    return GroupBoxes(boxes, spans, lab, scale_out, host_slots if host_slots is not None else slot_t, G, P, g["height"], g["width"],
                      g["lines_per_page"], g["margin_left"], g["margin_top"], g["pitch"], g["line_width"])


def group_boxes(strokes, groups, G: int, lengths=None, slots=None, *, labels: bool = False, pages=None, height: int = 1980, width: int = 1400,
                lines_per_page: int = 20, margin_left: float = 70.0, margin_top: float = 70.0, pitch: float = 92.0, line_width: float = 2.0,
                scale=None) -> GroupBoxes:
    """Where every group of stroke rows sits on the pages of ``render_page``, on the GPU (include/dhw.h dhw_truth).

    strokes, lengths, slots, pages, the geometry, line_width and scale are ``render_page``'s: the same arguments give the boxes
    and labels of the very page it draws.  ``groups``: an integer tensor (or array) [N,L], the group of the segment that ends at
    stroke row i of line n; a value outside [0, G) leaves the row's ink unassigned.  It goes to the device unread.  ``G`` in
    [1, 256].  ``labels``: also the per-pixel map of the nearest group's id, 1 + n G + g (0: no ink within half the line width
    plus half a pixel, or unassigned ink nearest).

    Returns a ``GroupBoxes`` record, its tensors on the GPU.  Every argument rule raises ValueError before a device is
    touched.  One workspace is cached per device: calls on one device must be ordered on one stream."""
    x, N, L, G, g, host_lens, host_slots, P = _check_call(strokes, G, lengths, slots, labels, pages, height, width, lines_per_page, margin_left,
                                                          margin_top, pitch, line_width, scale)
    grp = _check_groups(groups, N, L)
    return _device_call(x, grp, N, L, G, g, host_lens, lengths, host_slots, slots, P, labels)


# ---------------------------------------------------------------- from an attention map to the group of every row (host)
def monotone_tokens(mean, n_tokens, rows=None):
    """The monotone reading of an attention map, on the host in float64: per line b the non-decreasing sequence k_q in
    [0, n_tokens[b]) that maximises sum_q log(mean[b,q,k_q] + 1e-12) -> token int32 [B,Lq] (a CPU tensor).

    Both ends are free and any forward jump is allowed; of several maximisers the lexicographically smallest sequence is
    returned (the sum is formed from the last row backwards, so equal sums are equal floats).  ``mean`` [B,Lq,Lt] (a tensor on
    any device, or an array), ``n_tokens``: B integers in [1, Lt].  ``rows`` (optional, B integers in [0, Lq]): line b has that
    many rows; the rows past them are -1.  O(Lq Lt) per line with a running maximum: at Lq <= 512 and Lt <= 50 that is
    25 600 steps, less than the time of one kernel launch and a copy back, so it stays on the host."""
    import torch

    m = np.asarray(mean.detach().cpu() if isinstance(mean, torch.Tensor) else mean, dtype=np.float64)
    if m.ndim != 3:
        raise ValueError(f"mean must be [B, Lq, Lt], got {m.shape}")
    B, Lq, Lt = m.shape
    nt = _call.host_ints("n_tokens", n_tokens, B)
    if any(not 1 <= v <= Lt for v in nt):
        raise ValueError(f"n_tokens must be {B} integers in [1, {Lt}], got {nt}")
    nr = [Lq] * B if rows is None else _call.host_ints("rows", rows, B)
    if any(not 0 <= v <= Lq for v in nr):
        raise ValueError(f"rows must be {B} integers in [0, {Lq}], got {nr}")
    out = np.full((B, Lq), -1, dtype=np.int32)
    for b in range(B):
        K, Q = nt[b], nr[b]
        if Q == 0:
            continue
        lp = np.log(m[b, :Q, :K] + 1e-12)
        # V[q, k] = the best sum of rows q.. with k_q = k; S[q, k] = max over k' >= k of V[q, k']
        V = np.empty((Q, K))
        S = np.empty((Q, K))
        V[Q - 1] = lp[Q - 1]
        S[Q - 1] = np.maximum.accumulate(V[Q - 1][::-1])[::-1]
        for q in range(Q - 2, -1, -1):
            V[q] = lp[q] + S[q + 1]
            S[q] = np.maximum.accumulate(V[q][::-1])[::-1]
        k = 0
        for q in range(Q):
            k = k + int(np.flatnonzero(V[q, k:] == S[q, k])[0])   # the smallest k' >= k that reaches the maximum
            out[b, q] = k
    return torch.from_numpy(out)


def word_map(prompts):
    """Token position -> word index: (map int32 [B,Lt] (a CPU tensor), words).  A word is a maximal run of non-space characters
    of the prompt; one character is one token (``Tokenizer.encode``, which appends the end token: Lt = the longest prompt + 1).
    Spaces, the end token and padding map to -1.  ``words[b]`` lists (text, first token, last token + 1) per word."""
    import torch

    prompts = list(prompts)
    if not prompts or any(not isinstance(p, str) for p in prompts):
        raise ValueError("prompts must be a non-empty list of str")
    Lt = max(len(p) for p in prompts) + 1
    m = np.full((len(prompts), Lt), -1, dtype=np.int32)
    words = []
    for b, p in enumerate(prompts):
        ws, k = [], 0
        while k < len(p):
            if p[k] == " ":
                k += 1
                continue
            e = k
            while e < len(p) and p[e] != " ":
                e += 1
            m[b, k:e] = len(ws)
            ws.append((p[k:e], k, e))
            k = e
        words.append(ws)
    return torch.from_numpy(m), words


def _char_map(prompts):
    """``word_map`` for characters: token k < len(prompt) is group k (spaces too); the end token and padding are -1."""
    import torch

    Lt = max(len(p) for p in prompts) + 1
    m = np.full((len(prompts), Lt), -1, dtype=np.int32)
    for b, p in enumerate(prompts):
        m[b, :len(p)] = np.arange(len(p))
    return torch.from_numpy(m), [[(ch, k, k + 1) for k, ch in enumerate(p)] for p in prompts]


@dataclass
class TruthItem:
    """One word or character: its text, its tokens [a, b), the stroke rows [a, b) that draw it, its ink box (left, top, right,
    bottom in page pixels); ``empty``: it drew nothing (rows and box are zeros)."""
    text: str
    tokens: tuple
    rows: tuple
    box: tuple
    empty: bool


@dataclass
class TruthLine:
    """One line: its text, slot and page (page -1: the slot is off the pages), its items, and ``box``: the hull of the boxes of
    its items that drew something (zeros when none did) — not the line's ink box, which also holds unassigned ink."""
    text: str
    slot: int
    page: int
    box: tuple
    items: list = field(default_factory=list)


@dataclass
class PageTruth:
    """What ``page_truth`` returns: ``lines`` (one ``TruthLine`` per line), ``level``, ``G``, ``labels`` (int32 [P,1,H,W] on the GPU:
    item j of line n has id 1 + n G + j; or None), ``scale`` (a float) and the geometry of the call."""
    lines: list
    level: str
    G: int
    labels: object
    scale: float
    pages: int
    height: int
    width: int
    lines_per_page: int
    margin_left: float
    margin_top: float
    pitch: float
    line_width: float


def page_truth(strokes, alignment, prompts, lengths=None, slots=None, *, level: str = "word", labels: bool = False, pages=None,
               height: int = 1980, width: int = 1400, lines_per_page: int = 20, margin_left: float = 70.0, margin_top: float = 70.0,
               pitch: float = 92.0, line_width: float = 2.0, scale=None) -> PageTruth:
    """The words (``level="word"``) or characters (``"char"``) of written lines on the pages ``render_page`` draws of the same
    arguments: one ``group_boxes`` call whose groups are ``word_map(prompts)[token]`` (words) or the token itself with the end
    token unassigned (characters), ``token`` = ``alignment.token`` [N,L] (``alignment``: an ``Alignment``, or the token tensor itself).  Use ``align_monotone`` for the alignment: only then
    is every item's ``rows`` one contiguous span and are the spans of a line in order.  Every argument rule raises ValueError
    before a device is touched; the result is on the host but for ``labels``."""
    import torch

    x, N, L, _, g, host_lens, host_slots, P = _check_call(strokes, 1, lengths, slots, labels, pages, height, width, lines_per_page, margin_left,
                                                          margin_top, pitch, line_width, scale)
    if level not in ("word", "char"):
        raise ValueError(f"level must be 'word' or 'char', got {level!r}")
    prompts = list(prompts)
    if len(prompts) != N or any(not isinstance(p, str) for p in prompts):
        raise ValueError(f"prompts must be {N} str, one per line")
    token = alignment if isinstance(alignment, torch.Tensor) else getattr(alignment, "token", None)
    if not isinstance(token, torch.Tensor) or tuple(token.shape) != (N, L) or token.is_floating_point():
        raise ValueError(f"alignment.token must be an integer tensor [N, L] = [{N}, {L}]")
    m, items = word_map(prompts) if level == "word" else _char_map(prompts)
    G = max(1, max(len(it) for it in items))
    if G > TRUTH_MAX_G:
        raise ValueError(f"a line holds {G} {level}s, more than {TRUTH_MAX_G}")

    Lt = m.shape[1]
    tk = token.to(torch.int64)
    inside = (tk >= 0) & (tk < Lt)
    groups = torch.where(inside, m.to(token.device, torch.int64).gather(1, tk.clamp(0, Lt - 1)), torch.full_like(tk, -1)).to(torch.int32)
    gb = _device_call(x, groups, N, L, G, g, host_lens, lengths, host_slots, slots, P, labels)

    boxes, spans = gb.boxes.cpu().numpy(), gb.spans.cpu().numpy()
    slot_list = list(range(N)) if gb.slots is None else [int(v) for v in (gb.slots.cpu().tolist() if hasattr(gb.slots, "cpu") else gb.slots)]
    lines = []
    for n in range(N):
        its = []
        for j, (text, a, b) in enumerate(items[n]):
            empty = int(spans[n, j, 2]) == 0
            its.append(TruthItem(text, (a, b), (int(spans[n, j, 0]), int(spans[n, j, 1])), tuple(float(v) for v in boxes[n, j]), empty))
        drew = [it.box for it in its if not it.empty]
        hull = (min(b[0] for b in drew), min(b[1] for b in drew), max(b[2] for b in drew), max(b[3] for b in drew)) if drew else (0.0,) * 4
        on = 0 <= slot_list[n] < P * g["lines_per_page"]
        lines.append(TruthLine(prompts[n], slot_list[n], slot_list[n] // g["lines_per_page"] if on else -1, hull, its))
    return PageTruth(lines, level, G, gb.labels, float(gb.scale.cpu()[0]), P, g["height"], g["width"], g["lines_per_page"], g["margin_left"],
                     g["margin_top"], g["pitch"], g["line_width"])


def truth_json(truth: PageTruth, page: int, precision: int = 2) -> str:
    """One page of a ``PageTruth`` as JSON, keys in this order and floats with ``precision`` decimals (but ``scale``, which is
    written with the shortest digits that give back its float32):
    ``{"page", "width", "height", "scale", "line_width", "level", "groups", "lines": [{"line", "slot", "text", "box",
    "items": [{"id", "text", "tokens", "rows", "box", "empty"}]}]}``, one line of the page per text line, in line order.
    ``box`` = [left, top, right, bottom]; a line's box is the hull of its items' boxes; ``id`` is the item's value in the label
    map, 1 + line x groups + its index."""
    page = _call.check_int("page", page, 0)
    if page >= truth.pages:
        raise ValueError(f"page = {page} must be below the record's {truth.pages} pages")
    precision = _call.check_int("precision", precision, 0)

    def num(v):
        return format(float(v), f".{precision}f")

    scale = np.format_float_positional(np.float32(truth.scale), unique=True, trim="0")   # every digit of the float32: it reproduces the placement (trim "0": 2.0, never a bare "2.")

    def box(b):
        return "[" + ", ".join(num(v) for v in b) + "]"

    out = [f'{{"page": {page}, "width": {truth.width}, "height": {truth.height}, "scale": {scale}, '
           f'"line_width": {num(truth.line_width)}, "level": {json.dumps(truth.level)}, "groups": {truth.G}, "lines": [']
    rows = []
    for n, ln in enumerate(truth.lines):
        if ln.page != page:
            continue
        its = [f'{{"id": {1 + n * truth.G + j}, "text": {json.dumps(it.text)}, "tokens": [{it.tokens[0]}, {it.tokens[1]}], '
               f'"rows": [{it.rows[0]}, {it.rows[1]}], "box": {box(it.box)}, "empty": {"true" if it.empty else "false"}}}'
               for j, it in enumerate(ln.items)]
        rows.append(f' {{"line": {n}, "slot": {ln.slot}, "text": {json.dumps(ln.text)}, "box": {box(ln.box)}, "items": [\n  '
                    + ",\n  ".join(its) + "]}")
    out.append(",\n".join(rows))
    out.append("]}")
    return "\n".join(out) + "\n"


def save_page_truth(truth: PageTruth, page: int, name: str, precision: int = 2) -> None:
    """Write one page of ``page_truth`` to ./<name>.json (``truth_json``) and, when the record has labels, that page's label
    map int32 [H,W] to ./<name>_labels.npy."""
    text = truth_json(truth, page, precision)
    with open(f"./{name}.json", "w", encoding="utf-8") as f:
        f.write(text)
    if truth.labels is not None:
        np.save(f"./{name}_labels.npy", truth.labels[page, 0].detach().cpu().numpy())
