"""Host side of the page ground truth (include/dhw.h dhw_truth; dhg_amd.group_boxes, monotone_tokens, align_monotone, word_map,
page_truth, truth_json, save_page_truth, write_page_file(truth=True)) that needs no GPU: the two symbols declared, exported and
bound; every argument rule of the C entry through the handle-less error path; every ValueError of group_boxes / page_truth,
raised before a device is touched; monotone_tokens against exhaustive enumeration; word_map; exact JSON strings; infer.py
--truth dispatch and refusals; the numpy statement of the rules (tests/truth_ref.py) on cases worked out by hand; that the
label inputs of the GPU tests are not vacuous; and csrc/truth/truth_host.h alone under AddressSanitizer + UBSan."""
import ctypes as C
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, truth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import truth_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- the C-ABI
def test_truth_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bsize_t\s+dhw_truth_workspace_bytes\s*\(", header) and re.search(r"\bint\s+dhw_truth\s*\(", header)
    l = _lib.lib()
    for name in ("dhw_truth_workspace_bytes", "dhw_truth"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_truth.restype is C.c_int and l.dhw_truth_workspace_bytes.restype is C.c_size_t and len(_lib.SIGNATURES["dhw_truth"][1]) == 23
    for name in ("group_boxes", "monotone_tokens", "word_map", "page_truth", "truth_json", "save_page_truth", "GroupBoxes", "PageTruth"):
        assert getattr(dhg_amd, name) is getattr(truth, name)
    assert dhg_amd.align_monotone is dhg_amd.inference.align_monotone
    with open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "host", "error.h")) as f:
        assert "dhw_truth" in f.read()


def test_truth_workspace_bytes():
    f = _lib.lib().dhw_truth_workspace_bytes
    assert f(1, 1, 1) == 64 and f(5, 40, 5) == 5 * 32 + 5 * 40 * 20 and f(4096, 4096, 256) == 4096 * 32 + 4096 * 4096 * 20
    assert f(3, 7, 256) == (3 * 32 + 3 * 7 * 20 + 15) // 16 * 16
    assert f(0, 8, 1) == 0 and f(4097, 8, 1) == 0 and f(1, 0, 1) == 0 and f(1, 4097, 1) == 0 and f(1, 1, 0) == 0 and f(1, 1, 257) == 0


def _call(**kw):
    a = dict(strokes=FAKE, lens=None, slots=None, groups=FAKE, N=3, L=40, G=5, P=2, H=160, W=256, lpp=3, ml=6.0, mt=4.0, pitch=48.0, lw=2.0, scale=0.0,
             boxes=FAKE, spans=FAKE, labels=FAKE, scale_out=FAKE, workspace=FAKE, workspace_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(l.dhw_truth_workspace_bytes(min(max(a["N"], 1), 4096), min(max(a["L"], 1), 4096), min(max(a["G"], 1), 256)), 16)
    rc = l.dhw_truth(a["strokes"], a["lens"], a["slots"], a["groups"], a["N"], a["L"], a["G"], a["P"], a["H"], a["W"], a["lpp"], a["ml"], a["mt"],
                     a["pitch"], a["lw"], a["scale"], a["boxes"], a["spans"], a["labels"], a["scale_out"], a["workspace"], a["workspace_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


BAD_C = [
    (dict(N=0), "N"), (dict(N=4097), "N"), (dict(L=0), "L"), (dict(L=4097), "L"), (dict(G=0), "G must"), (dict(G=257), "G must"), (dict(G=-1), "G must"),
    (dict(P=0), "P"), (dict(H=7), "H"), (dict(W=4), "W"), (dict(W=130), "W"), (dict(P=2, H=2 ** 15, W=2 ** 15), "2\\^31"),
    (dict(P=2 ** 24, H=8, W=8), "launch grid"), (dict(lpp=0), "lines_per_page"),
    (dict(pitch=0.0), "pitch"), (dict(pitch=-1.0), "pitch"), (dict(pitch=NAN), "pitch"), (dict(pitch=INF), "pitch"),
    (dict(ml=-1.0), "margin_left"), (dict(ml=NAN), "margin_left"), (dict(ml=INF), "margin_left"), (dict(ml=128.0), "margin_left"),
    (dict(mt=-1.0), "margin_top"), (dict(mt=NAN), "margin_top"), (dict(mt=INF), "margin_top"),
    (dict(lw=0.25), "line_width"), (dict(lw=16.5), "line_width"), (dict(lw=NAN), "line_width"),
    (dict(scale=-0.5), "scale"), (dict(scale=NAN), "scale"), (dict(scale=INF), "scale"),
    (dict(strokes=None), "strokes"), (dict(groups=None), "groups is NULL"), (dict(boxes=None), "boxes_out"), (dict(spans=None), "spans_out"),
    (dict(scale_out=None), "scale_out"), (dict(workspace=None), "workspace"), (dict(workspace_bytes=15), "workspace_bytes"),
    (dict(labels=FAKE + 8), "16-byte aligned"), (dict(workspace=FAKE + 4), "16-byte aligned"),
    (dict(strokes=FAKE + 2), "4-byte aligned"), (dict(lens=FAKE + 1), "4-byte aligned"), (dict(slots=FAKE + 2), "4-byte aligned"),
    (dict(groups=FAKE + 2), "4-byte aligned"), (dict(boxes=FAKE + 2), "4-byte aligned"), (dict(spans=FAKE + 1), "4-byte aligned"),
    (dict(scale_out=FAKE + 3), "4-byte aligned"),
]


@pytest.mark.parametrize("bad,name", BAD_C)
def test_each_argument_rule_of_dhw_truth_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_truth:"), (bad, msg)


def test_truth_workspace_one_byte_short_is_rejected():
    need = _lib.lib().dhw_truth_workspace_bytes(5, 40, 5)
    rc, msg = _call(N=5, workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in msg


def test_kernel_constants_match_the_python_side():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "truth", "truth_host.h")).read()
    assert int(re.search(r"constexpr int TRUTH_MAX_G = (\d+);", src).group(1)) == truth.TRUTH_MAX_G == 256
    assert "hip" not in src.lower().replace("dhw_truth", "").replace("no hip", "")   # truth_host.h holds no HIP


# ---------------------------------------------------------------- ValueError before a device is touched
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(truth, "_device_call", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


ST = np.zeros((3, 16, 3), np.float32)
GR = np.zeros((3, 16), np.int32)
SMALL = dict(height=96, width=128, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=40.0)
BAD_GEOMETRY = [
    (dict(pages=0), "pages = 0"), (dict(pages=1.0), "pages = 1.0 is not an integer"), (dict(pages=True), "not an integer"),
    (dict(height=7), "height = 7"), (dict(height=96.0), "not an integer"),
    (dict(width=4), "width = 4"), (dict(width=130), "width = 130 must be a multiple of 4"),
    (dict(pages=2, height=2 ** 15, width=2 ** 15), "below 2\\^31"),
    (dict(pages=2 ** 24, height=8, width=8, margin_left=0), "launch grid"),
    (dict(lines_per_page=0), "lines_per_page = 0"), (dict(lines_per_page=2.5), "not an integer"),
    (dict(pitch=0), "pitch = 0.0 must be > 0"), (dict(pitch=-3.0), "pitch"), (dict(pitch=NAN), "pitch = nan must be finite"),
    (dict(pitch="92"), "pitch = '92' is not a number"),
    (dict(margin_left=-1), "margin_left = -1.0"), (dict(margin_left=INF), "margin_left = inf must be finite"),
    (dict(margin_top=-0.5), "margin_top = -0.5"), (dict(margin_top=NAN), "margin_top"),
    (dict(width=128, margin_left=64), "leaves no room"),
    (dict(line_width=0.25), r"line_width = 0.25 must lie in \[0.5, 16\]"), (dict(line_width=17), "line_width"), (dict(line_width=NAN), "line_width"),
    (dict(scale=0), "scale = 0.0 must be > 0"), (dict(scale=-1.0), "scale"), (dict(scale=INF), "scale = inf must be finite"),
    (dict(scale=True), "scale = True is not a number"),
    (dict(labels=1), "labels = 1 must be a bool"), (dict(labels="yes"), "labels"),
    (dict(strokes=np.zeros((16, 3), np.float32)), r"strokes must be \[N, L, 3\]"),
    (dict(strokes=np.zeros((2, 16, 2), np.float32)), r"strokes must be \[N, L, 3\]"),
    (dict(strokes=np.zeros((0, 16, 3), np.float32)), "N in"),
    (dict(strokes=np.zeros((1, 4097, 3), np.float32)), "L in"),
    (dict(strokes=np.zeros((3, 16, 3), np.int32)), "floating-point"),
    (dict(lengths=[16, 16]), "lengths must hold 3 entries"), (dict(lengths=[16, 0, 16]), r"lengths must be 3 integers in \[1, 16\]"),
    (dict(lengths=[16, 17, 16]), "lengths must be 3 integers"), (dict(lengths=[16, 8.0, 16]), r"lengths\[1\] = 8.0 is not an integer"),
    (dict(slots=[0, 1]), "slots must hold 3 entries"), (dict(slots=[0, 1.5, 2]), r"slots\[1\] = 1.5 is not an integer"),
    (dict(slots=[0, True, 2]), r"slots\[1\] = True"), (dict(slots=[0, 1, 2 ** 31]), "does not fit int32"),
    (dict(slots=[0, 1, 2 ** 26], height=64, width=64, lines_per_page=1), "below 2\\^31"),
]
BAD_BOXES = BAD_GEOMETRY + [
    (dict(G=0), r"G = 0 must lie in \[1, 256\]"), (dict(G=257), "G = 257"), (dict(G=2.0), "G = 2.0 is not an integer"), (dict(G=True), "G = True"),
    (dict(groups=np.zeros((3, 15), np.int32)), r"groups must be \[N, L\] = \[3, 16\]"), (dict(groups=np.zeros((16,), np.int32)), "groups must be"),
    (dict(groups=np.zeros((3, 16), np.float32)), "groups must hold integers"), (dict(groups=np.zeros((3, 16), bool)), "groups must hold integers"),
]


@pytest.mark.parametrize("kw,msg", BAD_BOXES)
def test_group_boxes_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    with pytest.raises(ValueError, match=msg):
        dhg_amd.group_boxes(kw.pop("strokes", ST), kw.pop("groups", GR), kw.pop("G", 4), kw.pop("lengths", None), kw.pop("slots", None), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(lengths=[16, 1, 8]), dict(slots=[5, -1, 0]), dict(pages=3, scale=0.5), dict(labels=True), dict(G=256),
                                dict(groups=torch.full((3, 16), -7, dtype=torch.int64)),
                                dict(lengths=torch.tensor([1, 2, 3]), slots=torch.tensor([2, 1, 0]))])
def test_group_boxes_valid_arguments_get_as_far_as_the_device(monkeypatch, kw):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.group_boxes(ST, kw.pop("groups", GR), kw.pop("G", 4), kw.pop("lengths", None), kw.pop("slots", None), **kw)


PROMPTS = ["ab cd", "x", "hello you"]
TOKEN = torch.zeros((3, 16), dtype=torch.int32)
BAD_TRUTH = BAD_GEOMETRY + [
    (dict(level="line"), "level must be 'word' or 'char'"), (dict(prompts=["a", "b"]), "prompts must be 3 str"),
    (dict(prompts=["a", "b", 3]), "prompts must be 3 str"), (dict(token=torch.zeros((3, 8), dtype=torch.int32)), r"alignment.token must be an integer tensor"),
    (dict(token=torch.zeros((3, 16))), "alignment.token"), (dict(token=None), "alignment.token"),
    (dict(prompts=["a " * 257, "b", "c"], level="word"), "more than 256"),
]


@pytest.mark.parametrize("kw,msg", BAD_TRUTH)
def test_page_truth_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    al = dhg_amd.Alignment(None, kw.pop("token", TOKEN), spans=[])
    with pytest.raises(ValueError, match=msg):
        dhg_amd.page_truth(kw.pop("strokes", ST), al, kw.pop("prompts", PROMPTS), kw.pop("lengths", None), kw.pop("slots", None), **kw)


def test_page_truth_builds_the_groups_and_the_record(monkeypatch):
    """The device call replaced by one that records its groups and answers by hand: words -> word_map[token], characters ->
    the token itself with the end token and -1 rows unassigned; the record's lines, hulls, pages and empty items."""
    seen = {}

    def fake(x, groups, N, L, G, g, host_lens, lengths, host_slots, slots, P, labels):
        seen.update(groups=groups.clone(), G=G, P=P, labels=labels, slots=host_slots)
        boxes, spans = torch.zeros((N, G, 4)), torch.zeros((N, G, 3), dtype=torch.int32)
        boxes[0, 0], spans[0, 0] = torch.tensor([4.0, 10.0, 9.0, 14.0]), torch.tensor([1, 5, 4])
        boxes[0, 1], spans[0, 1] = torch.tensor([11.0, 8.5, 20.0, 13.0]), torch.tensor([6, 9, 3])
        return truth.GroupBoxes(boxes, spans, None, torch.tensor([1.5]), host_slots, G, P, g["height"], g["width"], g["lines_per_page"], g["margin_left"],
                                g["margin_top"], g["pitch"], g["line_width"])

    monkeypatch.setattr(truth, "_device_call", fake)
    token = torch.tensor([[0, 0, 1, 2, 3, 3, 4, 5, -1, -1], [0, 0, 0, 1, 1, 1, 1, -1, -1, -1]], dtype=torch.int32)
    st = np.zeros((2, 10, 3), np.float32)
    rec = dhg_amd.page_truth(st, dhg_amd.Alignment(None, token, spans=[]), ["ab cd", "x"], None, [0, 7], **SMALL)
    assert seen["groups"].tolist() == [[0, 0, 0, -1, 1, 1, 1, -1, -1, -1], [0, 0, 0, -1, -1, -1, -1, -1, -1, -1]] and seen["groups"].dtype == torch.int32
    assert seen["G"] == 2 and seen["P"] == 4 and seen["labels"] is False and rec.G == 2 and rec.level == "word" and rec.scale == 1.5
    l0, l1 = rec.lines
    assert (l0.text, l0.slot, l0.page, l0.box) == ("ab cd", 0, 0, (4.0, 8.5, 20.0, 14.0))
    assert [(i.text, i.tokens, i.rows, i.box, i.empty) for i in l0.items] == [("ab", (0, 2), (1, 5), (4.0, 10.0, 9.0, 14.0), False),
                                                                              ("cd", (3, 5), (6, 9), (11.0, 8.5, 20.0, 13.0), False)]
    assert (l1.slot, l1.page, l1.box) == (7, 3, (0.0,) * 4) and [(i.text, i.empty, i.rows) for i in l1.items] == [("x", True, (0, 0))]
    rec = dhg_amd.page_truth(st, dhg_amd.Alignment(None, token, spans=[]), ["ab cd", "x"], None, [0, 9], level="char", pages=2, **SMALL)
    assert seen["groups"].tolist() == [[0, 0, 1, 2, 3, 3, 4, -1, -1, -1], [0, 0, 0, -1, -1, -1, -1, -1, -1, -1]] and seen["G"] == 5
    assert [i.text for i in rec.lines[0].items] == list("ab cd") and rec.lines[1].page == -1     # slot 9 is off the two pages


# ---------------------------------------------------------------- monotone_tokens
def _enumerate_monotone(m, K):
    """The lexicographically smallest of the best non-decreasing sequences, by trying all of them; the sum is taken from the
    last row backwards, as monotone_tokens states it."""
    lp = np.log(np.asarray(m, np.float64)[:, :K] + 1e-12)
    best, arg = None, None
    for seq in itertools.combinations_with_replacement(range(K), len(lp)):   # (non-decreasing tuples, in lexicographic order)
        tot = 0.0
        for q in range(len(lp) - 1, -1, -1):
            tot = lp[q, seq[q]] + tot if q < len(lp) - 1 else lp[q, seq[q]]
        if best is None or tot > best:
            best, arg = tot, seq
    return list(arg)


def test_monotone_tokens_against_exhaustive_enumeration():
    rng = np.random.default_rng(5)
    cases = 0
    for Lq in range(1, 7):
        for Lt in range(1, 5):
            for kind in ("random", "ties", "flat"):
                m = rng.random((3, Lq, Lt))
                if kind == "ties":
                    m = rng.choice([0.125, 0.25, 0.5], (3, Lq, Lt))           # few values: many equal sums
                if kind == "flat":
                    m = np.full((3, Lq, Lt), 0.25)                             # every sequence ties: all zeros wins
                nt = [Lt, max(1, Lt - 1), 1]
                got = dhg_amd.monotone_tokens(torch.from_numpy(m), nt)
                assert got.dtype == torch.int32 and tuple(got.shape) == (3, Lq)
                for b in range(3):
                    assert got[b].tolist() == _enumerate_monotone(m[b], nt[b]), (Lq, Lt, kind, b)
                    cases += 1
                if kind == "flat":
                    assert not got.any()
    assert cases == 6 * 4 * 3 * 3


def test_monotone_tokens_by_hand_rows_and_refusals():
    m = np.array([[[0.9, 0.1, 0.0], [0.1, 0.8, 0.1], [0.7, 0.2, 0.1], [0.0, 0.1, 0.9]]])       # row 2 looks back at token 0: not allowed
    assert dhg_amd.monotone_tokens(m, [3]).tolist() == [[0, 1, 1, 2]]
    assert np.argmax(m[0], -1).tolist() == [0, 1, 0, 2]                                            # (what the row-wise argmax says)
    assert dhg_amd.monotone_tokens(m, [2]).tolist() == [[0, 1, 1, 1]]                              # the third token is past the prompt
    assert dhg_amd.monotone_tokens(m, [3], rows=[2]).tolist() == [[0, 1, -1, -1]] and dhg_amd.monotone_tokens(m, [3], rows=[0]).tolist() == [[-1] * 4]
    for bad, msg in ((dict(n_tokens=[0]), "n_tokens must be"), (dict(n_tokens=[4]), "n_tokens must be"), (dict(n_tokens=[1, 2]), "must hold 1 entries"),
                     (dict(n_tokens=[2], rows=[5]), "rows must be"), (dict(n_tokens=[2], mean=m[0]), r"mean must be \[B, Lq, Lt\]")):
        with pytest.raises(ValueError, match=msg):
            dhg_amd.monotone_tokens(bad.pop("mean", m), **bad)


def test_align_monotone_keeps_the_map_and_makes_spans_contiguous():
    mean = torch.zeros((2, 4, 4))
    mean[0] = torch.tensor([[0.9, 0.1, 0, 0], [0.1, 0.8, 0.1, 0], [0.7, 0.2, 0.1, 0], [0.0, 0.1, 0.9, 0]])
    mean[1, :2] = torch.tensor([[0.6, 0.4, 0, 0], [0.2, 0.8, 0, 0]])
    text = torch.tensor([[5, 6, 1, 0], [7, 1, 0, 0]])
    token = torch.tensor([[0] * 2 + [1] * 2 + [0] * 2 + [2] * 2, [0] * 2 + [1] * 2 + [-1] * 4], dtype=torch.int32)
    al = dhg_amd.Alignment(mean, token, None, [8, 4], 3)
    mono = dhg_amd.align_monotone(al, text)
    assert mono.mean is mean and mono.lengths == [8, 4] and mono.layer == 3 and mono.token.dtype == torch.int32
    assert mono.token.tolist() == [[0, 0, 1, 1, 1, 1, 2, 2], [0, 0, 1, 1, -1, -1, -1, -1]]
    assert mono.spans == [[(0, 2), (2, 6), (6, 8), None], [(0, 2), (2, 4), None, None]]
    assert al.token is token and al.spans[0][0] == (0, 6)                      # align's own record is untouched
    with pytest.raises(ValueError, match="text must hold integer token ids"):
        dhg_amd.align_monotone(al, text[:, :3])
    with pytest.raises(ValueError, match="at least one token"):
        dhg_amd.align_monotone(al, torch.zeros((2, 4), dtype=torch.int64))


# ---------------------------------------------------------------- word_map
def test_word_map():
    m, words = dhg_amd.word_map(["  ab  c ", "word", "   ", "a b"])
    assert m.dtype == torch.int32 and tuple(m.shape) == (4, 9)
    assert m.tolist() == [[-1, -1, 0, 0, -1, -1, 1, -1, -1],          # leading, double and trailing spaces; position 8 is the end token
                          [0, 0, 0, 0, -1, -1, -1, -1, -1],           # one word, its end token, padding
                          [-1] * 9,                                   # only spaces
                          [0, -1, 1, -1, -1, -1, -1, -1, -1]]
    assert words == [[("ab", 2, 4), ("c", 6, 7)], [("word", 0, 4)], [], [("a", 0, 1), ("b", 2, 3)]]
    assert len(dhg_amd.tokenizer.Tokenizer().encode("  ab  c ")) == 9         # one character is one token, plus the end token
    for bad in ([], ["a", 3], [None]):
        with pytest.raises(ValueError, match="prompts"):
            dhg_amd.word_map(bad)


# ---------------------------------------------------------------- truth_json
def _record(labels=None):
    items0 = [truth.TruthItem("ab", (0, 2), (1, 5), (4.0, 10.0, 9.125, 14.0), False), truth.TruthItem('c"d', (3, 6), (0, 0), (0.0,) * 4, True)]
    items1 = [truth.TruthItem("x", (0, 1), (2, 9), (5.0, 30.5, 7.0, 33.0), False)]
    lines = [truth.TruthLine('ab c"d', 0, 0, (4.0, 10.0, 9.125, 14.0), items0), truth.TruthLine("x", 3, 1, (5.0, 30.5, 7.0, 33.0), items1),
             truth.TruthLine("off", 9, -1, (0.0,) * 4, [])]
    return truth.PageTruth(lines, "word", 2, labels, 1.25, 2, 40, 32, 2, 4.0, 4.0, 16.0, 2.0)


def test_truth_json_exact_strings():
    rec = _record()
    assert dhg_amd.truth_json(rec, 0) == (
        '{"page": 0, "width": 32, "height": 40, "scale": 1.25, "line_width": 2.00, "level": "word", "groups": 2, "lines": [\n'
        ' {"line": 0, "slot": 0, "text": "ab c\\"d", "box": [4.00, 10.00, 9.12, 14.00], "items": [\n'
        '  {"id": 1, "text": "ab", "tokens": [0, 2], "rows": [1, 5], "box": [4.00, 10.00, 9.12, 14.00], "empty": false},\n'
        '  {"id": 2, "text": "c\\"d", "tokens": [3, 6], "rows": [0, 0], "box": [0.00, 0.00, 0.00, 0.00], "empty": true}]}\n'
        ']}\n')
    assert dhg_amd.truth_json(rec, 1, precision=1) == (
        '{"page": 1, "width": 32, "height": 40, "scale": 1.25, "line_width": 2.0, "level": "word", "groups": 2, "lines": [\n'
        ' {"line": 1, "slot": 3, "text": "x", "box": [5.0, 30.5, 7.0, 33.0], "items": [\n'
        '  {"id": 3, "text": "x", "tokens": [0, 1], "rows": [2, 9], "box": [5.0, 30.5, 7.0, 33.0], "empty": false}]}\n'
        ']}\n')
    for page in (0, 1):
        doc = json.loads(dhg_amd.truth_json(rec, page, precision=3))
        assert list(doc) == ["page", "width", "height", "scale", "line_width", "level", "groups", "lines"] and len(doc["lines"]) == 1
        assert list(doc["lines"][0]) == ["line", "slot", "text", "box", "items"]
        assert all(list(i) == ["id", "text", "tokens", "rows", "box", "empty"] for i in doc["lines"][0]["items"])
    assert json.loads(dhg_amd.truth_json(rec, 0, precision=3))["lines"][0]["box"] == [4.0, 10.0, 9.125, 14.0]
    rec.scale = float(np.float32(0.4637))                                # the scale keeps every digit of its float32 at any precision
    assert '"scale": 0.4637, ' in dhg_amd.truth_json(rec, 0, precision=1)
    assert np.float32(json.loads(dhg_amd.truth_json(rec, 0, precision=0))["scale"]) == np.float32(0.4637)
    for value, text in ((1.0, "1.0"), (2.0, "2.0"), (3e9, "3000000000.0"), (0.5, "0.5"), (float(np.float32(5.818182)), "5.818182"),
                        (float(np.float32(1e-7)), "0.0000001")):       # whole numbers keep a digit after the point: always a JSON number
        rec.scale = value
        for precision in (0, 2):
            doc = dhg_amd.truth_json(rec, 0, precision=precision)
            assert f'"height": 40, "scale": {text}, "line_width"' in doc, (value, doc[:120])
            assert np.float32(json.loads(doc)["scale"]) == np.float32(value)
    for bad, msg in ((dict(page=2), "page = 2"), (dict(page=-1), "page = -1"), (dict(page=0, precision=-1), "precision"), (dict(page=0.0), "not an integer")):
        with pytest.raises(ValueError, match=msg):
            dhg_amd.truth_json(rec, **bad)


def test_save_page_truth_writes_the_files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    dhg_amd.save_page_truth(_record(), 1, "out_p1")
    assert (tmp_path / "out_p1.json").read_text() == dhg_amd.truth_json(_record(), 1) and not (tmp_path / "out_p1_labels.npy").exists()
    labels = torch.arange(2 * 40 * 32, dtype=torch.int32).reshape(2, 1, 40, 32)
    dhg_amd.save_page_truth(_record(labels), 1, "lab_p1", precision=0)
    got = np.load(tmp_path / "lab_p1_labels.npy")
    assert got.dtype == np.int32 and np.array_equal(got, labels[1, 0].numpy()) and json.loads((tmp_path / "lab_p1.json").read_text())["page"] == 1


# ---------------------------------------------------------------- write_page_file(truth=...) and the command line
def test_write_page_file_truth_uses_the_page_arguments(monkeypatch, tmp_path):
    from dhg_amd import checkpoint, inference, vis
    seen, saved, rounds = {}, [], []
    strokes = [np.zeros((40, 3), np.float32), np.zeros((56, 3), np.float32), np.zeros((24, 3), np.float32)]

    class Model:
        _cap = dict(max_B=2)

    def fake_align(model, st, text, sv, lengths=None, **kw):
        rounds.append((tuple(st.shape), tuple(text.shape), lengths))
        B, L = st.shape[:2]
        mean = torch.full((B, L // 8, text.shape[1]), 0.1)
        return dhg_amd.Alignment(mean, torch.zeros((B, L), dtype=torch.int32), None, lengths, 4)

    def fake_truth(st, al, prompts, lengths, slots, **kw):
        seen.update(shape=st.shape, token=al.clone(), prompts=prompts, lengths=lengths, slots=slots, **kw)
        return _record()

    monkeypatch.setattr(checkpoint, "load_model", lambda *a, **k: Model())
    monkeypatch.setattr(inference, "load_style", lambda *a: torch.zeros((1, 14, 1280)))
    monkeypatch.setattr(inference, "write_page", lambda text, style, model, **k: (torch.full((2, 1, 8, 8), 255.0), strokes))
    monkeypatch.setattr(inference, "align", fake_align)
    monkeypatch.setattr(vis, "save_page_png", lambda page, name: saved.append(name + ".png"))
    monkeypatch.setattr(truth, "page_truth", fake_truth)
    monkeypatch.setattr(truth, "save_page_truth", lambda rec, page, name: saved.append(name + ".json"))
    out = dhg_amd.write_page_file("on\n\n\nthree\nx", "s.npy", "c.yml", "m.pth", output="letter", pitch=50.0, lines_per_page=2, line_width=3.0,
                                  truth=True, truth_level="char", truth_labels=True)
    assert out is strokes and saved == ["letter_p0.png", "letter_p1.png", "letter_p0.json", "letter_p1.json"]
    assert rounds == [((2, 56, 3), (2, 6), [40, 56]), ((1, 24, 3), (1, 2), [24])]              # rounds of max_B lines
    tok = seen.pop("token")
    assert tuple(tok.shape) == (3, 56) and tok[0].tolist() == [0] * 40 + [-1] * 16 and tok[2].tolist() == [0] * 24 + [-1] * 32
    assert seen == dict(shape=(3, 56, 3), prompts=["on", "three", "x"], lengths=[40, 56, 24], slots=[0, 3, 4], level="char", labels=True, pages=2,
                        pitch=50.0, lines_per_page=2, line_width=3.0)
    saved.clear()
    dhg_amd.write_page_file("on\n\n\nthree\nx", "s.npy", "c.yml", "m.pth", output="letter")
    assert saved == ["letter_p0.png", "letter_p1.png"]                  # truth=False: today's files
    with pytest.raises(ValueError, match="truth_level"):
        dhg_amd.write_page_file("on", "s.npy", "c.yml", "m.pth", truth=True, truth_level="line")


def test_infer_cli_truth_dispatch_and_refusals(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake(text, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(text=text, output=output, **kw)
        return [np.zeros((8, 3), np.float32)] * 2

    monkeypatch.setattr(dhg_amd, "write_page_file", fake)
    f = tmp_path / "text.txt"
    f.write_text("Dear reader,\n\nthis is it.\n")
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp", "--output", "out", "--truth"])
    assert seen["truth"] is True and seen["truth_level"] == "word" and seen["truth_labels"] is False and "svg" not in seen
    seen.clear()
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp", "--truth", "--truth-level", "char", "--truth-labels", "--svg"])
    assert seen["truth"] is True and seen["truth_level"] == "char" and seen["truth_labels"] is True and seen["svg"] is True
    seen.clear()
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp"])
    assert not {"truth", "truth_level", "truth_labels"} & set(seen)      # without --truth: today's call, argument for argument
    for argv in (["Hello", "style.npy", "--truth"], ["--prompts-file", str(f), "style.npy", "--truth"],
                 ["--page-file", str(f), "style.npy", "--truth-labels"], ["--page-file", str(f), "style.npy", "--truth-level", "char"],
                 ["--page-file", str(f), "style.npy", "--truth", "--truth-level", "line"]):
        with pytest.raises(SystemExit):
            infer.main(argv)


# ---------------------------------------------------------------- the numpy statement of the rules, on cases worked out by hand
GEO = dict(pages=1, height=64, width=64, lines_per_page=2, margin_left=4.0, margin_top=8.0, pitch=24.0)


def _hand_line(dx, dy, n):
    """n strokes of (dx, dy), pen down, a lift on the last: segments 1 .. n-2 are drawn, between positions 0 .. n-2."""
    st = np.zeros((n, 3), np.float32)
    st[:, 0], st[:, 1], st[:, 2] = dx, dy, 0.3
    st[n - 1, 2] = 0.98
    return st


def test_ref_one_group_is_the_line_box():
    st = _hand_line(1.0, 0.5, 8)[None]                                   # positions (1, .5) .. (7, 3.5): segments 1..6
    r = truth_ref.truth_ref(st, np.zeros((1, 8), np.int32), 1, scale=2.0, labels=True, **GEO)
    assert r["scale"].tolist() == [2.0] and r["spans"].tolist() == [[[1, 7, 6]]]
    # ex = 6, ey = 3: oy = 8 + (24 - 6) / 2 = 17; the box is the line's ink box
    assert r["boxes"].tolist() == [[[4.0, 17.0, 16.0, 23.0]]] and r["ids"].tolist() == [1]
    lab = r["labels"][0]
    assert set(np.unique(lab).tolist()) == {0, 1} and lab[22, 4] == 1 and lab[17, 15] == 1 and lab[17, 4] == 0
    auto = truth_ref.truth_ref(st, np.zeros((1, 8), np.int32), 1, **GEO)
    assert auto["scale"][0] == np.float32(24.0) / np.float32(3.0) and auto["boxes"].tolist() == [[[4.0, 8.0, 52.0, 32.0]]]


def test_ref_groups_empty_group_and_unassigned_rows():
    st = _hand_line(1.0, 0.0, 10)[None]                                  # a flat line, positions x = 1 .. 9: segments 1..8
    g = np.array([[0, 0, 0, 0, 2, 2, -1, 7, 2, 0]], np.int32)            # group 1 never occurs; rows 6, 7 unassigned (-1, G <= 7)
    r = truth_ref.truth_ref(st, g, 3, scale=2.0, labels=True, **GEO)
    assert r["spans"].tolist() == [[[1, 4, 3], [0, 0, 0], [4, 9, 3]]]   # group 2 = rows 4, 5, 8: its span is their hull
    # xmin = 1, oy = 8 + 12 = 20 (ey = 0)
    assert r["boxes"].tolist() == [[[4.0, 20.0, 10.0, 20.0], [0.0] * 4, [10.0, 20.0, 20.0, 20.0]]]
    assert r["ids"].tolist() == [0, 1, 3]
    row = r["labels"][0, 20]                                             # pixel centres y = 20.5, x = c + .5; ink from x = 4 to 20
    assert row[3:9].tolist() == [1] * 6 and row[11:13].tolist() == [3, 3] and row[15:17].tolist() == [0, 0] and row[19] == 3 and row[23] == 0
    assert row[14] == 0 and row[13] == 3                                 # the joint at x = 14 between group 2 and unassigned ink
    everything = truth_ref.truth_ref(st, np.full((1, 10), 5, np.int32), 3, scale=2.0, labels=True, **GEO)
    assert not everything["boxes"].any() and not everything["spans"].any() and not everything["labels"].any() and everything["ids"].tolist() == [0]


def test_ref_lines_that_take_no_part_and_clamped_lengths():
    st = np.stack([_hand_line(1.0, 0.5, 8)] * 3)
    st[0, :, 2] = 0.3                                                   # no lift: nothing is drawn
    st[1, :, 2] = 0.98                                                  # every row a lift
    g = np.zeros((3, 8), np.int32)
    r = truth_ref.truth_ref(st, g, 2, [8, 8, 8], [0, 1, 5], labels=True, **GEO)      # line 2: a slot off the page
    assert not r["boxes"].any() and not r["spans"].any() and not r["labels"].any() and r["scale"].tolist() == [1.0] and len(r["ids"]) == 0
    a = truth_ref.truth_ref(st[2:], g[2:], 2, [99], **GEO)
    b = truth_ref.truth_ref(st[2:], g[2:], 2, [8], **GEO)
    assert np.array_equal(a["boxes"], b["boxes"]) and a["boxes"].any()
    assert not truth_ref.truth_ref(st[2:], g[2:], 2, [-3], **GEO)["spans"].any()


def test_ref_accept_rule_on_a_joint():
    """Two groups meeting at a joint: the pixels behind it are at the same distance from both, so both ids are accepted there
    and nowhere far from it; a device that swaps the two groups is caught."""
    st = _hand_line(1.0, 0.0, 10)[None]
    st[0, 5:, 1] = 1.0                                                   # a corner at position 4: x runs on, y starts to climb
    g = np.array([[0] * 5 + [1] * 5], np.int32)
    r = truth_ref.truth_ref(st, g, 2, scale=3.0, labels=True, **GEO)
    ink, size = truth_ref.accept_set_sizes(r)
    assert ink.sum() > 50 and (size[ink] > 1).any() and (size[~ink] >= 1).all()
    assert not truth_ref.label_errors(r["labels"], r).any()
    swapped = np.where(r["labels"] == 1, 2, np.where(r["labels"] == 2, 1, 0))
    assert truth_ref.label_errors(swapped, r).sum() > 20
    assert truth_ref.label_errors(np.zeros_like(r["labels"]), r).sum() > 20 and truth_ref.label_errors(np.full_like(r["labels"], 1), r).sum() > 20
    assert truth_ref.label_errors(np.full_like(r["labels"], 7), r).all()                 # an id that does not exist is never accepted


def test_ref_label_inputs_of_the_gpu_tests_are_not_vacuous():
    """Every label case of tests/test_gpu_truth.py built from groups of >= 8 rows at scale >= 1: at least 90 % of the ink pixels
    have a one-element accept set, and at least one pixel a larger one."""
    st, g = truth_ref.basic_batch()
    for kw in (dict(), dict(scale=1.5)):
        r = truth_ref.truth_ref(st, g, 5, truth_ref.BASIC_LENS, labels=True, **truth_ref.BASIC_GEO, **kw)
        assert float(r["scale"][0]) >= 1.0
        ink, size = truth_ref.accept_set_sizes(r)
        share = float((size[ink] == 1).mean())
        print("basic batch", kw, "scale", float(r["scale"][0]), "ink pixels", int(ink.sum()), "one-element accept sets", share)
        assert ink.sum() > 500 and share >= 0.9 and (size > 1).any()
        assert not truth_ref.label_errors(r["labels"], r).any()
        assert len(r["ids"]) >= 15 and (r["spans"][..., 2] > 0).sum() >= 15
    spread = truth_ref.truth_ref(st, g, 5, truth_ref.BASIC_LENS, [0, 2, 4, 6, 8], labels=True, **dict(truth_ref.BASIC_GEO, pages=3))
    st2, g2 = truth_ref.overlap_batch()
    overlap = truth_ref.truth_ref(st2, g2, 6, labels=True, **truth_ref.OVERLAP_GEO)
    st3, g3 = truth_ref.clamped_batch()
    clamped = truth_ref.truth_ref(st3, g3, 5, truth_ref.CLAMPED_LENS, labels=True, **truth_ref.BASIC_GEO)
    st4, g4 = truth_ref.nopart_batch()
    nopart = truth_ref.truth_ref(st4, g4, 5, None, truth_ref.NOPART_SLOTS, labels=True, **truth_ref.BASIC_GEO)
    assert not nopart["spans"][:3].any() and (nopart["spans"][3:, :, 2] > 0).all() and not clamped["spans"][1::2].any()
    for name, r in (("every other slot", spread), ("overlap", overlap), ("clamped lengths", clamped), ("lines that take no part", nopart)):
        ink, size = truth_ref.accept_set_sizes(r)
        share = float((size[ink] == 1).mean())
        print(name, "scale", float(r["scale"][0]), "ink pixels", int(ink.sum()), "one-element accept sets", share)
        assert float(r["scale"][0]) >= 1.0 and ink.sum() > 400 and share >= 0.9 and (size > 1).any()
    st, g = truth_ref.boundary_batch()
    r = truth_ref.truth_ref(st, g, truth_ref.BOUNDARY_G, **truth_ref.BOUNDARY_GEO)
    assert r["spans"][0, :, :2].tolist()[1:4] == [[15, 16], [16, 17], [17, 31]] and r["spans"][0, 9, :2].tolist() == [1023, 1025]
    assert r["spans"][1, 8, :2].tolist() == [1000, 1050] and (r["spans"][..., 2] > 0).sum() >= 20


# ---------------------------------------------------------------- truth_host.h alone under ASan + UBSan
def test_truth_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/truth_host_check.cpp (csrc/truth/truth_host.h, which asks csrc/page/page_host.h for the geometry) built with the
    host compiler under AddressSanitizer + UBSan where the toolchain links them (as tests/test_page_cpu.py builds its
    program), run on the CPU: the workspace size, every refusal, and (inside the program) a message buffer shorter than the
    message."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "truth_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "truth_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("truth_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    good = dict(N=3, L=40, G=5, P=2, H=160, W=256, lpp=3, ml=6.0, mt=4.0, pitch=48.0, lw=2.0, scale=0.0, null=0, mis=0, short=0)

    def run(**kw):
        a = {**good, **kw}
        r = subprocess.run([exe, *(str(a[k]) for k in good)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (kw, r.stdout + r.stderr)
        return r.stdout.strip()

    assert run() == f"ok {3 * 32 + 3 * 40 * 20}" and run(N=4096, L=4096, G=256, P=1, scale=0.5) == f"ok {4096 * 32 + 4096 * 4096 * 20}"
    assert run(N=3, L=7) == f"ok {(3 * 32 + 3 * 7 * 20 + 15) // 16 * 16}" and run(G=1).startswith("ok") and run(lw=0.5).startswith("ok")
    assert run(null=64 + 128 + 256).startswith("ok")                    # labels_out, lens and slots may be NULL
    for kw, what in ((dict(N=0), "N must"), (dict(N=4097), "N must"), (dict(L=0), "L must"), (dict(L=4097), "L must"), (dict(G=0), "G must"),
                     (dict(G=257), "G must"), (dict(P=0), "P must"), (dict(H=7), "H must"), (dict(W=4), "W must"), (dict(W=130), "multiple of 4"),
                     (dict(P=2 ** 31 // (160 * 256) + 1), "below 2^31"), (dict(P=2 ** 24, H=8, W=8), "launch grid"), (dict(lpp=0), "lines_per_page"),
                     (dict(pitch=0), "pitch"), (dict(pitch="nan"), "pitch"), (dict(ml=-1), "margin_left"), (dict(ml=128), "W - 2 margin_left"),
                     (dict(mt=-1), "margin_top"), (dict(mt="inf"), "margin_top"), (dict(lw=0.25), "line_width"), (dict(lw=17), "line_width"),
                     (dict(lw="nan"), "line_width"), (dict(scale=-1), "scale"), (dict(scale="nan"), "scale"),
                     (dict(null=1), "strokes is NULL"), (dict(null=2), "groups is NULL"), (dict(null=4), "boxes_out is NULL"),
                     (dict(null=8), "spans_out is NULL"), (dict(null=16), "scale_out is NULL"), (dict(null=32), "workspace is NULL"),
                     (dict(short=1), "workspace_bytes"), (dict(mis=32), "16-byte aligned"), (dict(mis=64), "16-byte aligned"),
                     (dict(mis=1), "4-byte aligned"), (dict(mis=2), "4-byte aligned"), (dict(mis=4), "4-byte aligned"), (dict(mis=8), "4-byte aligned"),
                     (dict(mis=16), "4-byte aligned"), (dict(mis=128), "4-byte aligned"), (dict(mis=256), "4-byte aligned")):
        out = run(**kw)
        assert out.startswith("err ") and what in out, (kw, out)
