"""Host side of the vector output (include/dhw.h dhw_paths; dhg_amd.stroke_paths, page_svg, save_page_svg, write_page_file(svg=True))
that needs no GPU: the two symbols declared, exported and bound; every argument rule of the C entry through the handle-less
error path; every ValueError of stroke_paths, raised before a device is touched; the numpy statement of the rules
(tests/paths_ref.py) on cases that can be worked out by hand, its determinism rule, and that the inputs of the GPU tests are
not vacuous; page_svg against exact strings; infer.py --svg dispatch and refusal; and csrc/paths/paths_host.h alone under
AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, vector

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paths_ref  # noqa: E402
from paths_ref import F32  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- the C-ABI
def test_paths_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bsize_t\s+dhw_paths_workspace_bytes\s*\(", header) and re.search(r"\bint\s+dhw_paths\s*\(", header)
    l = _lib.lib()
    for name in ("dhw_paths_workspace_bytes", "dhw_paths"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_paths.restype is C.c_int and l.dhw_paths_workspace_bytes.restype is C.c_size_t and len(_lib.SIGNATURES["dhw_paths"][1]) == 24
    assert dhg_amd.stroke_paths is vector.stroke_paths and dhg_amd.page_svg is vector.page_svg and dhg_amd.save_page_svg is vector.save_page_svg
    assert dhg_amd.StrokePaths is vector.StrokePaths


def test_paths_workspace_bytes():
    f = _lib.lib().dhw_paths_workspace_bytes
    assert f(1, 1) == 16 and f(4, 488) == 16 and f(5, 8) == 32 and f(4096, 4096) == 4096 * 4
    assert f(0, 8) == 0 and f(4097, 8) == 0 and f(1, 0) == 0 and f(1, 4097) == 0 and f(-1, -1) == 0


def _call(**kw):
    a = dict(strokes=FAKE, lens=None, slots=None, N=3, L=40, P=2, H=160, W=256, lpp=3, ml=6.0, mt=4.0, pitch=48.0, scale=0.0, smooth=1, tol=0.25,
             rounds=4, points=FAKE, index=FAKE, counts=FAKE, scale_out=FAKE, boxes_out=FAKE, workspace=FAKE, workspace_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(l.dhw_paths_workspace_bytes(min(max(a["N"], 1), 4096), min(max(a["L"], 1), 4096)), 16)
    rc = l.dhw_paths(a["strokes"], a["lens"], a["slots"], a["N"], a["L"], a["P"], a["H"], a["W"], a["lpp"], a["ml"], a["mt"], a["pitch"], a["scale"],
                     a["smooth"], a["tol"], a["rounds"], a["points"], a["index"], a["counts"], a["scale_out"], a["boxes_out"], a["workspace"],
                     a["workspace_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


BAD_C = [
    (dict(N=0), "N"), (dict(N=4097), "N"), (dict(L=0), "L"), (dict(L=4097), "L"), (dict(P=0), "P"), (dict(H=7), "H"),
    (dict(W=4), "W"), (dict(W=130), "W"), (dict(P=2, H=2 ** 15, W=2 ** 15), "2\\^31"), (dict(P=2 ** 24, H=8, W=8), "launch grid"),
    (dict(lpp=0), "lines_per_page"), (dict(pitch=0.0), "pitch"), (dict(pitch=-1.0), "pitch"), (dict(pitch=NAN), "pitch"), (dict(pitch=INF), "pitch"),
    (dict(ml=-1.0), "margin_left"), (dict(ml=NAN), "margin_left"), (dict(ml=INF), "margin_left"), (dict(ml=128.0), "margin_left"),
    (dict(mt=-1.0), "margin_top"), (dict(mt=NAN), "margin_top"), (dict(mt=INF), "margin_top"),
    (dict(scale=-0.5), "scale"), (dict(scale=NAN), "scale"), (dict(scale=INF), "scale"),
    (dict(smooth=-1), "smooth"), (dict(smooth=9), "smooth"), (dict(rounds=-1), "rounds"), (dict(rounds=9), "rounds"),
    (dict(tol=-0.5), "tol"), (dict(tol=NAN), "tol"), (dict(tol=INF), "tol"),
    (dict(strokes=None), "strokes"), (dict(points=None), "points_out"), (dict(index=None), "index_out"), (dict(counts=None), "counts_out"),
    (dict(scale_out=None), "scale_out"), (dict(boxes_out=None), "boxes_out"), (dict(workspace=None), "workspace"),
    (dict(workspace_bytes=15), "workspace_bytes"),
    (dict(points=FAKE + 8), "16-byte aligned"), (dict(workspace=FAKE + 4), "16-byte aligned"),
    (dict(strokes=FAKE + 2), "4-byte aligned"), (dict(lens=FAKE + 1), "4-byte aligned"), (dict(slots=FAKE + 2), "4-byte aligned"),
    (dict(index=FAKE + 2), "4-byte aligned"), (dict(counts=FAKE + 1), "4-byte aligned"), (dict(scale_out=FAKE + 2), "4-byte aligned"),
    (dict(boxes_out=FAKE + 3), "4-byte aligned"),
]


@pytest.mark.parametrize("bad,name", BAD_C)
def test_each_argument_rule_of_dhw_paths_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_paths:"), (bad, msg)


def test_paths_workspace_one_byte_short_is_rejected():
    need = _lib.lib().dhw_paths_workspace_bytes(5, 40)
    rc, msg = _call(N=5, workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in msg


def test_kernel_constants_match_the_python_side():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "paths", "paths_host.h")).read()
    assert int(re.search(r"constexpr int PATHS_MAX_SMOOTH = (\d+);", src).group(1)) == vector.PATHS_MAX_SMOOTH
    assert int(re.search(r"constexpr int PATHS_MAX_ROUNDS = (\d+);", src).group(1)) == vector.PATHS_MAX_ROUNDS


# ---------------------------------------------------------------- ValueError before a device is touched
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


ST = np.zeros((3, 16, 3), np.float32)
SMALL = dict(height=96, width=128, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=40.0)
BAD_PATHS = [
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
    (dict(scale=0), "scale = 0.0 must be > 0"), (dict(scale=-1.0), "scale"), (dict(scale=INF), "scale = inf must be finite"),
    (dict(scale=True), "scale = True is not a number"),
    (dict(smooth=-1), "smooth = -1"), (dict(smooth=9), r"smooth = 9 must lie in \[0, 8\]"), (dict(smooth=1.0), "smooth = 1.0 is not an integer"),
    (dict(smooth=True), "smooth = True"), (dict(rounds=-1), "rounds = -1"), (dict(rounds=9), r"rounds = 9 must lie in \[0, 8\]"),
    (dict(rounds=2.0), "rounds = 2.0 is not an integer"),
    (dict(tol=-0.25), "tol = -0.25 must be >= 0"), (dict(tol=NAN), "tol = nan must be finite"), (dict(tol=INF), "tol = inf must be finite"),
    (dict(tol="1"), "tol = '1' is not a number"),
    (dict(strokes=np.zeros((16, 3), np.float32)), r"strokes must be \[N, L, 3\]"),
    (dict(strokes=np.zeros((2, 16, 2), np.float32)), r"strokes must be \[N, L, 3\]"),
    (dict(strokes=np.zeros((0, 16, 3), np.float32)), "N in"),
    (dict(strokes=np.zeros((1, 4097, 3), np.float32)), "L in"),
    (dict(strokes=torch.zeros((4097, 1, 3))), "N in"),
    (dict(strokes=np.zeros((3, 16, 3), np.int32)), "floating-point"),
    (dict(lengths=[16, 16]), "lengths must hold 3 entries"), (dict(lengths=[16, 0, 16]), r"lengths must be 3 integers in \[1, 16\]"),
    (dict(lengths=[16, 17, 16]), "lengths must be 3 integers"), (dict(lengths=[16, 8.0, 16]), r"lengths\[1\] = 8.0 is not an integer"),
    (dict(slots=[0, 1]), "slots must hold 3 entries"), (dict(slots=[0, 1.5, 2]), r"slots\[1\] = 1.5 is not an integer"),
    (dict(slots=[0, True, 2]), r"slots\[1\] = True"), (dict(slots=[0, 1, 2 ** 31]), "does not fit int32"),
    (dict(slots=[0, 1, 2 ** 26], height=64, width=64, lines_per_page=1), "below 2\\^31"),
]


@pytest.mark.parametrize("kw,msg", BAD_PATHS)
def test_stroke_paths_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    strokes = kw.pop("strokes", ST)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.stroke_paths(strokes, kw.pop("lengths", None), kw.pop("slots", None), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(lengths=[16, 1, 8]), dict(slots=[5, -1, 0]), dict(pages=3, scale=0.5), dict(smooth=0, tol=0, rounds=0),
                                dict(smooth=8, tol=3.5, rounds=8), dict(lengths=torch.tensor([1, 2, 3]), slots=torch.tensor([2, 1, 0]))])
def test_stroke_paths_valid_arguments_get_as_far_as_the_device(monkeypatch, kw):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.stroke_paths(ST, kw.pop("lengths", None), kw.pop("slots", None), **kw)


def test_stroke_paths_has_no_line_width():
    with pytest.raises(TypeError):
        dhg_amd.stroke_paths(ST, line_width=2.0)


# ---------------------------------------------------------------- the numpy statement of the rules, on cases worked out by hand
GEO = dict(pages=1, height=64, width=64, lines_per_page=2, margin_left=4.0, margin_top=8.0, pitch=24.0)


def _hand_line(dx, dy, n):
    """n strokes of (dx, dy), pen down, a lift on the last: positions 0 .. n-2 form one polyline of n - 1 points."""
    st = np.zeros((n, 3), np.float32)
    st[:, 0], st[:, 1], st[:, 2] = dx, dy, 0.3
    st[n - 1, 2] = 0.98
    return st


def test_ref_straight_run_of_five_points_keeps_its_ends_after_two_rounds():
    st = _hand_line(1.0, 0.0, 6)[None]                                   # positions (1,0) .. (5,0): five points in a row
    full = paths_ref.paths_ref(st, scale=2.0, smooth=0, tol=0.0, rounds=0, **GEO)
    assert full["counts"].tolist() == [[5, 1]] and full["index"][0, :5].tolist() == [[i, 0] for i in range(5)]
    assert full["points"][0, :5, 0].tolist() == [4.0, 6.0, 8.0, 10.0, 12.0]          # x = margin_left + (pos.x - 1) 2
    assert (full["points"][0, :5, 1] == 8.0 + 12.0).all()                              # a flat line: centred in slot 0
    assert full["points"][0, :5, 2].tolist() == [F32(2) / F32(6), F32(4) / F32(6), F32(4) / F32(6), F32(4) / F32(6), F32(2) / F32(6)]
    assert not full["points"][0, :5, 3].any() and not full["points"][0, 5:].any() and (full["index"][0, 5:] == -1).all()
    assert full["boxes"].tolist() == [[4.0, 20.0, 12.0, 20.0]] and full["scale"].tolist() == [2.0]
    one = paths_ref.paths_ref(st, scale=2.0, smooth=0, tol=0.0, rounds=1, **GEO)
    assert one["index"][0, :3].tolist() == [[0, 0], [2, 0], [4, 0]] and one["counts"].tolist() == [[3, 1]]   # ranks 1 and 3 go (d2 = 0 <= 0)
    two = paths_ref.paths_ref(st, scale=2.0, smooth=0, tol=0.0, rounds=2, **GEO)
    assert two["counts"].tolist() == [[2, 1]] and two["index"][0, :2].tolist() == [[0, 0], [4, 0]]
    assert two["points"][0, :2].tolist() == [[4.0, 20.0, F32(8) / F32(6), 0.0], [12.0, 20.0, F32(8) / F32(6), 0.0]]
    more = paths_ref.paths_ref(st, scale=2.0, smooth=3, tol=0.0, rounds=8, **GEO)      # smoothing a straight, evenly spaced run moves nothing
    assert np.array_equal(more["points"], two["points"]) and np.array_equal(more["index"], two["index"])


def test_ref_hairpin_takes_the_zero_length_branch():
    st = np.zeros((1, 4, 3), np.float32)                                 # positions A = (0,0), P = (1,0), A again; a lift ends it
    st[0, :, 2] = [0.3, 0.3, 0.3, 0.98]
    st[0, 1, 0], st[0, 2, 0] = 1.0, -1.0
    for tol, gone in ((2.0, True), (1.9375, False), (2.5, True), (0.0, False)):     # |AP| s = 2: removed iff 2 <= tol
        stats = {}
        r = paths_ref.paths_ref(st, scale=2.0, smooth=0, tol=tol, rounds=1, stats=stats, **GEO)
        assert stats == dict(len2_zero=1, evaluated=1)
        assert r["counts"].tolist() == [[2 if gone else 3, 1]], tol
        assert r["index"][0, :3, 0].tolist() == ([0, 2, -1] if gone else [0, 1, 2])
        ends = r["points"][0, [0, 1 if gone else 2]]
        assert ends[:, :2].tolist() == [[4.0, 20.0], [4.0, 20.0]]                       # A and A: coincident ends
        assert ends[:, 2:].tolist() == ([[0.0, 0.0]] * 2 if gone else [[F32(2) / F32(6), 0.0], [F32(-2) / F32(6), 0.0]])


def test_ref_lines_without_a_path_and_a_single_line():
    st = np.stack([_hand_line(1.0, 0.5, 8)] * 3)
    st[0, :, 2] = 0.3                                                   # no lift: nothing is drawn
    st[1, :, 2] = 0.98                                                  # every row a lift: polylines of one point each, no path
    r = paths_ref.paths_ref(st, [8, 8, 1], pages=2, **{k: v for k, v in GEO.items() if k != "pages"})
    assert r["counts"].tolist() == [[0, 0]] * 3 and not r["points"].any() and (r["index"] == -1).all() and not r["boxes"].any()
    assert r["scale"].tolist() == [1.0]                                  # no line takes part
    one = paths_ref.paths_ref(_hand_line(0.5, 1.0, 8)[None], smooth=0, rounds=0, **GEO)   # n = 1: positions (.5,1) .. (3.5,7)
    assert one["scale"][0] == F32(24.0) / F32(6.0) == 4.0 and one["counts"].tolist() == [[7, 1]]
    assert one["points"][0, :7, 0].tolist() == [4.0 + 2.0 * i for i in range(7)]
    assert one["points"][0, :7, 1].tolist() == [32.0 - 4.0 * i for i in range(7)]       # the stroke y axis points up
    assert one["boxes"].tolist() == [[4.0, 8.0, 16.0, 32.0]]
    lifted = _hand_line(1.0, 0.0, 9)[None]                               # a lift on row 4: polylines 0..3 and 4..7
    lifted[0, 4, 2] = 0.7
    r = paths_ref.paths_ref(lifted, smooth=0, rounds=0, scale=1.0, **GEO)
    assert r["counts"].tolist() == [[8, 2]] and r["index"][0, :8].tolist() == [[i, i // 4] for i in range(8)]
    off = paths_ref.paths_ref(lifted, None, [2], scale=1.0, **GEO)      # a slot off the page
    assert off["counts"].tolist() == [[0, 0]] and not off["boxes"].any()


PARAMS = dict(smooth=2, tol=0.5, rounds=4)


def test_ref_rule_10_batch_independence_and_line_order():
    st = paths_ref.basic_batch()
    lens, geo = paths_ref.BASIC_LENS, paths_ref.BASIC_GEO
    whole = paths_ref.paths_ref(st, lens, **PARAMS, **geo)
    for n, ln in enumerate(lens):
        alone = paths_ref.paths_ref(st[n:n + 1, :ln], None, [n], scale=float(whole["scale"][0]), **PARAMS, **geo)
        for k in ("points", "index"):
            assert np.array_equal(alone[k][0], whole[k][n, :ln]), (n, k)
        assert np.array_equal(alone["counts"][0], whole["counts"][n]) and np.array_equal(alone["boxes"][0].view(np.uint32), whole["boxes"][n].view(np.uint32))
    order = [3, 0, 4, 2, 1]
    perm = paths_ref.paths_ref(st[order], [lens[i] for i in order], order, **PARAMS, **geo)
    for k in ("points", "index", "counts", "boxes"):
        assert np.array_equal(perm[k], whole[k][order]), k
    assert np.array_equal(perm["scale"], whole["scale"])


def test_ref_inputs_of_the_gpu_tests_are_not_vacuous():
    st = paths_ref.basic_batch()
    before = paths_ref.paths_ref(st, paths_ref.BASIC_LENS, scale=2, smooth=2, tol=0.5, rounds=0, **paths_ref.BASIC_GEO)["counts"][:, 0]
    after = paths_ref.paths_ref(st, paths_ref.BASIC_LENS, scale=2, **PARAMS, **paths_ref.BASIC_GEO)["counts"][:, 0]
    print("basic batch, kept points per line:", before.tolist(), "->", after.tolist())
    assert before.tolist() == [39, 15, 32, 7, 39]
    assert (4 * (before - after) >= before).all() and (4 * after >= before).all()      # at least a quarter removed, at least a quarter kept
    smoothed = paths_ref.paths_ref(st, paths_ref.BASIC_LENS, scale=2, smooth=2, tol=0.5, rounds=0, **paths_ref.BASIC_GEO)["points"]
    raw = paths_ref.paths_ref(st, paths_ref.BASIC_LENS, scale=2, smooth=0, tol=0.5, rounds=0, **paths_ref.BASIC_GEO)["points"]
    assert not np.array_equal(smoothed, raw)                                           # and the smoothing moves points
    # the degenerate batch: lines without a path, and the len2 == 0 branch
    st, lens, slots = paths_ref.degenerate_batch()
    stats = {}
    r = paths_ref.paths_ref(st, lens, slots, stats=stats, **PARAMS, **paths_ref.DEGENERATE_GEO)
    print("degenerate batch:", stats, "counts of lines 0..7:", r["counts"][:8].tolist())
    assert stats["len2_zero"] >= 1 and stats["evaluated"] > stats["len2_zero"]
    assert r["counts"][:5].tolist() == [[0, 0]] * 5 and (r["counts"][5:, 0] >= 2).all() and len(st) == 70
    raw = paths_ref.paths_ref(st, lens, slots, smooth=0, tol=0.5, rounds=0, **paths_ref.DEGENERATE_GEO)
    p5 = raw["points"][5, :raw["counts"][5, 0], :2]
    assert np.array_equal(p5[0], p5[2]) and not np.array_equal(p5[0], p5[1])           # the hairpin line: A, P, A
    p6 = raw["points"][6, :raw["counts"][6, 0], :2]
    assert (np.diff(p6, axis=0) == 0).all(-1).sum() >= 4                               # the line with dx = dy = 0 rows: repeated points
    # the boundary batch: polylines end and start on both sides of the thread and wave boundaries, one spans the wave boundary
    st = paths_ref.boundary_batch()
    r = paths_ref.paths_ref(st, **PARAMS, **paths_ref.BOUNDARY_GEO)
    rows0 = set(r["index"][0, :r["counts"][0, 0], 0].tolist())
    assert not rows0 & {15, 16, 31, 1023, 1024, 1099} and {14, 30, 1022} <= rows0      # single points between two lifts are no path; ends stay
    poly1 = r["index"][1, :r["counts"][1, 0]]
    across = poly1[(poly1[:, 0] >= 990) & (poly1[:, 0] <= 1060)]
    assert len(set(across[:, 1].tolist())) == 1 and across[:, 0].min() < 1024 < across[:, 0].max()
    assert 0 < r["counts"][1, 0] < 1098 // 2


# ---------------------------------------------------------------- page_svg
def _record(**kw):
    """Two lines on two pages by hand: line 0 (slot 0) one polyline of three points, line 1 (slot 3: page 1) two polylines."""
    points = np.zeros((2, 6, 4), np.float32)
    index = np.full((2, 6, 2), -1, np.int32)
    points[0, :3] = [[10, 20, 1, 0.5], [16, 23, 1.5, 0.25], [19, 21.5, 0.5, -0.25]]
    index[0, :3] = [[0, 0], [2, 0], [3, 0]]
    points[1, :4] = [[4, 5, 0.125, 0], [4.75, 5, 0.125, 0], [8, 9.5, 0, 1], [8, 15.5, 0, 1]]
    index[1, :4] = [[0, 0], [1, 0], [4, 1], [5, 1]]
    a = dict(points=points, index=index, counts=np.array([[3, 1], [4, 2]], np.int32), scale=np.ones(1, np.float32), boxes=np.zeros((2, 4), np.float32),
             slots=[0, 3], pages=2, height=40, width=32, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=16.0)
    a.update(kw)
    return dhg_amd.StrokePaths(**a)


SVG_HEAD = '<svg xmlns="http://www.w3.org/2000/svg" width="32" height="40" viewBox="0 0 32 40">\n'
PATH_ATTRS = 'fill="none" stroke="black" stroke-width="{}" stroke-linecap="round" stroke-linejoin="round"'


def test_page_svg_exact_strings():
    rec = _record()
    assert dhg_amd.page_svg(rec, 0) == (
        SVG_HEAD + '<path id="line0" ' + PATH_ATTRS.format("2.00") + ' d="M 10.00 20.00 C 11.00 20.50 14.50 22.75 16.00 23.00 '
        'C 17.50 23.25 18.50 21.75 19.00 21.50"/>\n</svg>\n')
    assert dhg_amd.page_svg(rec, 0, curves=False, line_width=1.5, precision=1) == (
        SVG_HEAD + '<path id="line0" ' + PATH_ATTRS.format("1.5") + ' d="M 10.0 20.0 L 16.0 23.0 L 19.0 21.5"/>\n</svg>\n')
    assert dhg_amd.page_svg(rec, 1, precision=3) == (
        SVG_HEAD + '<path id="line1" ' + PATH_ATTRS.format("2.000") + ' d="M 4.000 5.000 C 4.125 5.000 4.625 5.000 4.750 5.000 '
        'M 8.000 9.500 C 8.000 10.500 8.000 14.500 8.000 15.500"/>\n</svg>\n')
    assert dhg_amd.page_svg(rec, 1, curves=False, precision=0) == (
        SVG_HEAD + '<path id="line1" ' + PATH_ATTRS.format("2") + ' d="M 4 5 L 5 5 M 8 10 L 8 16"/>\n</svg>\n')
    # tensors instead of arrays, slots as a tensor, slot n = n, and a line without points
    t = _record(points=torch.from_numpy(rec.points), index=torch.from_numpy(rec.index), counts=torch.from_numpy(rec.counts),
                slots=torch.tensor([0, 3], dtype=torch.int32))
    assert dhg_amd.page_svg(t, 0) == dhg_amd.page_svg(rec, 0) and dhg_amd.page_svg(t, 1) == dhg_amd.page_svg(rec, 1)
    both = dhg_amd.page_svg(_record(slots=None), 0, curves=False)
    assert both.count("<path") == 2 and both.index('id="line0"') < both.index('id="line1"')
    assert dhg_amd.page_svg(_record(slots=None), 1) == SVG_HEAD + "</svg>\n"
    assert dhg_amd.page_svg(_record(counts=np.array([[0, 0], [4, 2]], np.int32)), 0) == SVG_HEAD + "</svg>\n"
    assert dhg_amd.page_svg(_record(slots=[-1, 4]), 0) == SVG_HEAD + "</svg>\n"          # slots off the pages
    for bad, msg in ((dict(page=2), "page = 2"), (dict(page=-1), "page = -1"), (dict(page=0, precision=-1), "precision"),
                     (dict(page=0, line_width=0), "line_width"), (dict(page=0.0), "not an integer")):
        with pytest.raises(ValueError, match=msg):
            dhg_amd.page_svg(rec, **bad)


def test_save_page_svg_writes_the_document(tmp_path, monkeypatch):
    import xml.etree.ElementTree as ET
    monkeypatch.chdir(tmp_path)
    dhg_amd.save_page_svg(_record(), 1, "out_p1", curves=False)
    text = (tmp_path / "out_p1.svg").read_text()
    assert text == dhg_amd.page_svg(_record(), 1, curves=False)
    root = ET.fromstring(text)
    assert root.tag == "{http://www.w3.org/2000/svg}svg" and [p.get("id") for p in root] == ["line1"]


# ---------------------------------------------------------------- write_page_file(svg=...) and the command line
def test_write_page_file_svg_uses_the_page_arguments(monkeypatch, tmp_path):
    from dhg_amd import checkpoint, inference, vis
    seen, saved = {}, []
    strokes = [np.zeros((8, 3), np.float32), np.zeros((16, 3), np.float32)]
    monkeypatch.setattr(checkpoint, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(inference, "load_style", lambda *a: torch.zeros((1, 14, 1280)))
    monkeypatch.setattr(inference, "write_page", lambda text, style, model, **k: (torch.full((2, 1, 8, 8), 255.0), strokes))
    monkeypatch.setattr(vis, "save_page_png", lambda page, name: saved.append(name + ".png"))

    def fake_paths(st, lengths, slots, **kw):
        seen.update(shape=st.shape, lengths=lengths, slots=slots, **kw)
        return _record()

    monkeypatch.setattr(vector, "stroke_paths", fake_paths)
    monkeypatch.setattr(vector, "save_page_svg", lambda paths, page, name, **kw: saved.append((name + ".svg", kw)))
    out = dhg_amd.write_page_file("one\n\n\ntwo", "s.npy", "c.yml", "m.pth", output="letter", pitch=50.0, lines_per_page=2, line_width=3.0, svg=True)
    assert out is strokes and saved == ["letter_p0.png", "letter_p1.png", ("letter_p0.svg", dict(line_width=3.0)), ("letter_p1.svg", dict(line_width=3.0))]
    assert seen == dict(shape=(2, 16, 3), lengths=[8, 16], slots=[0, 3], pages=2, pitch=50.0, lines_per_page=2)
    saved.clear()
    dhg_amd.write_page_file("one\n\n\ntwo", "s.npy", "c.yml", "m.pth", output="letter")
    assert saved == ["letter_p0.png", "letter_p1.png"]                  # svg=False: today's files


def test_infer_cli_svg_dispatch_and_refusal(monkeypatch, tmp_path):
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
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp", "--output", "out", "--svg"])
    assert seen["svg"] is True and seen["output"] == "out" and seen["text"].startswith("Dear reader")
    seen.clear()
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp"])
    assert "svg" not in seen                                            # without --svg: today's call, argument for argument
    for argv in (["Hello", "style.npy", "--svg"], ["--prompts-file", str(f), "style.npy", "--svg"]):
        with pytest.raises(SystemExit):
            infer.main(argv)


# ---------------------------------------------------------------- paths_host.h alone under ASan + UBSan
def test_paths_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/paths_host_check.cpp (csrc/paths/paths_host.h, which asks csrc/page/page_host.h for the geometry) built with the
    host compiler under AddressSanitizer + UBSan where the toolchain links them (as tests/test_page_cpu.py builds its
    program), run on the CPU: the workspace size, every refusal, and (inside the program) a message buffer shorter than the
    message."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "paths_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "paths_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("paths_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    good = dict(N=3, L=40, P=2, H=160, W=256, lpp=3, ml=6.0, mt=4.0, pitch=48.0, scale=0.0, smooth=1, tol=0.25, rounds=4, null=0, mis=0, short=0)

    def run(**kw):
        a = {**good, **kw}
        r = subprocess.run([exe, *(str(a[k]) for k in good)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (kw, r.stdout + r.stderr)
        return r.stdout.strip()

    assert run() == "ok 16" and run(N=4096, L=4096, P=1, scale=0.5) == f"ok {4096 * 4}" and run(N=5) == "ok 32"
    assert run(smooth=0, tol=0, rounds=0).startswith("ok") and run(smooth=8, tol=100, rounds=8).startswith("ok")
    assert run(null=128 + 256).startswith("ok")                         # lens and slots may be NULL
    for kw, what in ((dict(N=0), "N must"), (dict(N=4097), "N must"), (dict(L=0), "L must"), (dict(L=4097), "L must"), (dict(P=0), "P must"),
                     (dict(H=7), "H must"), (dict(W=4), "W must"), (dict(W=130), "multiple of 4"),
                     (dict(P=2 ** 31 // (160 * 256) + 1), "below 2^31"), (dict(P=2 ** 24, H=8, W=8), "launch grid"), (dict(lpp=0), "lines_per_page"),
                     (dict(pitch=0), "pitch"), (dict(pitch="nan"), "pitch"), (dict(ml=-1), "margin_left"), (dict(ml=128), "W - 2 margin_left"),
                     (dict(mt=-1), "margin_top"), (dict(mt="inf"), "margin_top"), (dict(scale=-1), "scale"), (dict(scale="nan"), "scale"),
                     (dict(smooth=-1), "smooth must"), (dict(smooth=9), "smooth must"), (dict(rounds=-1), "rounds must"), (dict(rounds=9), "rounds must"),
                     (dict(tol=-1), "tol must"), (dict(tol="nan"), "tol must"), (dict(tol="inf"), "tol must"),
                     (dict(null=1), "strokes is NULL"), (dict(null=2), "points_out is NULL"), (dict(null=4), "index_out is NULL"),
                     (dict(null=8), "counts_out is NULL"), (dict(null=16), "scale_out is NULL"), (dict(null=32), "boxes_out is NULL"),
                     (dict(null=64), "workspace is NULL"), (dict(short=1), "workspace_bytes"), (dict(mis=2), "16-byte aligned"),
                     (dict(mis=64), "16-byte aligned"), (dict(mis=1), "4-byte aligned"), (dict(mis=4), "4-byte aligned"), (dict(mis=8), "4-byte aligned"),
                     (dict(mis=16), "4-byte aligned"), (dict(mis=32), "4-byte aligned"), (dict(mis=128), "4-byte aligned"), (dict(mis=256), "4-byte aligned")):
        out = run(**kw)
        assert out.startswith("err ") and what in out, (kw, out)
