"""Host side of the stroke encoder (include/dhw.h dhw_encode; dhg_amd.encode_strokes, read_strokes_xml, make_batches) that
needs no GPU: the CPU statement of the rules (tests/encode_ref.py) against the reference's recorded outputs
(tests/golden/encode_lines.npz, written by tools/make_encode_golden.py), the k = M / 5 identity, the lineStrokes reader, the
two symbols exported and bound, every argument rule of the C entry through the handle-less error path, make_batches on a
stubbed encoder, and every ValueError of the wrapper, raised before a device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, encode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "encode_lines.npz"))
CASES = sorted(int(k.split("_")[1]) for k in GOLDEN.files if k.startswith("points_"))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


# ---------------------------------------------------------------- the rules against the reference's recorded outputs
def test_golden_cases_are_the_ones_asked_for():
    assert [len(GOLDEN[f"points_{c}"]) for c in CASES] == [6, 7, 9, 40, 65, 66, 258, 333, 700, 1500, 400]
    for c in CASES:
        assert (GOLDEN[f"gaps_{c}"] >= 1e-9).all(), c                       # the merged set is decided well above rounding
        p = GOLDEN[f"points_{c}"]
        assert p.dtype == np.float32 and (p[:, :2] == np.rint(p[:, :2])).all() and p[-1, 2] == 1 and p[:, 2].sum() >= 2
    assert [c for c in CASES if GOLDEN[f"dropped_{c}"]] == [9, 10]


@pytest.mark.parametrize("c", CASES)
def test_encode_ref_matches_the_reference(c):
    gaps = []
    rows, ok = encode_ref.encode_rows(GOLDEN[f"points_{c}"], 3, gaps)
    want = GOLDEN[f"rows_{c}"]
    assert ok and rows.shape == want.shape                                   # lengths
    assert np.array_equal(rows[:, 2], want[:, 2])                            # pen, exactly
    assert np.abs(rows[:, :2] - want[:, :2]).max() <= 1e-12
    assert np.allclose([g for g, _, _ in gaps], GOLDEN[f"gaps_{c}"], rtol=0, atol=1e-12) and all(z <= k for _, z, k in gaps)
    L = int(GOLDEN["max_seq_len"])
    strokes, M, status = encode_ref.encode_ref(GOLDEN[f"points_{c}"], L=L)
    assert M == len(want) and (status != 0) == bool(GOLDEN[f"dropped_{c}"])
    assert status == {9: 4, 10: 8}.get(c, 0)                                 # too long for max_seq_len; an offset above 15
    if status == 0:
        assert np.array_equal(strokes, GOLDEN[f"padded_{c}"])                # the f32 rows and the (0, 0, 1) padding
    else:
        assert (strokes == np.array([0, 0, 1], np.float32)).all()


def test_merge_count_equals_the_references_for_every_row_count():
    assert all(M // 5 == int(M * 0.2) for M in range(4097))
    for n in (2, 6, 700, 4096):
        assert encode_ref.final_rows(n, 3) == encode.upper_bound_rows(n, 3)
    assert encode.upper_bound_rows(700, 3) == 359 and encode.upper_bound_rows(700, 0) == 699 and encode.upper_bound_rows(2, 8) == 1


def test_encode_ref_small_cases_by_hand():
    # n = 2, dx != dy: one row, std of {3, -4} = 3.5
    s, M, st = encode_ref.encode_ref(np.array([[0, 0, 0], [3, 4, 1]], np.float32), L=8, rounds=0)
    assert (M, st) == (1, 0) and s[0].tolist() == [np.float32(3 / 3.5), np.float32(-4 / 3.5), 1.0] and (s[1:] == [0, 0, 1]).all()
    # dx == dy: std 0
    assert encode_ref.encode_ref(np.array([[0, 0, 0], [2, -2, 1]], np.float32), L=8)[1:] == (1, 2)
    assert encode_ref.encode_ref(np.array([[0, 0, 0], [np.nan, 1, 1], [2, 2, 1]], np.float32), L=8)[1:] == (2, 2)
    assert encode_ref.encode_ref(np.zeros((1, 3), np.float32), L=8)[1:] == (0, 1)
    # ties: every key is exactly 0, the lowest j merge
    line = np.zeros((11, 3), np.float32)
    line[:, 0], line[:, 1], line[-1, 2] = np.arange(11) * 3, np.arange(11) * -1, 1
    rows, ok = encode_ref.encode_rows(line, 1)
    assert ok and len(rows) == 8 and np.allclose(rows[:2, 0] / rows[2, 0], 2) and np.allclose(rows[2:, 0], rows[2, 0])


# ---------------------------------------------------------------- the reader
def test_read_strokes_xml_gives_the_golden_points(tmp_path):
    pts = dhg_amd.read_strokes_xml(os.path.join(ROOT, "tests", "golden", "encode_line.xml"))
    assert pts.dtype == np.float32 and np.array_equal(pts, GOLDEN[f"points_{int(GOLDEN['xml_case'])}"])
    # file order is kept (no sort by time), every Stroke's last point is an end
    (tmp_path / "a.xml").write_text('<S><StrokeSet><Stroke><Point x="5" y="6" time="9"/><Point x="1" y="2" time="1"/></Stroke>'
                                    '<Stroke><Point x="7" y="8" time="0"/></Stroke></StrokeSet></S>')
    assert dhg_amd.read_strokes_xml(tmp_path / "a.xml").tolist() == [[5, 6, 0], [1, 2, 1], [7, 8, 1]]
    (tmp_path / "b.xml").write_text("<S><Other/></S>")
    with pytest.raises(ValueError, match="StrokeSet"):
        dhg_amd.read_strokes_xml(tmp_path / "b.xml")


# ---------------------------------------------------------------- the C-ABI
def test_encode_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bsize_t\s+dhw_encode_workspace_bytes\s*\(", header) and re.search(r"\bint\s+dhw_encode\s*\(", header)
    l = _lib.lib()
    for name in ("dhw_encode_workspace_bytes", "dhw_encode"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_encode.restype is C.c_int and l.dhw_encode_workspace_bytes.restype is C.c_size_t and len(_lib.SIGNATURES["dhw_encode"][1]) == 13
    for name in ("encode_strokes", "padded_lengths", "read_strokes_xml", "make_batches"):
        assert getattr(dhg_amd, name) is getattr(encode, name)


def test_encode_workspace_bytes_is_zero_outside_the_ranges():
    f = _lib.lib().dhw_encode_workspace_bytes
    for B, N in ((0, 8), (65536, 8), (1, 1), (1, 4097), (-1, -1)):
        assert f(B, N) == 0


def _call(**kw):
    a = dict(points=FAKE, counts=None, B=3, N=40, L=32, rounds=3, max_abs=15.0, strokes_out=FAKE, lens_out=FAKE, status_out=FAKE,
             workspace=FAKE, workspace_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = l.dhw_encode_workspace_bytes(a["B"], a["N"])
    rc = l.dhw_encode(a["points"], a["counts"], a["B"], a["N"], a["L"], a["rounds"], a["max_abs"], a["strokes_out"], a["lens_out"],
                      a["status_out"], a["workspace"], a["workspace_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


NAN, INF = float("nan"), float("inf")
BAD_C = [
    (dict(B=0), "B"), (dict(B=65536), "B"), (dict(N=1), "N"), (dict(N=4097), "N"), (dict(L=7), "L"), (dict(L=4097), "L"),
    (dict(rounds=-1), "rounds"), (dict(rounds=9), "rounds"),
    (dict(max_abs=0.0), "max_abs"), (dict(max_abs=-1.0), "max_abs"), (dict(max_abs=NAN), "max_abs"), (dict(max_abs=INF), "max_abs"),
    (dict(points=None), "points"), (dict(strokes_out=None), "strokes_out"), (dict(lens_out=None), "lens_out"), (dict(status_out=None), "status_out"),
    (dict(points=FAKE + 8), "16-byte aligned"), (dict(strokes_out=FAKE + 4), "16-byte aligned"), (dict(workspace=FAKE + 8), "16-byte aligned"),
    (dict(lens_out=FAKE + 2), "4-byte aligned"), (dict(status_out=FAKE + 1), "4-byte aligned"), (dict(counts=FAKE + 2), "counts"),
]


@pytest.mark.parametrize("bad,name", BAD_C)
def test_each_argument_rule_of_dhw_encode_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call.  (The
    workspace_bytes rule cannot be broken today: the size asked for is 0 at every shape.)"""
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_encode:"), (bad, msg)


def test_kernel_constants_match_the_wrapper():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "encode", "encode_host.h")).read()
    for name in ("ENCODE_MAX_B", "ENCODE_MAX_N", "ENCODE_MAX_L", "ENCODE_MAX_ROUNDS"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(encode, name)


# ---------------------------------------------------------------- ValueError before a device is touched
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


LINE = GOLDEN["points_3"]
BAD_WRAPPER = [
    (dict(lines=[]), "non-empty list"), (dict(lines=LINE), "non-empty list"), (dict(lines=[LINE[:, :2]]), r"lines\[0\] must be an \[n, 3\]"),
    (dict(lines=[LINE, LINE[:1]]), r"lines\[1\] must hold 2 to 4096 points, got 1"), (dict(lines=[np.zeros((4097, 3))]), "2 to 4096 points"),
    (dict(lines=[[LINE[:5]]]), r"lines\[0\]\[0\] must be an \[m, 2\] polyline"), (dict(lines=[[LINE[:1, :2]]]), "got 1"),
    (dict(L=7), r"L = 7 must lie in \[8, 4096\]"), (dict(L=4097), "L = 4097"), (dict(L=32.0), "L = 32.0 is not an integer"),
    (dict(rounds=-1), "rounds = -1"), (dict(rounds=9), r"rounds = 9 must lie in \[0, 8\]"), (dict(rounds=True), "rounds = True is not an integer"),
    (dict(max_abs=0), "max_abs = 0.0 must be finite and > 0"), (dict(max_abs=NAN), "max_abs = nan"), (dict(max_abs=INF), "max_abs = inf"),
    (dict(max_abs="15"), "max_abs = '15' is not a number"),
]


@pytest.mark.parametrize("kw,msg", BAD_WRAPPER)
def test_encode_strokes_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.encode_strokes(kw.pop("lines", [LINE]), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(L=8), dict(rounds=0, max_abs=1), dict(lines=[[LINE[:5, :2], LINE[5:9, :2]], LINE])])
def test_encode_strokes_valid_arguments_get_as_far_as_the_device(monkeypatch, kw):
    _no_device(monkeypatch)
    kw = dict(kw)
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.encode_strokes(kw.pop("lines", [LINE]), **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_encode_strokes_fails_loudly_without_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU path"):
        dhg_amd.encode_strokes([LINE])


def test_padded_lengths():
    assert dhg_amd.padded_lengths([0, 1, 8, 9, 359, 360]) == [8, 8, 8, 16, 360, 360]
    assert dhg_amd.padded_lengths(torch.tensor([21, 34], dtype=torch.int32)) == [24, 40]


# ---------------------------------------------------------------- make_batches on a stubbed encoder
def test_make_batches_shapes_drops_and_kept(monkeypatch):
    seen = {}

    def fake(lines, L=None, rounds=3, max_abs=15.0, device=None):
        seen.update(n=len(lines), L=L, rounds=rounds, max_abs=max_abs)
        st = torch.arange(len(lines) * L * 3, dtype=torch.float32).reshape(len(lines), L, 3)
        return st, torch.full((len(lines),), 5, dtype=torch.int32), torch.tensor([0, 4, 0, 8, 0], dtype=torch.int32)

    monkeypatch.setattr(encode, "encode_strokes", fake)
    texts = ["Hi there", "dropped by status", "x" * 12, "also dropped", "ok"]
    style = torch.arange(5, dtype=torch.float32).reshape(5, 1, 1).expand(5, 14, 1280)
    out = dhg_amd.make_batches([LINE] * 5, texts, style, max_seq_len=40, max_text_len=12)
    assert seen == dict(n=5, L=40, rounds=3, max_abs=15.0)
    assert set(out) == {"strokes", "text", "style", "kept"} and out["kept"] == [0, 4]       # 1 and 3 by status, 2 by len(text) >= 12
    assert out["strokes"].shape == (2, 40, 3) and out["strokes"].dtype == torch.float32 and out["strokes"][1, 0, 0] == 4 * 40 * 3
    assert out["text"].shape == (2, 12) and out["text"].dtype == torch.int64
    ids = dhg_amd.Tokenizer().encode("Hi there")
    assert out["text"][0].tolist() == ids + [0] * (12 - len(ids)) and out["text"][1].tolist()[:4] == dhg_amd.Tokenizer().encode("ok") + [0]
    assert out["style"].shape == (2, 14, 1280) and out["style"][:, 0, 0].tolist() == [0, 4]
    with pytest.raises(ValueError, match="texts must hold 5"):
        dhg_amd.make_batches([LINE] * 5, texts[:4], style)
    with pytest.raises(ValueError, match=r"style must be \[5, 14, 1280\]"):
        dhg_amd.make_batches([LINE] * 5, texts, style[:4])
