"""Host side of the page compositor (include/dhw.h dhw_page; dhg_amd.render_page, wrap_text, write_page) that needs no GPU:
word wrap; every ValueError of render_page / write_page, raised before a device is touched; the two symbols exported and
bound; every argument rule of the C entry through the handle-less error path; infer.py --page-file dispatch and refusals;
the CPU statement of the rules (tests/page_ref.py) on cases that can be worked out by hand; and csrc/page/page_host.h alone
under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec, vis

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


# ---------------------------------------------------------------- wrap_text
def test_wrap_text_greedy():
    lines, slots = dhg_amd.wrap_text("the quick brown fox jumps over the lazy dog", 10)
    assert lines == ["the quick", "brown fox", "jumps over", "the lazy", "dog"] and slots == [0, 1, 2, 3, 4]
    assert dhg_amd.wrap_text("  spaces   collapse \t here ", 40) == (["spaces collapse here"], [0])
    assert dhg_amd.wrap_text("exactly ten", 11) == (["exactly ten"], [0])          # a line may be max_chars long
    assert dhg_amd.wrap_text("exactly ten", 10) == (["exactly", "ten"], [0, 1])
    assert dhg_amd.wrap_text("", 40) == ([], []) and dhg_amd.wrap_text(" \n \n", 40) == ([], [])
    for text in ("a bb ccc dddd eeeee ffffff ggggggg", "one\ntwo three four five six seven eight nine ten"):
        for mc in range(1, 20):
            lines, slots = dhg_amd.wrap_text(text, mc)
            assert all(1 <= len(ln) <= mc for ln in lines) and "".join(lines).replace(" ", "") == text.replace(" ", "").replace("\n", "")
            assert len(slots) == len(lines) and all(b > a for a, b in zip(slots, slots[1:]))


def test_wrap_text_long_words_are_split_hard():
    assert dhg_amd.wrap_text("abcdefghij", 4) == (["abcd", "efgh", "ij"], [0, 1, 2])
    assert dhg_amd.wrap_text("hi abcdefghij k", 4) == (["hi", "abcd", "efgh", "ij k"], [0, 1, 2, 3])   # the rest of a split word takes more words
    assert dhg_amd.wrap_text("abcdefgh", 4) == (["abcd", "efgh"], [0, 1])                             # no empty tail
    assert dhg_amd.wrap_text("x" * 100)[0] == ["x" * 40, "x" * 40, "x" * 20]


def test_wrap_text_paragraph_gaps_and_newlines():
    lines, slots = dhg_amd.wrap_text("Dear reader,\n\nthis is the first paragraph of it\nand a forced break.\n\n\nBye\n", 20)
    assert lines == ["Dear reader,", "this is the first", "paragraph of it", "and a forced break.", "Bye"]
    assert slots == [0, 2, 3, 4, 7]                                   # one blank line skips one slot, two skip two; the final newline adds none
    assert dhg_amd.wrap_text("\nlate start", 40) == (["late start"], [1])
    assert dhg_amd.wrap_text("a\r\n\r\nb", 40) == (["a", "b"], [0, 2])


def test_wrap_text_limits():
    assert dhg_amd.wrap_text("y" * 48, 48) == (["y" * 48], [0]) and dhg_amd.wrap_text("ab", 1) == (["a", "b"], [0, 1])
    for bad in (0, 49, -1, 40.0, True, None):
        with pytest.raises(ValueError, match="max_chars"):
            dhg_amd.wrap_text("hello", bad)
    for bad in (None, b"bytes", ["a"]):
        with pytest.raises(ValueError, match="text must be a str"):
            dhg_amd.wrap_text(bad)


# ---------------------------------------------------------------- ValueError before a device is touched
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


ST = np.zeros((3, 16, 3), np.float32)
BAD_GEOMETRY = [
    (dict(pages=0), "pages = 0"), (dict(pages=1.0), "pages = 1.0 is not an integer"), (dict(pages=True), "not an integer"),
    (dict(height=7), "height = 7"), (dict(height=96.0), "not an integer"),
    (dict(width=4), "width = 4"), (dict(width=130), "width = 130 must be a multiple of 4"),
    (dict(pages=2, height=2 ** 15, width=2 ** 15), "below 2\\^31"),
    (dict(pages=2 ** 24, height=8, width=8, margin_left=0), "launch grid"),
    (dict(lines_per_page=0), "lines_per_page = 0"), (dict(lines_per_page=2.5), "not an integer"),
    (dict(pitch=0), "pitch = 0.0 must be > 0"), (dict(pitch=-3.0), "pitch"), (dict(pitch=float("nan")), "pitch = nan must be finite"),
    (dict(pitch="92"), "pitch = '92' is not a number"),
    (dict(margin_left=-1), "margin_left = -1.0"), (dict(margin_left=float("inf")), "margin_left = inf must be finite"),
    (dict(margin_top=-0.5), "margin_top = -0.5"), (dict(margin_top=float("nan")), "margin_top"),
    (dict(width=128, margin_left=64), "leaves no room"), (dict(width=128, margin_left=70.5), "leaves no room"),
    (dict(line_width=0.25), "line_width = 0.25"), (dict(line_width=16.5), "line_width"), (dict(line_width=float("nan")), "line_width"),
    (dict(scale=0), "scale = 0.0 must be > 0"), (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale = inf must be finite"),
    (dict(scale=True), "scale = True is not a number"),
]
BAD_RENDER = BAD_GEOMETRY + [
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
    (dict(slots=[0, 1, 2 ** 26], height=64, width=64, lines_per_page=1), "below 2\\^31"),      # pages=None: as many as the largest slot asks for
]
SMALL = dict(height=96, width=128, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=40.0)


@pytest.mark.parametrize("kw,msg", BAD_RENDER)
def test_render_page_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    strokes = kw.pop("strokes", ST)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.render_page(strokes, kw.pop("lengths", None), kw.pop("slots", None), **kw)


@pytest.mark.parametrize("kw", [dict(), dict(lengths=[16, 1, 8]), dict(slots=[5, -1, 0]), dict(pages=3, scale=0.5), dict(slots=np.array([0, 2, 4])),
                                dict(lengths=torch.tensor([1, 2, 3]), slots=torch.tensor([2, 1, 0])), dict(margin_left=0, margin_top=0, line_width=16)])
def test_render_page_valid_arguments_get_as_far_as_the_device(monkeypatch, kw):
    _no_device(monkeypatch)
    kw = {**SMALL, **kw}
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.render_page(ST, kw.pop("lengths", None), kw.pop("slots", None), **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_render_page_fails_loudly_without_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU path"):
        dhg_amd.render_page(ST)


def _model():
    m = dhg_amd.DiffusionModel(1, c2=48, precision="fp32", max_B=2, max_L=64, max_Lt=8).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(1, c2=48).items()})
    return m


STYLE = torch.zeros((1, 14, 1280))
BAD_WRITE = BAD_GEOMETRY + [
    (dict(text=""), "holds no word"), (dict(text=" \n\n "), "holds no word"), (dict(text=7), "text must be a str"),
    (dict(max_chars=0), "max_chars = 0"), (dict(max_chars=49), r"max_chars = 49 must lie in \[1, 48\]"),
    (dict(candidates=0), "candidates"), (dict(steps=0), "steps = 0"), (dict(steps=61), "steps = 61"), (dict(T=0), "T = 0"),
    (dict(first_sample=-1), "first_sample = -1"), (dict(candidates=2, levels=[60]), r"levels\[0\] = 60"),
    (dict(diffusion_mode="old"), "diffusion_mode"),
    (dict(style=torch.zeros((2, 14, 1280))), "style_vector"), (dict(style=torch.zeros((14, 1280))), "style_vector"),
    (dict(text="a\n" + "\n" * 2 ** 14 + "b", height=512, width=512, lines_per_page=1), "below 2\\^31"),   # the pages the text needs
]


@pytest.mark.parametrize("kw,msg", BAD_WRITE)
def test_write_page_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch)
    monkeypatch.setattr(m, "_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device was touched")))
    kw = {**SMALL, **kw}
    text, style = kw.pop("text", "Hello there\n\nworld"), kw.pop("style", STYLE)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.write_page(text, style, m, **kw)


def test_write_page_samples_in_rounds_within_the_batch_capacity(monkeypatch):
    """Lines go to infer_batch at most max_B at a time, round i0 with first_sample + i0 * candidates; the page call gets every
    line's length and the slots of wrap_text."""
    from dhg_amd import inference
    calls, page = [], {}

    def fake_batch(prompts, sv, model, **kw):
        calls.append((list(prompts), kw))
        return [np.zeros((8 * (1 + len(p)), 3), np.float32) for p in prompts]

    def fake_page(strokes, lengths, slots, **kw):
        page.update(shape=strokes.shape, lengths=lengths, slots=slots, **kw)
        return "pages", "scale", "boxes"

    monkeypatch.setattr(inference, "infer_batch", fake_batch)
    monkeypatch.setattr(vis, "render_page", fake_page)
    m = _model()
    text = "aa bb cc dd ee\n\nff"
    out, strokes = dhg_amd.write_page(text, STYLE, m, max_chars=2, seed=5, first_sample=10, pitch=50.0)
    assert out == "pages" and [c[0] for c in calls] == [["aa", "bb"], ["cc", "dd"], ["ee", "ff"]]
    assert [c[1]["first_sample"] for c in calls] == [10, 12, 14] and all(c[1]["seed"] == 5 and c[1]["candidates"] == 1 for c in calls)
    assert len(strokes) == 6 and page["shape"] == (6, 24, 3) and page["lengths"] == [24] * 6 and page["slots"] == [0, 1, 2, 3, 4, 6]
    assert page["pitch"] == 50.0 and page["pages"] is None and page["scale"] is None
    calls.clear()
    dhg_amd.write_page(text, STYLE, m, max_chars=2, candidates=3, steps=4, first_sample=1)
    assert [c[1]["first_sample"] for c in calls] == [1, 7, 13] and all(c[1]["steps"] == 4 and c[1]["candidates"] == 3 for c in calls)


# ---------------------------------------------------------------- the C-ABI
def test_page_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bsize_t\s+dhw_page_workspace_bytes\s*\(", header) and re.search(r"\bint\s+dhw_page\s*\(", header)
    l = _lib.lib()
    for name in ("dhw_page_workspace_bytes", "dhw_page"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_page.restype is C.c_int and l.dhw_page_workspace_bytes.restype is C.c_size_t and len(_lib.SIGNATURES["dhw_page"][1]) == 20
    assert dhg_amd.render_page is vis.render_page and callable(vis.save_page_png)
    for name in ("wrap_text", "write_page", "write_page_file"):
        assert callable(getattr(dhg_amd, name)), name


def test_page_workspace_bytes():
    f = _lib.lib().dhw_page_workspace_bytes
    assert f(1, 1) == 32 + 16 and f(64, 488) == 64 * 32 + 64 * 488 * 16 and f(4096, 4096) == 4096 * 32 + 4096 * 4096 * 16
    assert f(0, 8) == 0 and f(4097, 8) == 0 and f(1, 0) == 0 and f(1, 4097) == 0 and f(-1, -1) == 0


def _call(**kw):
    a = dict(strokes=FAKE, lens=None, slots=None, N=3, L=40, P=2, H=160, W=256, lpp=3, ml=6.0, mt=4.0, pitch=48.0, lw=2.0, scale=0.0,
             pages=FAKE, scale_out=FAKE, boxes_out=FAKE, workspace=FAKE, workspace_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(l.dhw_page_workspace_bytes(min(max(a["N"], 1), 4096), min(max(a["L"], 1), 4096)), 16)
    rc = l.dhw_page(a["strokes"], a["lens"], a["slots"], a["N"], a["L"], a["P"], a["H"], a["W"], a["lpp"], a["ml"], a["mt"], a["pitch"], a["lw"],
                    a["scale"], a["pages"], a["scale_out"], a["boxes_out"], a["workspace"], a["workspace_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


NAN, INF = float("nan"), float("inf")
BAD_C = [
    (dict(N=0), "N"), (dict(N=4097), "N"), (dict(L=0), "L"), (dict(L=4097), "L"), (dict(P=0), "P"), (dict(H=7), "H"),
    (dict(W=4), "W"), (dict(W=130), "W"), (dict(P=2, H=2 ** 15, W=2 ** 15), "2\\^31"), (dict(P=2 ** 24, H=8, W=8), "launch grid"),
    (dict(lpp=0), "lines_per_page"), (dict(pitch=0.0), "pitch"), (dict(pitch=-1.0), "pitch"), (dict(pitch=NAN), "pitch"), (dict(pitch=INF), "pitch"),
    (dict(ml=-1.0), "margin_left"), (dict(ml=NAN), "margin_left"), (dict(ml=INF), "margin_left"), (dict(ml=128.0), "margin_left"),
    (dict(mt=-1.0), "margin_top"), (dict(mt=NAN), "margin_top"), (dict(mt=INF), "margin_top"),
    (dict(lw=0.25), "line_width"), (dict(lw=16.5), "line_width"), (dict(lw=NAN), "line_width"),
    (dict(scale=-0.5), "scale"), (dict(scale=NAN), "scale"), (dict(scale=INF), "scale"),
    (dict(strokes=None), "strokes"), (dict(pages=None), "pages"), (dict(scale_out=None), "scale_out"), (dict(boxes_out=None), "boxes_out"),
    (dict(workspace=None), "workspace"), (dict(workspace_bytes=15), "workspace_bytes"),
    (dict(pages=FAKE + 8), "16-byte aligned"), (dict(workspace=FAKE + 4), "16-byte aligned"), (dict(scale_out=FAKE + 2), "4-byte aligned"),
]


@pytest.mark.parametrize("bad,name", BAD_C)
def test_each_argument_rule_of_dhw_page_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_page:"), (bad, msg)


def test_page_workspace_one_byte_short_is_rejected():
    need = _lib.lib().dhw_page_workspace_bytes(3, 40)
    rc, msg = _call(workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in msg


def test_kernel_constants_match_the_header():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "page", "page_host.h")).read()
    assert int(re.search(r"constexpr int PAGE_MAX_N = (\d+);", src).group(1)) == vis.PAGE_MAX_N
    assert int(re.search(r"constexpr int PAGE_MAX_L = (\d+);", src).group(1)) == vis.PAGE_MAX_L


# ---------------------------------------------------------------- the command line
def test_infer_cli_page_file_dispatch_and_refusals(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake(text, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(text=text, source=source, experiment_path=experiment_path, output=output, mode=mode, **kw)
        return [np.zeros((8, 3), np.float32)] * 2

    monkeypatch.setattr(dhg_amd, "write_page_file", fake)
    f = tmp_path / "text.txt"
    f.write_text("Dear reader,\n\nthis is it.\n")
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp", "--output", "out"])
    assert seen["text"] == "Dear reader,\n\nthis is it.\n" and seen["source"] == "style.npy" and seen["output"] == "out" and seen["experiment_path"] == "exp"
    assert "steps" not in seen and "candidates" not in seen and seen["seed"] == 0 and seen["precision"] == "bf16"
    seen.clear()
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp", "--steps", "12", "--candidates", "3", "--seed", "4"])
    assert seen["steps"] == 12 and seen["candidates"] == 3 and seen["seed"] == 4
    seen.clear()
    infer.main(["--page-file", str(f), "style.npy", "--save-strokes", str(tmp_path / "s.npy")])
    assert np.load(tmp_path / "s.npy").shape == (2, 8, 3)
    empty = tmp_path / "empty.txt"
    empty.write_text(" \n\n")
    for bad in (["--score", "old.npy"], ["--align", "old.npy"], ["--restyle", "old.npy"], ["--prompts-file", str(f)], ["extra"]):
        with pytest.raises(SystemExit):
            infer.main(["--page-file", str(f), "style.npy", *bad])
    for argv in (["--page-file", str(f)], ["--page-file", str(empty), "style.npy"]):
        with pytest.raises(SystemExit):
            infer.main(argv)


def test_save_page_png_rounds(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    img = np.full((1, 8, 12), 255.0, np.float32)
    img[0, 3, :5] = [0.4, 0.5, 1.5, 2.5, 254.6]
    vis.save_page_png(torch.from_numpy(img), "p")
    got = np.asarray(Image.open(tmp_path / "p.png"))
    assert got.shape == (8, 12) and got.dtype == np.uint8 and got[3, :5].tolist() == [0, 0, 2, 2, 255] and (np.delete(got, 3, axis=0) == 255).all()


# ---------------------------------------------------------------- the CPU statement of the rules, on cases worked out by hand
def _hand_line(dx, dy, n=6):
    """n strokes of (dx, dy), pen down, a lift on the last: segments 1 .. n-2 are drawn, n-2 of them."""
    st = np.zeros((n, 3), np.float32)
    st[:, 0], st[:, 1], st[:, 2] = dx, dy, 0.3
    st[n - 1, 2] = 0.98
    return st


def test_page_ref_by_hand():
    geo = dict(pages=1, height=64, width=64, lines_per_page=2, margin_left=4.0, margin_top=8.0, pitch=24.0)
    # line 0: a horizontal stroke 8 units long (4 drawn segments of 2); line 1: a vertical one 12 units high
    st = np.stack([_hand_line(2.0, 0.0), _hand_line(0.0, 3.0)])
    (img,), s, boxes, counts = page_ref.page_ref(st, **geo)
    assert counts == [4, 4] and s.dtype == np.float32
    assert s == np.float32(24.0) / np.float32(12.0) == 2.0                # the height of line 1 limits: 56 / 8 = 7 for line 0
    assert boxes[0].tolist() == [4.0, 8.0 + 12.0, 4.0 + 16.0, 20.0]        # zero height: centred in its slot
    assert boxes[1].tolist() == [4.0, 32.0, 4.0, 56.0]                    # fills its slot's height
    assert img[20, 10] == 255.0 * (1 - 1.0) and img[19, 10] == 0.0         # on the stroke (centre 0.5 away: coverage clamps to 1)
    assert img[17, 10] == 255.0 and img[18, 10] == 255.0 * (1 - 0.0)       # 1.5 px away: coverage 0 at line_width 2
    assert img[40, 4] == 0.0 and img[40, 6] == 255.0 and (img[:, 30:] == 255).all() and (img[:8] == 255).all()
    # explicit scale: no part of the scale rule applies; ink past the page is clipped, a slot off the pages draws nothing
    (img2,), s2, boxes2, counts2 = page_ref.page_ref(st, slots=[1, 2], scale=10.0, **geo)
    assert s2 == np.float32(10) and counts2 == [4, 0] and boxes2[1].tolist() == [0, 0, 0, 0]
    assert boxes2[0].tolist() == [4.0, 44.0, 84.0, 44.0] and img2[44, 63] == 0.0 and img2[43, 63] == 0.0 and img2[41, 63] == 255.0
    # nothing draws: white, scale 1
    none = np.stack([_hand_line(1.0, 1.0)])
    none[0, :, 2] = 0.3
    (img3,), s3, boxes3, counts3 = page_ref.page_ref(none, **geo)
    assert (img3 == 255).all() and s3 == np.float32(1) and counts3 == [0] and not boxes3.any()
    # a dot alone: s_n = +inf, so s = 1; it sits at the left margin in the middle of its slot
    dot = np.stack([_hand_line(0.0, 0.0)])
    (img4,), s4, boxes4, _ = page_ref.page_ref(dot, **geo)
    assert s4 == np.float32(1) and boxes4[0].tolist() == [4.0, 20.0, 4.0, 20.0] and img4[19, 3] < 255 and img4[19, 3] == img4[20, 4]
    # the page of all lines is the minimum of the pages of each line alone at the shared scale
    alone = [page_ref.page_ref(st[n:n + 1], slots=[n], scale=float(s), **geo)[0][0] for n in range(2)]
    assert np.array_equal(img, np.minimum(alone[0], alone[1]))


# ---------------------------------------------------------------- page_host.h alone under ASan + UBSan
def test_page_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/page_host_check.cpp (csrc/page/page_host.h only) built with the host compiler under AddressSanitizer + UBSan
    where the toolchain links them (as tests/test_ddim_cpu.py builds its program), run on the CPU: the workspace size, every
    refusal, and (inside the program) a message buffer shorter than the message."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "page_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "page_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("page_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    good = dict(N=3, L=40, P=2, H=160, W=256, lpp=3, ml=6.0, mt=4.0, pitch=48.0, lw=2.0, scale=0.0, null=0, mis=0, short=0)

    def run(**kw):
        a = {**good, **kw}
        r = subprocess.run([exe, *(str(a[k]) for k in good)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (kw, r.stdout + r.stderr)
        return r.stdout.strip()

    assert run() == f"ok {3 * 32 + 3 * 40 * 16}"
    assert run(N=4096, L=4096, P=1, scale=0.5) == f"ok {4096 * 32 + 4096 * 4096 * 16}"
    assert run(P=2 ** 31 // (160 * 256) - 1).startswith("ok") and run(ml=127.9375).startswith("ok") and run(lw=0.5, ml=0, mt=0).startswith("ok")
    for kw, what in ((dict(N=0), "N must"), (dict(N=4097), "N must"), (dict(L=0), "L must"), (dict(L=4097), "L must"), (dict(P=0), "P must"),
                     (dict(P=-2 ** 31), "P must"), (dict(H=7), "H must"), (dict(W=4), "W must"), (dict(W=130), "multiple of 4"),
                     (dict(P=2 ** 31 // (160 * 256) + 1), "below 2^31"), (dict(P=2 ** 30, H=2 ** 30, W=2 ** 30), "below 2^31"),
                     (dict(P=2 ** 24, H=8, W=8), "launch grid"), (dict(P=1, H=2 ** 23, W=8), "launch grid"), (dict(lpp=0), "lines_per_page"),
                     (dict(pitch=0), "pitch"), (dict(pitch="nan"), "pitch"), (dict(pitch="inf"), "pitch"), (dict(ml=-1), "margin_left"),
                     (dict(ml="nan"), "margin_left"), (dict(ml=128), "W - 2 margin_left"), (dict(mt=-1), "margin_top"), (dict(mt="inf"), "margin_top"),
                     (dict(lw=0.25), "line_width"), (dict(lw=17), "line_width"), (dict(lw="nan"), "line_width"), (dict(scale=-1), "scale"),
                     (dict(scale="nan"), "scale"), (dict(scale="inf"), "scale"), (dict(null=1), "strokes is NULL"), (dict(null=2), "pages is NULL"),
                     (dict(null=4), "scale_out is NULL"), (dict(null=8), "boxes_out is NULL"), (dict(null=16), "workspace is NULL"),
                     (dict(short=1), "workspace_bytes"), (dict(mis=2), "16-byte aligned"), (dict(mis=16), "16-byte aligned"),
                     (dict(mis=4), "4-byte aligned"), (dict(mis=8), "4-byte aligned")):
        out = run(**kw)
        assert out.startswith("err ") and what in out, (kw, out)
