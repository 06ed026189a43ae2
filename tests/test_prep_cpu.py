"""Host side of the writer-image preparation (include/dhw.h dhw_prep; dhg_amd.prepare_images, load_styles) that needs no GPU:
the numpy statement of the rules (tests/prep_ref.py) against the reference's recorded outputs (tests/golden/prep_images.npz,
written by tools/make_prep_golden.py) and against the float resize of read_img, the properties of the fixed-point scheme, the
two symbols exported and bound, every argument rule of the C entry through the handle-less error path, and every ValueError
of the wrappers, raised before a device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, imgprep
from dhg_amd.inference import _resize_cubic, remove_whitespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "prep_images.npz"))
CASES = sorted(int(k.split("_")[1]) for k in GOLDEN.files if k.startswith("image_"))
GH, GW, GT = int(GOLDEN["H"]), int(GOLDEN["W"]), int(GOLDEN["thresh"])
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


# ---------------------------------------------------------------- the rules against the reference's recorded outputs
def test_golden_cases_are_the_ones_asked_for():
    assert len(CASES) == 8 and (GH, GW, GT) == (32, 160, 127)
    for c in CASES:
        img = GOLDEN[f"image_{c}"]
        assert img.dtype == np.uint8 and img.shape[0] <= 64 and img.shape[1] <= 256
    dark = GOLDEN["image_1"] < GT                                            # ink touching every image edge
    assert dark[0].any() and dark[-1].any() and dark[:, 0].any() and dark[:, -1].any()
    assert (GOLDEN["image_2"] < GT).any(axis=1).sum() == 2 and GOLDEN["crop_2"].shape[0] == 1   # two inked rows, a crop of one
    vals = set(np.unique(GOLDEN["image_3"]).tolist())                        # 126 is dark; 127 and 128 lie outside its box
    assert {126, 127, 128} <= vals and min(vals) == 126
    assert GOLDEN["crop_6"].shape[0] == GH                                   # the identity resize


@pytest.mark.parametrize("c", CASES)
def test_prep_ref_matches_the_reference(c):
    img, crop = GOLDEN[f"image_{c}"], GOLDEN[f"crop_{c}"]
    out, ow, box, status = prep_ref.prep_ref(img, GH, GW, GT)
    r0, r1, c0, c1 = box.tolist()
    assert status == 0 and ow == GH * crop.shape[1] // crop.shape[0]
    assert img[r0:r1, c0:c1].shape == crop.shape and np.array_equal(img[r0:r1, c0:c1], crop)   # the reference's own crop
    assert np.array_equal(crop, remove_whitespace(img, GT))
    want = GOLDEN[f"padded_{c}"]
    assert out.dtype == want.dtype == np.float32 and np.array_equal(out, want)                 # the reference's pad_img
    assert (want[:, ow:] == 255).all()


# ---------------------------------------------------------------- the fixed-point scheme
def _crops():
    """60 crops: random grey, binary and text-like, at sizes that upscale, keep and downscale."""
    g = np.random.Generator(np.random.PCG64(11))
    out = []
    for i in range(60):
        ch, cw = int(g.integers(1, 200)), int(g.integers(1, 400))
        H = (8, 32, 96)[i % 3]
        ow = H * cw // ch
        if not 1 <= ow <= 1024:
            ch, cw, ow = H + i % 5 - 2, 3 * H, H * (3 * H) // (H + i % 5 - 2)
        if i % 3 == 0:
            crop = g.integers(0, 256, (ch, cw)).astype(np.uint8)
        elif i % 3 == 1:
            crop = ((g.random((ch, cw)) < 0.5) * 255).astype(np.uint8)
        else:
            crop = np.full((ch, cw), 255, np.uint8)
            crop[g.random((ch, cw)) < 0.15] = 20
            crop[:, ::7] = np.minimum(crop[:, ::7], 90)
        out.append((crop, ow, H))
    return out


def test_fixed_point_resize_is_within_one_grey_level_of_the_float_resize():
    """The bound is derived: each of c_0..c_2 is off by at most 2^-12 and c_3 by at most 3 * 2^-12, at most 255 * 3 / 2048 =
    0.37 of error in a pass; the first pass's error is amplified by sum |w| <= 1.375 in the second: the real values are less
    than 1 apart before the rounding, and roundings of values less than 1 apart differ by at most 1."""
    worst, off, total = 0, 0, 0
    for crop, ow, H in _crops():
        d = np.abs(prep_ref.resize_fixed(crop, ow, H).astype(np.int64) - _resize_cubic(crop, ow, H).astype(np.int64))
        worst, off, total = max(worst, int(d.max())), off + int((d > 0).sum()), total + d.size
    print(f"max |fixed - float| {worst}, {off} of {total} pixels off by one")
    assert worst <= 1


def test_a_constant_crop_stays_constant():
    for v in (0, 1, 126, 200, 255):
        for ch, cw, H in ((1, 1, 8), (5, 7, 32), (97, 300, 96), (1000, 90, 96)):
            ow = max(1, H * cw // ch)
            assert (prep_ref.resize_fixed(np.full((ch, cw), v, np.uint8), ow, H) == v).all(), (v, ch, cw, H)


def test_an_identity_resize_is_an_exact_copy():
    g = np.random.Generator(np.random.PCG64(12))
    for ch, cw in ((8, 8), (32, 57), (96, 300)):
        crop = g.integers(0, 256, (ch, cw)).astype(np.uint8)
        idx, c = prep_ref.cubic_taps(cw, cw)
        assert (c == [0, 2048, 0, 0]).all() and (idx[:, 1] == np.arange(cw)).all()
        assert np.array_equal(prep_ref.resize_fixed(crop, cw, ch), crop)


def test_coefficients_sum_to_2048_and_the_sums_fit_int32():
    """sum |c| <= 2816 on each axis, over a sweep of size ratios: |sum| + 2^21 <= 255 * 2816^2 + 2^21 < 2^31; and the largest
    sum the scheme can actually produce (black where the product of coefficients is negative, white elsewhere) stays below."""
    worst = 0
    for n_in in (1, 2, 3, 5, 8, 31, 95, 96, 97, 100, 385, 1000, 4096, 16384):
        for n_out in (1, 2, 7, 8, 63, 64, 65, 96, 255, 256, 257, 512, 1400, 4096):
            idx, c = prep_ref.cubic_taps(n_in, n_out)
            assert (c.sum(axis=1) == 2048).all() and idx.min() >= 0 and idx.max() <= n_in - 1
            worst = max(worst, int(np.abs(c).sum(axis=1).max()))
    assert worst <= 2816
    assert 255 * worst * worst + (1 << 21) < 1 << 31
    g = np.random.Generator(np.random.PCG64(13))
    for ch, cw, H in ((2, 2, 8), (64, 64, 96), (3, 200, 8)):       # upscales: t = 1/2 occurs, where sum |c| peaks
        crop = ((g.random((ch, cw)) < 0.5) * 255).astype(np.uint8)
        assert np.abs(prep_ref.resize_sums(crop, H * cw // ch, H)).max() + (1 << 21) < 1 << 31


def test_prep_ref_status_bits_and_boxes():
    white = np.full((12, 20), 255, np.uint8)
    out, ow, box, st = prep_ref.prep_ref(None, 8, 16)                # a size that does not fit its slot
    assert (st, ow, box.tolist()) == (1, 0, [0, 0, 0, 0]) and (out == 255).all()
    out, ow, box, st = prep_ref.prep_ref(white, 8, 16)
    assert (st, ow, box.tolist()) == (2, 0, [0, 0, 0, 0]) and (out == 255).all()
    one_row = white.copy()
    one_row[5, 3:9] = 0                                              # ink in one row only: ch == 0, the box is still reported
    out, ow, box, st = prep_ref.prep_ref(one_row, 8, 16)
    assert (st, ow, box.tolist()) == (2, 0, [5, 5, 3, 8]) and (out == 255).all()
    wide = white.copy()
    wide[4, 0], wide[6, 19] = 0, 0                                   # 2 x 19 crop: ow = 8 * 19 // 2 = 76 > 16
    assert prep_ref.prep_ref(wide, 8, 16)[3] == 4 and prep_ref.prep_ref(wide, 8, 76)[1] == 76
    tall = np.full((40, 20), 255, np.uint8)
    tall[0, 3], tall[39, 4] = 0, 0                                   # 39 x 1 crop: ow = 8 // 39 = 0
    assert prep_ref.prep_ref(tall, 8, 16)[3] == 8
    edge = white.copy()
    edge[2, 2], edge[3, 3] = 126, 127                                # 127 is not dark at thresh 127
    assert prep_ref.prep_ref(edge, 8, 16)[3] == 2 and prep_ref.prep_ref(edge, 8, 16, thresh=128)[2].tolist() == [2, 3, 2, 3]


# ---------------------------------------------------------------- the C-ABI
def test_prep_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bsize_t\s+dhw_prep_workspace_bytes\s*\(", header) and re.search(r"\bint\s+dhw_prep\s*\(", header)
    assert "UNPINNED" in header[header.index("Writer-image preparation"):header.index("size_t dhw_prep_workspace_bytes")]
    l = _lib.lib()
    for name in ("dhw_prep_workspace_bytes", "dhw_prep"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_prep.restype is C.c_int and l.dhw_prep_workspace_bytes.restype is C.c_size_t and len(_lib.SIGNATURES["dhw_prep"][1]) == 15
    for name in ("prepare_images", "load_styles"):
        assert getattr(dhg_amd, name) is getattr(imgprep, name)


def test_prep_workspace_bytes_is_zero_outside_the_range():
    f = _lib.lib().dhw_prep_workspace_bytes
    assert [f(B) for B in (0, -1, 65536)] == [0, 0, 0]
    assert f(1) == 16 and f(65535) == 65535 * 16


def _call(**kw):
    a = dict(images=FAKE, sizes=None, B=3, Hin=40, Win=64, H=32, W=128, thresh=127, img_out=FAKE, widths_out=None, boxes_out=None,
             status_out=FAKE, workspace=FAKE, workspace_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = l.dhw_prep_workspace_bytes(a["B"])
    rc = l.dhw_prep(a["images"], a["sizes"], a["B"], a["Hin"], a["Win"], a["H"], a["W"], a["thresh"], a["img_out"], a["widths_out"],
                    a["boxes_out"], a["status_out"], a["workspace"], a["workspace_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


BAD_C = [
    (dict(B=0), "B must"), (dict(B=65536), "B must"), (dict(Hin=0), "Hin"), (dict(Hin=4097), "Hin"),
    (dict(Win=0), "Win"), (dict(Win=8), "Win"), (dict(Win=72), "Win"), (dict(Win=16400), "Win"),
    (dict(H=7), "H must"), (dict(H=513), "H must"), (dict(W=4), "W must"), (dict(W=130), "W must"), (dict(W=4100), "W must"),
    (dict(B=65535, H=512, W=68), "B H W"), (dict(thresh=0), "thresh"), (dict(thresh=256), "thresh"),
    (dict(images=None), "images is NULL"), (dict(img_out=None), "img_out is NULL"), (dict(status_out=None), "status_out is NULL"),
    (dict(workspace=None), "workspace is NULL"),
    (dict(images=FAKE + 8), "16-byte aligned"), (dict(img_out=FAKE + 4), "16-byte aligned"), (dict(workspace=FAKE + 8), "16-byte aligned"),
    (dict(sizes=FAKE + 2), "4-byte aligned"), (dict(widths_out=FAKE + 1), "4-byte aligned"), (dict(boxes_out=FAKE + 2), "4-byte aligned"),
    (dict(status_out=FAKE + 3), "4-byte aligned"), (dict(workspace_bytes=47), "workspace_bytes"), (dict(workspace_bytes=0), "workspace_bytes"),
]


@pytest.mark.parametrize("bad,name", BAD_C)
def test_each_argument_rule_of_dhw_prep_answers_without_a_gpu(bad, name):
    """No handle: every refusal is read through dhw_last_error(NULL), names its argument, and comes before any HIP call."""
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(name, msg) and msg.startswith("dhw_prep:"), (bad, msg)


def test_kernel_constants_match_the_wrapper():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "prep", "prep_host.h")).read()
    for name in ("PREP_MAX_B", "PREP_MAX_HIN", "PREP_MAX_WIN", "PREP_MIN_H", "PREP_MAX_H", "PREP_MIN_W", "PREP_MAX_W"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(imgprep, name)


# ---------------------------------------------------------------- ValueError before a device is touched
def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)


IMG = GOLDEN["image_0"]
BAD_PREPARE = [
    (dict(images=[]), "non-empty list"), (dict(images=IMG), "non-empty list"), (dict(images=[IMG.astype(np.float32)]), r"images\[0\] must be a uint8"),
    (dict(images=[IMG, IMG[0]]), r"images\[1\] must be a uint8 \[h, w\]"), (dict(images=[IMG[:0]]), "1..4096 rows"),
    (dict(images=[np.zeros((4097, 4), np.uint8)]), "1..4096 rows"), (dict(images=[np.zeros((4, 16385), np.uint8)]), "1..16384 columns"),
    (dict(height=7), r"height = 7 must lie in \[8, 512\]"), (dict(height=513), "height = 513"), (dict(height=96.0), "height = 96.0 is not an integer"),
    (dict(width=4), r"width = 4 must lie in \[8, 4096\]"), (dict(width=4100), "width = 4100"), (dict(width=1402), "width = 1402 must be a multiple of 4"),
    (dict(width=True), "width = True is not an integer"), (dict(thresh=0), r"thresh = 0 must lie in \[1, 255\]"), (dict(thresh=256), "thresh = 256"),
    (dict(thresh=127.0), "thresh = 127.0 is not an integer"), (dict(images=[IMG] * 2048, height=512, width=4096), "2\\^31"),
]


@pytest.mark.parametrize("kw,msg", BAD_PREPARE)
def test_prepare_images_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.prepare_images(kw.pop("images", [IMG]), **kw)


def test_prepare_images_reads_a_path_before_any_device_access(monkeypatch, tmp_path):
    from PIL import Image
    Image.fromarray(IMG).save(tmp_path / "a.png")
    _no_device(monkeypatch)
    with pytest.raises(AssertionError, match="device was touched"):           # valid: gets as far as the device
        dhg_amd.prepare_images([tmp_path / "a.png", str(tmp_path / "a.png"), torch.from_numpy(IMG.copy())])
    with pytest.raises(FileNotFoundError):
        dhg_amd.prepare_images([tmp_path / "missing.png"])


BAD_STYLES = [
    (dict(batch=0), "batch = 0"), (dict(batch=2.0), "batch = 2.0 is not an integer"), (dict(precision="fp16"), "precision must be"),
    (dict(width=64), r"width = 64 must lie in \[96, 4096\]"), (dict(width=1402), "multiple of 4"), (dict(sources=[]), "non-empty list"),
    (dict(sources=[IMG.astype(np.int32)]), "must be a uint8"),
]


@pytest.mark.parametrize("kw,msg", BAD_STYLES)
def test_load_styles_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    _no_device(monkeypatch)
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.load_styles(kw.pop("sources", [IMG]), **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_prepare_images_and_load_styles_fail_loudly_without_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU path"):
        dhg_amd.prepare_images([IMG])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dhg_amd.load_styles([IMG])
