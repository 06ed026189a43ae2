"""The writer-image preparation on the GPU (include/dhw.h dhw_prep, dhg_amd.prepare_images, load_styles) against the reference's
recorded outputs (tests/golden/prep_images.npz) and against the int64 statement of the rules (tests/prep_ref.py).

Every comparison is exact equality: both sides are integers (the coefficients are fixed by fp64 expressions without fused
multiply-add, everything after them is integer arithmetic) and f32 holds 0..255 exactly.  In a batch the area past each image's
(h, w) is filled with 0, which is dark: any read of it moves the crop box."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, inference

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "prep_images.npz"))
CASES = sorted(int(k.split("_")[1]) for k in GOLDEN.files if k.startswith("image_"))
GH, GW, GT = int(GOLDEN["H"]), int(GOLDEN["W"]), int(GOLDEN["thresh"])
H, W = 96, 320


def prep_raw(images, sizes, H, W, thresh=127, outputs=True):
    """dhw_prep on device tensors, on the current stream: images u8 [B,Hin,Win], sizes int32 [B,2] or None."""
    B, Hin, Win = (int(v) for v in images.shape)
    l = _lib.lib()
    img = torch.empty((B, 1, H, W), device="cuda", dtype=torch.float32)
    widths = torch.empty((B,), device="cuda", dtype=torch.int32)
    boxes = torch.empty((B, 4), device="cuda", dtype=torch.int32)
    status = torch.empty((B,), device="cuda", dtype=torch.int32)
    need = int(l.dhw_prep_workspace_bytes(B))
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    _lib.check(l.dhw_prep(images.data_ptr(), sizes.data_ptr() if sizes is not None else None, B, Hin, Win, H, W, thresh, img.data_ptr(),
                          widths.data_ptr() if outputs else None, boxes.data_ptr() if outputs else None, status.data_ptr(), ws.data_ptr(), need,
                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return img, widths, boxes, status


def batch_of(images, Hin=None, Win=None):
    """Images of different sizes in one [B,Hin,Win] array (Win a multiple of 16); what lies past an image is 0: dark."""
    Hin = max(a.shape[0] for a in images) if Hin is None else Hin
    Win = -(-max(a.shape[1] for a in images) // 16) * 16 if Win is None else Win
    host = np.zeros((len(images), Hin, Win), np.uint8)
    for b, a in enumerate(images):
        host[b, :a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(host).cuda(), torch.tensor([a.shape for a in images], dtype=torch.int32).cuda()


def run(images, H, W, thresh=127, Hin=None, Win=None, sizes=True):
    src, sz = batch_of(images, Hin, Win)
    out = prep_raw(src, sz if sizes else None, H, W, thresh)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check(got, want, label):
    (gi, gw, gb, gs), (wi, ww, wb, ws) = got, want
    assert gs.tolist() == ws.tolist(), (label, gs.tolist(), ws.tolist())
    assert gb.tolist() == wb.tolist(), (label, gb.tolist(), wb.tolist())
    assert gw.tolist() == ww.tolist(), (label, gw.tolist(), ww.tolist())
    for b in range(len(gi)):
        bad = int((gi[b] != wi[b]).sum())
        print(f"{label}[{b}]: status {gs[b]} box {gb[b].tolist()} ow {gw[b]} pixels that differ {bad}")
        assert bad == 0, (label, b, bad)


def inked(ch, cw, seed, pad=(3, 2, 4, 5), solid_edge=False):
    """An image whose crop is exactly ch x cw: random grey levels over the (ch + 1) x (cw + 1) inked area, its two corners dark,
    white margins (top, bottom, left, right).  solid_edge: the last inked row and column, which the crop drops, are black."""
    g = np.random.Generator(np.random.PCG64(seed))
    top, bottom, left, right = pad
    img = np.full((top + ch + 1 + bottom, left + cw + 1 + right), 255, np.uint8)
    img[top:top + ch + 1, left:left + cw + 1] = g.integers(0, 256, (ch + 1, cw + 1))
    img[top, left] = img[top + ch, left + cw] = 0
    if solid_edge:
        img[top + ch, left:left + cw + 1] = 0
        img[top:top + ch + 1, left + cw] = 0
    return img


def _small():
    white = np.full((10, 20), 255, np.uint8)
    one_row = white.copy()
    one_row[4, 3:11] = 5
    near = np.full((12, 40), 255, np.uint8)      # 126 is dark, the 127 beside it and the 127s further out are not
    near[2, 5], near[2, 4], near[9, 21], near[9, 20], near[0, 0], near[11, 39] = 126, 127, 127, 126, 127, 127
    imgs = [inked(1, 1, 1), inked(2, 3, 2), inked(5, 7, 3)]                                     # 0-2: every tap clamps; 1 x 1 -> ow = H
    imgs += [inked(95, 200, 4), inked(97, 200, 5), inked(385, 600, 6), inked(1000, 700, 7)]     # 3-6: up- and downscale
    imgs += [inked(96, cw, 10 + cw, pad=(0, 0, 0, 0)) for cw in (63, 64, 65, 255, 256, 257, W, W + 1)]   # 7-14: identity rows; ow = cw
    imgs += [inked(200, 2, 8), white, one_row, near, inked(40, 90, 9, solid_edge=True)]         # 15-19
    imgs += [inked(20, 1100, 20, pad=(1, 1, 1030, 3))]                                          # 20: ink past column 2048 -> bit 4
    return imgs


_cache = {}


def small_batch():
    """The mixed-size batch, its expected result and the kernel's result, computed once."""
    if not _cache:
        imgs = _small()
        _cache["imgs"], _cache["want"], _cache["got"] = imgs, prep_ref.prep_batch_ref(imgs, H, W), run(imgs, H, W)
    return _cache["imgs"], _cache["want"], _cache["got"]


# ---------------------------------------------------------------- against the reference's recorded outputs
def test_golden_images_match_the_reference():
    imgs = [GOLDEN[f"image_{c}"] for c in CASES]
    got = run(imgs, GH, GW, GT, Hin=64, Win=256)
    want_img = np.stack([GOLDEN[f"padded_{c}"] for c in CASES])[:, None]      # the reference's own pad_img outputs
    crops = [GOLDEN[f"crop_{c}"] for c in CASES]
    want_w = np.array([GH * c.shape[1] // c.shape[0] for c in crops], np.int32)
    assert got[3].tolist() == [0] * len(CASES) and got[1].tolist() == want_w.tolist()
    for b, (im, crop) in enumerate(zip(imgs, crops)):
        r0, r1, c0, c1 = got[2][b].tolist()
        assert np.array_equal(im[r0:r1, c0:c1], crop), b                       # the reference's own remove_whitespace
        assert np.array_equal(got[0][b], want_img[b]), (b, int((got[0][b] != want_img[b]).sum()))


# ---------------------------------------------------------------- against the rules, on the smallest shapes that can go wrong
def test_small_shapes_match_the_rules():
    imgs, want, got = small_batch()
    st, ww = want[3].tolist(), want[1].tolist()
    assert ww[:3] == [H, 144, 134] and ww[3:7] == [202, 197, 149, 67]          # 1 x 1 -> ow = H; 95, 97, 385 and 1000 rows
    assert ww[7:15] == [63, 64, 65, 255, 256, 257, W, 0] and st[7:15] == [0] * 7 + [4]
    assert st[15:18] == [8, 2, 2] and st[18:] == [0, 0, 4] and sum(st[:7]) == 0
    assert want[2][17].tolist() == [4, 4, 3, 10] and want[2][18].tolist() == [2, 9, 5, 20]   # one inked row; the 126s alone
    assert want[2][20].tolist() == [1, 21, 1030, 2130]
    check(got, want, "small")


def test_sizes_that_do_not_fit_set_bit_1_and_leave_the_neighbours_alone():
    imgs = [inked(30, 50, 41), inked(20, 70, 42), inked(25, 60, 43), inked(10, 30, 44)]
    src, sz = batch_of(imgs)
    Hin, Win = int(src.shape[1]), int(src.shape[2])
    src[0], src[2] = 0, 0                                                      # all dark: reading it would show
    sz[0] = torch.tensor([0, 40], dtype=torch.int32)
    sz[2] = torch.tensor([Hin + 1, 40], dtype=torch.int32)
    got = tuple(t.cpu().numpy() for t in prep_raw(src, sz, 32, 128))
    want = prep_ref.prep_batch_ref([None, imgs[1], None, imgs[3]], 32, 128)
    assert want[3].tolist() == [1, 0, 1, 0] and want[1][1] > 0
    check(got, want, "bad sizes")
    sz[0] = torch.tensor([10, Win + 1], dtype=torch.int32)
    sz[2] = torch.tensor([-3, 5], dtype=torch.int32)
    check(tuple(t.cpu().numpy() for t in prep_raw(src, sz, 32, 128)), want, "bad widths")


def test_whole_slots_without_sizes_at_a_height_that_is_no_multiple_of_the_band():
    imgs = [inked(33, 50, 51, pad=(2, 4, 5, 8)), inked(30, 47, 52, pad=(7, 2, 3, 13))]    # both 40 x 64: Hin x Win
    assert [a.shape for a in imgs] == [(40, 64)] * 2
    for Hout in (40, 8):
        want = prep_ref.prep_batch_ref(imgs, Hout, 64)
        assert want[3].tolist() == [0, 0]
        check(run(imgs, Hout, 64, sizes=False), want, f"sizes=NULL/H={Hout}")
    src, _ = batch_of(imgs)
    img, _, _, status = prep_raw(src, None, 40, 64, outputs=False)              # widths_out and boxes_out are optional
    assert status.tolist() == [0, 0] and np.array_equal(img.cpu().numpy(), prep_ref.prep_batch_ref(imgs, 40, 64)[0])


def test_threshold_other_than_127():
    imgs = [_small()[18], inked(12, 30, 61)]
    for thresh in (1, 128, 255):
        check(run(imgs, 16, 64, thresh), prep_ref.prep_batch_ref(imgs, 16, 64, thresh), f"thresh={thresh}")


# ---------------------------------------------------------------- batch independence and determinism
def test_a_row_of_a_batch_equals_the_image_alone_bit_for_bit():
    imgs, want, first = small_batch()
    again = run(imgs, H, W)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    assert imgs[7].shape == (97, 64)
    for b in (0, 3, 6, 7, 13, 15, 16, 19):        # alone: Hin = h and Win = w rounded up to 16 (sizes = NULL where that is w), a wider W
        alone = run([imgs[b]], H, 512, sizes=imgs[b].shape[1] % 16 != 0)
        assert alone[3].tolist() == first[3][b:b + 1].tolist() and alone[1].tolist() == first[1][b:b + 1].tolist(), b
        assert alone[2].tolist() == first[2][b:b + 1].tolist(), b
        assert np.array_equal(alone[0][0, 0, :, :W], first[0][b, 0]) and (alone[0][0, 0, :, W:] == 255).all(), b


# ---------------------------------------------------------------- graph capture
def test_prep_in_a_graph_replays_identically():
    imgs = [GOLDEN[f"image_{c}"] for c in (0, 2, 5)] + [np.full((9, 9), 255, np.uint8)]
    src, sz = batch_of(imgs)
    eager = prep_raw(src, sz, GH, GW)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = prep_raw(src, sz, GH, GW)
    shots = []
    for _ in range(2):
        out[0].fill_(7.0)
        for t in out[1:]:
            t.fill_(-9)
        g.replay()
        torch.cuda.synchronize()
        shots.append(tuple(t.clone() for t in out))
    for x, y, e in zip(shots[0], shots[1], eager):
        assert torch.equal(x, y) and torch.equal(x, e)
    assert shots[0][3].tolist() == [0, 0, 0, 2]
    check(tuple(t.cpu().numpy() for t in shots[0]), prep_ref.prep_batch_ref(imgs, GH, GW), "graph")


# ---------------------------------------------------------------- the wrappers
def test_prepare_images_from_arrays_and_png_files(tmp_path):
    from PIL import Image
    imgs = [GOLDEN[f"image_{c}"] for c in CASES]
    want = prep_ref.prep_batch_ref(imgs, GH, GW)
    items = []
    for i, a in enumerate(imgs):
        if i % 3 == 0:
            Image.fromarray(a).save(tmp_path / f"w{i}.png")
            items.append(tmp_path / f"w{i}.png" if i else str(tmp_path / f"w{i}.png"))
        else:
            items.append(torch.from_numpy(a.copy()) if i % 3 == 1 else a)
    got = dhg_amd.prepare_images(items, height=GH, width=GW)
    assert got[0].shape == (len(imgs), 1, GH, GW) and all(t.is_cuda for t in got) and got[0].dtype == torch.float32
    assert all(t.dtype == torch.int32 for t in got[1:])
    check(tuple(t.cpu().numpy() for t in got), want, "wrapper")
    # the defaults: 96 rows, 1400 columns, thresh 127
    got = dhg_amd.prepare_images(imgs[:2])
    check(tuple(t.cpu().numpy() for t in got), prep_ref.prep_batch_ref(imgs[:2], 96, 1400), "wrapper defaults")


def test_load_styles_equals_the_extractor_on_the_reference_batch():
    imgs = [GOLDEN[f"image_{c}"] for c in (0, 3, 4, 6)] + [np.full((9, 9), 255, np.uint8)]
    want = prep_ref.prep_batch_ref(imgs, 96, 512)
    assert want[3].tolist() == [0, 0, 0, 0, 2] and want[1].tolist() == [462, 298, 320, 300, 0]
    with pytest.warns(UserWarning, match="random initialisation"):
        inference._extractors.pop("None", None)
        sv, widths, status = dhg_amd.load_styles(imgs, width=512, batch=3)
    assert sv.shape == (5, 14, 1280) and sv.dtype == torch.float32 and sv.is_cuda
    assert widths.tolist() == want[1].tolist() and status.tolist() == want[3].tolist()
    ex = inference._extractors["None"]                                          # the cached extractor, on the rules' batch
    ref = torch.cat([ex(torch.from_numpy(want[0][i:i + 3])) for i in (0, 3)])
    assert torch.equal(sv, ref)
    assert torch.isfinite(sv).all() and not torch.equal(sv[0], sv[1])
