"""The stroke rasteriser on the GPU (include/dhw.h dhw_render, dhg_amd.render_strokes) against a float64 brute-force numpy
reference whose drawn set comes from vis.strokes_to_polylines (pinned to the reference's show_strokes by golden/vis.npz).

Inputs: offsets are multiples of 1/16 (dx = round(N(0.6,1) 16)/16, dy = round(N(0,1) 16)/16) and pen values come from
{0.02, 0.3, 0.5, 0.7, 0.98}, so every fp32 prefix sum and the box are exact in any summation order.  What is left of the
fp32 error is a handful of roundings on pixel coordinates below 512, each at most 3e-5 px: about 0.07 grey levels in the
worst case.  The image tolerance is max abs diff <= 0.5 grey levels (~7x that bound); widths agree within +-1."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import spec, vis

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from page_ref import make_strokes  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 0.5


def ref_render(strokes, n, H, W, lw=2.0):
    """float64, brute force: min over all drawn segments for every pixel.  -> (image [H,W], width, number of segments, voff)"""
    s = np.asarray(strokes, np.float64)[:n]
    segs = []
    for line in vis.strokes_to_polylines(s):
        for k in range(1, len(line)):
            segs.append((line[k - 1], line[k]))
    if not segs:
        return np.full((H, W), 255.0), 0, 0, 0.0
    P = np.array(segs)                                   # [S, 2 endpoints, 2 coordinates]
    xmin, xmax = P[..., 0].min(), P[..., 0].max()
    ymin, ymax = P[..., 1].min(), P[..., 1].max()
    m = lw / 2 + 1
    ex, ey = xmax - xmin, ymax - ymin
    if ey > 0:
        sc = (H - 2 * m) / ey
        if ex * sc > W - 2 * m:
            sc = (W - 2 * m) / ex
    elif ex > 0:
        sc = min((W - 2 * m) / ex, H - 2 * m)
    else:
        sc = 1.0
    voff = (H - 2 * m - ey * sc) / 2
    A = np.stack([m + (P[:, 0, 0] - xmin) * sc, m + voff + (ymax - P[:, 0, 1]) * sc], -1)
    Bp = np.stack([m + (P[:, 1, 0] - xmin) * sc, m + voff + (ymax - P[:, 1, 1]) * sc], -1)
    cy, cx = (v.reshape(-1, 1) for v in np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij"))   # [H W, 1]
    d2 = np.full(H * W, np.inf)
    for k in range(0, len(A), 64):
        ax, ay = A[k:k + 64, 0], A[k:k + 64, 1]
        abx, aby = Bp[k:k + 64, 0] - ax, Bp[k:k + 64, 1] - ay
        l2 = abx * abx + aby * aby
        rx, ry = cx - ax, cy - ay                        # [H W, 64]
        t = np.clip((rx * abx + ry * aby) / np.where(l2 > 0, l2, 1.0), 0, 1) * (l2 > 0)   # a zero-length segment is a point
        rx -= t * abx
        ry -= t * aby
        d2 = np.minimum(d2, (rx * rx + ry * ry).min(-1))
    d = np.sqrt(d2).reshape(H, W)
    img = 255.0 * (1 - np.clip(lw / 2 + 0.5 - d, 0, 1))
    return img, min(W, int(np.ceil(ex * sc + 2 * m))), len(A), voff


def check_against_ref(strokes, lens, images, widths, H, W, lw=2.0, label=""):
    images, widths = images.cpu().numpy(), widths.cpu().numpy()
    assert images.shape == (len(strokes), 1, H, W) and images.dtype == np.float32
    out = []
    for b in range(len(strokes)):
        ref, wref, nseg, voff = ref_render(strokes[b], lens[b] if lens is not None else strokes.shape[1], H, W, lw)
        err = float(np.abs(images[b, 0] - ref).max())
        print(f"{label} row {b}: {nseg} segments, width {widths[b]} (ref {wref}), max abs diff {err:.4f} grey levels")
        assert np.isfinite(images[b]).all()
        assert err <= TOL, (b, err)
        assert abs(int(widths[b]) - wref) <= 1, (b, widths[b], wref)
        out.append((ref, wref, nseg, voff))
    return out


def test_basic_matches_the_reference_and_is_deterministic():
    B, L, H, W = 3, 40, 32, 128
    st = make_strokes(np.random.default_rng(1), B, L)
    st[0, :, 2] = 0.3
    st[0, [0, 10, 11, 39], 2] = [0.98, 0.7, 0.98, 0.7]      # a lift at row 0, two consecutive lifts, a lift on the last row
    st[1, L - 1, 2] = 0.98
    st[2, 30, 2] = 0.7
    img, wd = dhg_amd.render_strokes(st, height=H, width=W)
    assert img.is_cuda and wd.is_cuda and wd.dtype == torch.int32
    refs = check_against_ref(st, None, img, wd, H, W, label="basic")
    assert all(r[2] > 0 for r in refs) and img.min().item() < 64       # ink was drawn, and dark
    img2, wd2 = dhg_amd.render_strokes(torch.from_numpy(st).cuda(), height=H, width=W)
    assert torch.equal(img, img2) and torch.equal(wd, wd2)             # two calls: bit-identical


def test_ragged_rows_equal_the_prompt_rendered_alone():
    B, L, H, W = 4, 64, 32, 256
    lens = [8, 64, 24, 40]
    st = make_strokes(np.random.default_rng(2), B, L)
    for b, n in enumerate(lens):
        st[b, n - 1, 2] = 0.98
        st[b, n:] = np.nan                                             # rows past each length are never read
    img, wd = dhg_amd.render_strokes(st, lens, height=H, width=W)
    assert not torch.isnan(img).any()
    check_against_ref(st, lens, img, wd, H, W, label="ragged")
    for b, n in enumerate(lens):
        alone, walone = dhg_amd.render_strokes(st[b:b + 1, :n].copy(), height=H, width=W)
        assert torch.equal(alone[0], img[b]) and int(walone[0]) == int(wd[b]), b
    img_t, wd_t = dhg_amd.render_strokes(st, torch.tensor(lens, device="cuda"), height=H, width=W)   # lengths as a device tensor
    assert torch.equal(img_t, img) and torch.equal(wd_t, wd)


def test_degenerate_rows_in_one_batch():
    L, H, W, m = 24, 32, 64, 2.0
    st = np.zeros((5, L, 3), np.float32)
    st[..., 2] = 0.3
    rnd = make_strokes(np.random.default_rng(3), 5, L, lift_p=0.0)
    st[0, :, :2] = rnd[0, :, :2]                                       # 0: no lift at all
    st[1, [5, 20], 2] = [0.7, 0.98]                                    # 1: all offsets zero, with lifts: one dot
    st[2, :, 0] = np.abs(rnd[2, :, 0]) + 0.25                          # 2: dy == 0: a horizontal line
    st[2, L - 1, 2] = 0.98
    st[3, :, :2] = rnd[3, :, :2]                                       # 3: exactly one drawn segment (i = 1)
    st[3, 2, 2] = 0.98
    st[4, :, 0] = 2.5                                                  # 4: 40x wider than tall
    st[4, :, 1] = np.where(np.arange(L) % 2 == 0, 1.375, -1.375)
    st[4, L - 1, 2] = 0.98
    img, wd = dhg_amd.render_strokes(st, height=H, width=W)
    refs = check_against_ref(st, None, img, wd, H, W, label="degenerate")
    im, wd = img.cpu().numpy()[:, 0], wd.cpu().numpy()
    assert (im[0] == 255).all() and wd[0] == 0 and refs[0][2] == 0
    ys, xs = np.nonzero(im[1] < 255)                                   # the dot: centred on (m, H/2), radius line_width/2 + 0.5
    assert refs[1][2] > 0 and wd[1] == 4 and len(ys) > 0
    assert xs.max() < 4 and abs((ys.min() + ys.max() + 1) / 2 - H / 2) < 1e-6 and im[1].min() < 128
    ys, xs = np.nonzero(im[2] < 255)                                   # the horizontal line: centred vertically, full ink width
    assert abs((ys.min() + ys.max() + 1) / 2 - H / 2) < 1e-6 and ys.max() - ys.min() + 1 <= 4 and xs.max() >= wd[2] - 4
    assert refs[3][2] == 1
    ex, ey = 2.5 * 22, 1.375
    assert refs[4][3] > 0 and abs(refs[4][3] - (H - 2 * m - ey * (W - 2 * m) / ex) / 2) < 1e-9 and wd[4] == W   # width-limited scale
    ys, _ = np.nonzero(im[4] < 255)
    assert ys.min() > 8 and ys.max() < H - 8                          # ... and the ink sits in the middle rows


_stress = {}
STRESS_LENS = [1000, 1000, 1040]


def _stress_batch():
    """Row 0: a zig-zag whose ~1000 drawn segments all fall inside about 24 columns — several LDS chunks for one tile, the
    running minimum must survive the chunk boundaries.  Row 1: a left-to-right line with two segments that run across half
    the picture (several tile borders each).  Row 2: 1040 strokes, so thread 64 — the first of the second wave — takes part
    in the scan: its positions start from the first wave's sum, the last lift sits in it, and segments are drawn on both
    sides of stroke 1024.  Rendered once, shared by the three cases."""
    if not _stress:
        L, L2, H, W = 1000, 1040, 96, 512
        st = np.full((3, L2, 3), np.nan, np.float32)                   # rows past each length are never read
        st[:2, :L] = make_strokes(np.random.default_rng(4), 2, L, lift_p=0.03)
        st[2] = make_strokes(np.random.default_rng(41), 1, L2, lift_p=0.03)[0]
        st[2, 1016:1036, 2] = 0.3                                      # pen down across the wave boundary ...
        st[2, [1036, L2 - 1], 2] = [0.7, 0.98]                         # ... then a lift, and one on the last stroke
        i = np.arange(L)
        st[0, :L, 0] = np.where(i % 2 == 0, 5.0, -5.0)
        st[0, :L, 1] = np.where((i // 100) % 2 == 0, 0.25, -0.25)
        st[0, :L, 2] = 0.3
        st[0, [500, L - 1], 2] = [0.7, 0.98]
        st[1, L - 1, 2] = 0.98
        st[1, 498:503, 2] = 0.3
        back = float(st[1, :500, 0].astype(np.float64).sum())          # a multiple of 1/16: exact
        assert back > 100
        st[1, 500, :2] = [-back, 0.0]                                  # pen down, back to the start of the line ...
        st[1, 501, :2] = [back, 0.0]                                   # ... and forth again
        _stress["v"] = (st, *dhg_amd.render_strokes(st, STRESS_LENS, height=H, width=W), H, W)
    return _stress["v"]


@pytest.mark.parametrize("row", [0, 1, 2])
def test_cull_and_chunk_stress(row):
    st, img, wd, H, W = _stress_batch()
    (_, wref, nseg, _), = check_against_ref(st[row:row + 1], STRESS_LENS[row:row + 1], img[row:row + 1], wd[row:row + 1], H, W,
                                            label=f"stress[{row}]")
    if row == 0:
        assert nseg > 3 * vis.RENDER_CHUNK and wref <= 28              # more than any one chunk holds, all in one tile
    elif row == 1:
        assert wref == W and nseg > 900                                # row 1 spans every tile
    else:
        lifts = np.round(st[2, :, 2]) != 0
        assert not lifts[1016:1036].any() and lifts[1036] and lifts[1039] and nseg > 900   # segments 1016..1035 are drawn
        alone, walone = dhg_amd.render_strokes(st[2:3].copy(), height=H, width=W)          # the line alone at L = 1040
        assert torch.equal(alone[0], img[2]) and int(walone[0]) == int(wd[2])


def test_graph_capture_on_a_side_stream_replays_bit_identically():
    B, L, H, W = 2, 48, 32, 128
    rng = np.random.default_rng(5)
    batches = [torch.from_numpy(make_strokes(rng, B, L)).cuda() for _ in range(3)]
    for t in batches:
        t[:, L - 1, 2] = 0.98
    static = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dhg_amd.render_strokes(static, height=H, width=W)              # warm-up: the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        img, wd = dhg_amd.render_strokes(static, height=H, width=W)
    for t in batches[1:]:
        static.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        got_img, got_wd = img.clone(), wd.clone()
        eager_img, eager_wd = dhg_amd.render_strokes(t, height=H, width=W)
        torch.cuda.synchronize()
        assert torch.equal(got_img, eager_img) and torch.equal(got_wd, eager_wd)
        assert got_img.min().item() < 255


def test_images_feed_the_style_extractor_directly():
    B, L, H, W = 2, 64, 96, 192
    st = make_strokes(np.random.default_rng(6), B, L)
    st[:, L - 1, 2] = 0.98
    images, _ = dhg_amd.render_strokes(st, height=H, width=W)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ext = dhg_amd.StyleExtractor(None, precision="fp32")
    a = ext(images)
    b = ext(images.cpu().numpy())
    assert tuple(a.shape) == (B, 14, 1280) and torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_infer_file_batch_gpu_renderer(tmp_path, monkeypatch):
    """The pattern of test_infer_file_end_to_end with renderer="gpu": two prompts, one ragged sampler call, one render call."""
    from PIL import Image
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}
    (tmp_path / "config.yml").write_text("training_args:\n  att_layers_num: 2\n  channels: 128\n  dropout: 0.0\n")
    torch.save({"state_dict": sd}, tmp_path / "checkpoint_2000.pth")
    np.save(tmp_path / "style.npy", spec.synthetic_inputs(1, 8, 1, seed=9)["style"][0])
    monkeypatch.chdir(tmp_path)
    strokes = dhg_amd.infer_file_batch(["Hi there", "Rabbit"], str(tmp_path / "style.npy"), experiment_path=str(tmp_path),
                                       output="page", seed=3, renderer="gpu")
    assert [s.shape[0] for s in strokes] == [dhg_amd.stroke_length(len(dhg_amd.Tokenizer().encode(p))) for p in ("Hi there", "Rabbit")]
    (tmp_path / "direct").mkdir()
    for i, s in enumerate(strokes):
        got = np.asarray(Image.open(tmp_path / f"page_{i}.png"))
        assert got.ndim == 2 and got.shape[0] == 96 and got.dtype == np.uint8
        img, wd = dhg_amd.render_strokes(s[None])
        vis.save_line_png(img[0], int(wd[0]), f"direct/line_{i}")
        assert np.array_equal(got, np.asarray(Image.open(tmp_path / "direct" / f"line_{i}.png")))
