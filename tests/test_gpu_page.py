"""The page compositor on the GPU (include/dhw.h dhw_page, dhg_amd.render_page / write_page) against tests/page_ref.py, the
float64 brute-force statement of the rules whose drawn set comes from vis.strokes_to_polylines.

Inputs (page_ref.make_strokes, as tests/test_gpu_render.py): offsets are multiples of 1/16, pen values come from
{0.02, 0.3, 0.5, 0.7, 0.98}; margins and pitch are multiples of 1/16.  Every fp32 prefix sum, box and extent is therefore
exact in any summation order, the two fp32 divisions behind the scale are the reference's, and the shared scale is compared
bit for bit.  Every page is below 512 px on a side, so what is left of the fp32 error is the derivation of
tests/test_gpu_render.py: a handful of roundings on pixel coordinates below 512, each at most 3e-5 px, about 0.07 grey levels
in the worst case.  Image bound: max abs diff <= 0.5 grey levels (that test's figure, for the same arithmetic).  Box bound:
2.5e-4 px (each box value is four fp32 operations below 512 at half an ulp, 3e-5, each, doubled)."""
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 0.5
BOX_TOL = 2.5e-4


def bits(x):
    return np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x, np.float32).view(np.uint32)


def check_against_ref(st, lens, slots, geo, scale=None, label="", got=None):
    """Render (unless `got` = (pages, scale, boxes) is given), print every figure, then assert the three bounds."""
    pages, sc, boxes = got if got is not None else dhg_amd.render_page(st, lens, slots, scale=scale, **geo)
    ref, s_ref, boxes_ref, counts = page_ref.page_ref(st, lens, slots, scale=scale, **geo)
    assert pages.is_cuda and tuple(pages.shape) == (geo["pages"], 1, geo["height"], geo["width"]) and pages.dtype == torch.float32
    assert tuple(sc.shape) == (1,) and tuple(boxes.shape) == (len(st), 4)
    im, bx = pages.cpu().numpy()[:, 0], boxes.cpu().numpy()
    err = [float(np.abs(im[p] - ref[p]).max()) for p in range(geo["pages"])]
    berr = float(np.abs(bx - boxes_ref).max())
    print(f"{label}: segments {counts}, scale {float(sc[0]):.9g} (ref {float(s_ref):.9g}), max abs diff per page "
          f"{[round(e, 4) for e in err]} grey levels, max box diff {berr:.3e} px")
    assert np.isfinite(im).all()
    assert np.array_equal(bits(sc), bits([s_ref])), (float(sc[0]), float(s_ref))
    assert max(err) <= TOL, err
    assert berr <= BOX_TOL, berr
    return im, ref, boxes_ref, counts


# ---------------------------------------------------------------- 1-3: the basic batch
BASIC_GEO = dict(pages=2, height=160, width=256, lines_per_page=3, margin_left=6.0, margin_top=4.0, pitch=48.0)
BASIC_LENS = [40, 17, 33, 8, 40]
_basic = {}


def _basic_batch():
    """N = 5, L = 40, two pages of three slots; rendered once at the automatic scale, shared by the cases below."""
    if not _basic:
        st = page_ref.make_strokes(np.random.default_rng(11), 5, 40)
        for b, n in enumerate(BASIC_LENS):
            st[b, n - 1, 2] = 0.98
            st[b, n:] = np.nan                                             # rows past each length are never read
        _basic["v"] = (st, dhg_amd.render_page(st, BASIC_LENS, **BASIC_GEO))
    return _basic["v"]


def test_basic_matches_the_reference_and_is_deterministic():
    st, got = _basic_batch()
    im, ref, boxes_ref, counts = check_against_ref(st, BASIC_LENS, None, BASIC_GEO, label="basic", got=got)
    assert all(c > 0 for c in counts) and im[0].min() < 64 and im[1].min() < 64              # ink on both pages, and dark
    again = dhg_amd.render_page(torch.from_numpy(st).cuda(), torch.tensor(BASIC_LENS, device="cuda"), **BASIC_GEO)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                                # two calls (lengths on the device): identical bits
    # at the automatic scale every line stays inside its slot and the writing area, up to the rounding of the scale: s is
    # an fp32 quotient, at most (1 + 2^-24) times the exact pitch / ey_n and (W - 2 margin_left) / ex_n, so an extent times s
    # may pass its limit by that factor (3e-6 px at pitch 48); 2^-23 leaves room for the float64 products of the reference
    up = 1 + 2.0 ** -23
    avail = BASIC_GEO["width"] - 2 * BASIC_GEO["margin_left"]
    assert (boxes_ref[:, 2] - boxes_ref[:, 0] <= avail * up).all() and (boxes_ref[:, 0] == BASIC_GEO["margin_left"]).all()
    assert (boxes_ref[:, 3] - boxes_ref[:, 1] <= BASIC_GEO["pitch"] * up).all()
    assert (boxes_ref[:, 3] - boxes_ref[:, 1]).max() > BASIC_GEO["pitch"] * (1 - 2.0 ** -23)   # and the tightest line fills its slot


def test_explicit_scale():
    st, _ = _basic_batch()
    pages, sc, _ = got = dhg_amd.render_page(st, BASIC_LENS, scale=0.5, **BASIC_GEO)
    check_against_ref(st, BASIC_LENS, None, BASIC_GEO, scale=0.5, label="scale 0.5", got=got)
    assert float(sc[0]) == 0.5 and pages.min().item() < 255


def test_page_is_the_min_of_its_lines_alone_and_independent_of_line_order():
    st, (pages, sc, boxes) = _basic_batch()
    s = float(sc[0])
    want = torch.full_like(pages, 255.0)
    for n, ln in enumerate(BASIC_LENS):
        alone, sc1, box1 = dhg_amd.render_page(st[n:n + 1, :ln].copy(), None, [n], scale=s, **BASIC_GEO)   # the same slot, the batch's scale
        assert float(sc1[0]) == s and torch.equal(box1[0], boxes[n])
        want = torch.minimum(want, alone)
    assert torch.equal(want, pages)                                                          # bit for bit
    order = [3, 0, 4, 2, 1]
    pages2, sc2, boxes2 = dhg_amd.render_page(st[order], [BASIC_LENS[i] for i in order], order, **BASIC_GEO)
    assert torch.equal(pages2, pages) and torch.equal(sc2, sc) and torch.equal(boxes2, boxes[order])


# ---------------------------------------------------------------- 4: overlap and clipping
def test_overlap_and_clipping():
    geo = dict(pages=1, height=96, width=128, lines_per_page=3, margin_left=0.0, margin_top=4.0, pitch=24.0)
    st = page_ref.make_strokes(np.random.default_rng(12), 4, 40)
    st[:, 39, 2] = 0.98
    slots = [0, 0, 1, 2]                                                                     # two lines share slot 0
    im, ref, boxes_ref, counts = check_against_ref(st, None, slots, geo, scale=12.0, label="overlap")
    r = 2.0 / 2 + 0.5
    assert all(c > 0 for c in counts)
    assert boxes_ref[:, 1].min() + r < 0 and boxes_ref[:, 3].max() - r > geo["height"]       # ink beyond the top and the bottom edge,
    assert boxes_ref[:, 2].max() - r > geo["width"] and boxes_ref[:, 0].min() - r < 0        # the right and (by the pen's radius) the left one
    assert (boxes_ref[:, 3] - boxes_ref[:, 1] > 2 * geo["pitch"]).all()                      # and every line reaches into its neighbours' slots
    assert im.min() < 64


# ---------------------------------------------------------------- 5: degenerate lines
def test_degenerate_lines_in_one_batch():
    geo = dict(pages=1, height=128, width=128, lines_per_page=4, margin_left=5.0, margin_top=3.0, pitch=30.0)
    L = 24
    rnd = page_ref.make_strokes(np.random.default_rng(13), 5, L, lift_p=0.0)
    st = np.zeros((5, L, 3), np.float32)
    st[..., 2] = 0.3
    st[0, :, :2] = rnd[0, :, :2]                                       # 0: no lift at all: draws nothing
    st[1, [5, 20], 2] = [0.7, 0.98]                                    # 1: all offsets zero, with lifts: one dot
    st[2, :, 0] = np.abs(rnd[2, :, 0]) + 0.25                          # 2: dy == 0: a zero-height line
    st[2, L - 1, 2] = 0.98
    st[3, :, :2] = rnd[3, :, :2]                                       # 3: an ordinary line in a slot off the page
    st[3, L - 1, 2] = 0.98
    st[4, :, :2] = rnd[4, :, :2]                                       # 4: an ordinary line
    st[4, L - 1, 2] = 0.98
    slots = [0, 1, 2, 4, 3]
    im, ref, boxes_ref, counts = check_against_ref(st, None, slots, geo, label="degenerate")
    assert counts[0] == 0 and counts[3] == 0 and counts[1] > 0 and counts[2] > 0 and counts[4] > 0
    assert not boxes_ref[0].any() and not boxes_ref[3].any()
    # (slot k covers rows 3 + 30 k .. 33 + 30 k; its two border rows may hold the pen's radius of a neighbour: left out)
    ys, xs = np.nonzero(im[0][35:61] < 255)                            # the dot: at the left margin, in the middle of slot 1
    assert len(ys) > 0 and xs.max() < 8 and abs((ys.min() + ys.max() + 1) / 2 - 13) < 1e-6
    ys, xs = np.nonzero(im[0][65:91] < 255)                            # the zero-height line: centred in slot 2
    assert abs((ys.min() + ys.max() + 1) / 2 - 13) < 1e-6 and ys.max() - ys.min() + 1 <= 4 and xs.max() > 32
    assert (im[0][:32] == 255).all()                                   # slot 0 (the line without a lift) stays white
    # a batch in which nothing draws: white, scale 1
    pages, sc, boxes = dhg_amd.render_page(st[[0, 3]], None, [0, 4], **geo)
    assert (pages == 255).all().item() and float(sc[0]) == 1.0 and not boxes.any().item()


# ---------------------------------------------------------------- 6: shapes off the tile grid
def test_shapes_off_the_tile_grid():
    geo = dict(pages=2, height=200, width=260, lines_per_page=4, margin_left=1.5, margin_top=9.5, pitch=47.5)   # three bands; 260 = 8 tiles + 4 columns
    st = page_ref.make_strokes(np.random.default_rng(14), 7, 56)
    st[0, :, 0] = np.abs(st[0, :, 0]) + 0.5                            # line 0 is long and flat: its width sets the scale,
    st[0, :, 1] *= 0.25                                                # so its ink ends in the last, partial tile
    lens = [56, 31, 56, 9, 48, 56, 40]
    for b, n in enumerate(lens):
        st[b, n - 1, 2] = 0.98
    im, ref, boxes_ref, counts = check_against_ref(st, lens, [0, 1, 3, 2, 4, 5, 7], geo, label="off grid")
    assert all(c > 0 for c in counts) and boxes_ref[0, 2] == pytest.approx(260 - 1.5, abs=1e-3)
    assert ref[:, :, 256:].min() < 255 and ref[:, 192:].min() < 255    # (the inputs put ink into the last partial tile and into the last band)


# ---------------------------------------------------------------- 7: cull and chunk stress
def test_cull_and_chunk_stress():
    geo = dict(pages=1, height=96, width=128, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=44.0)
    L, L2 = 1024, 1040
    st = np.full((3, L2, 3), np.nan, np.float32)                       # rows past each length are never read
    st[:2, :L] = page_ref.make_strokes(np.random.default_rng(15), 2, L, lift_p=0.03)
    i = np.arange(L)
    st[0, :L, 0] = np.where(i % 2 == 0, 5.0, -5.0)                      # a zig-zag: ~1000 segments inside a dozen columns
    st[0, :L, 1] = np.where((i // 100) % 2 == 0, 0.25, -0.25)
    st[0, :L, 2] = 0.3
    st[0, [500, L - 1], 2] = [0.7, 0.98]
    st[1, 59, 2] = 0.98
    # line 2: 1040 strokes, so thread 64 — the first of the second wave — takes part in the scan: its positions start from the
    # first wave's sum, the last lift sits in it, and segments are drawn on both sides of stroke 1024.  (The generator's
    # offsets less the mean of dx and divided by 4: on the 1/64 grid with sums below 2^11, still exact in fp32, and small
    # enough that line 0 keeps setting the scale.)
    st[2] = page_ref.make_strokes(np.random.default_rng(151), 1, L2, lift_p=0.03)[0]
    st[2, :, :2] = (st[2, :, :2] - np.float32([0.625, 0.0])) / 4
    st[2, 1016:1036, 2] = 0.3                                          # pen down across the wave boundary ...
    st[2, [1036, L2 - 1], 2] = [0.7, 0.98]                             # ... then a lift, and one on the last stroke
    lens, slots = [L, 60, L2], [0, 1, 1]
    pages, sc, boxes = got = dhg_amd.render_page(st, lens, slots, **geo)
    im, ref, boxes_ref, counts = check_against_ref(st, lens, slots, geo, label="stress", got=got)
    assert counts[0] > 3 * 256 and counts[1] > 0                       # more than any one LDS chunk holds ...
    assert boxes_ref[0, 2] + 1.5 < 32                                  # ... all of it in the first 32-column tile
    lifts = np.round(st[2, :, 2]) != 0
    assert not lifts[1016:1036].any() and lifts[1036] and lifts[1039] and counts[2] > 900   # segments 1016..1035 are drawn
    alone, sc1, box1 = dhg_amd.render_page(st[2:3].copy(), None, [1], scale=float(sc[0]), **geo)   # the line alone at L = 1040
    others, _, _ = dhg_amd.render_page(st[:2, :L].copy(), lens[:2], slots[:2], scale=float(sc[0]), **geo)
    assert torch.equal(box1[0], boxes[2]) and torch.equal(torch.minimum(alone, others), pages)


def test_second_header_round_is_the_min_of_its_lines_alone():
    """260 lines on one page: the raster kernel takes the headers 256 at a time, so lines 256..259 come in a second round."""
    geo = dict(pages=1, height=96, width=128, lines_per_page=4, margin_left=4.0, margin_top=4.0, pitch=22.0)
    N, L, s = 260, 8, 4.0
    st = page_ref.make_strokes(np.random.default_rng(17), N, L, lift_p=0.0)
    st[:, L - 1, 2] = 0.98
    st[257, :, 0] = 3.0                                                # one line of the second round reaches past all others
    slots = [n % 4 for n in range(N)]
    pages, sc, boxes = got = dhg_amd.render_page(st, None, slots, scale=s, **geo)
    im, ref, boxes_ref, counts = check_against_ref(st, None, slots, geo, scale=s, label="260 lines", got=got)
    assert all(c == L - 2 for c in counts) and boxes_ref[257, 2] > boxes_ref[:256, 2].max() + 4
    want = torch.full_like(pages, 255.0)
    for n in range(N):
        if n == 256:
            assert not torch.equal(want, pages)                        # the first round alone is not the page
        alone, _, box1 = dhg_amd.render_page(st[n:n + 1], None, [slots[n]], scale=s, **geo)
        assert torch.equal(box1[0], boxes[n])
        want = torch.minimum(want, alone)
    assert torch.equal(want, pages)                                    # bit for bit


# ---------------------------------------------------------------- 8: graph capture
def test_graph_capture_on_a_side_stream_replays_bit_identically():
    geo = dict(pages=1, height=96, width=128, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=44.0)
    rng = np.random.default_rng(16)
    batches = [torch.from_numpy(page_ref.make_strokes(rng, 3, 48)).cuda() for _ in range(3)]
    for t in batches:
        t[:, 47, 2] = 0.98
    slots = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    static = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dhg_amd.render_page(static, None, slots, **geo)                # warm-up: the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = dhg_amd.render_page(static, None, slots, **geo)
    for t in batches[1:]:
        static.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in out]
        eager = dhg_amd.render_page(t, None, slots, **geo)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, eager))
        assert got[0].min().item() < 255


# ---------------------------------------------------------------- 9: write_page end to end
def test_write_page_end_to_end():
    m = dhg_amd.DiffusionModel(1, c2=48, precision="bf16", max_B=2, max_L=256, max_Lt=16).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(1, c2=48).items()})
    style = torch.from_numpy(spec.synthetic_inputs(1, 8, 1, seed=9)["style"])
    geo = dict(height=256, width=384, lines_per_page=4, margin_left=8.0, margin_top=8.0, pitch=56.0)
    text = "Hello there\nwhite rabbit\n\nthe end"
    lines, slots = dhg_amd.wrap_text(text)
    assert lines == ["Hello there", "white rabbit", "the end"] and slots == [0, 1, 3]
    pages, strokes = dhg_amd.write_page(text, style, m, T=4, seed=2, **geo)                  # three lines, capacity two: two sampler rounds
    assert pages.is_cuda and tuple(pages.shape) == (1, 1, 256, 384) and torch.isfinite(pages).all()
    assert pages.min().item() >= 0 and pages.max().item() <= 255
    assert [s.shape for s in strokes] == [(dhg_amd.stroke_length(len(dhg_amd.Tokenizer().encode(p))), 3) for p in lines]
    assert all(np.isfinite(s).all() for s in strokes)
    top = int(geo["margin_top"] + 2 * geo["pitch"])
    assert (pages[0, 0, top + 2:top + int(geo["pitch"]) - 2] == 255).all().item()            # the blank slot (less the pen's radius at its borders)
    direct, _, _ = dhg_amd.render_page(dhg_amd.pad_strokes(strokes), [len(s) for s in strokes], slots, **geo)
    assert torch.equal(direct, pages)
    one = dhg_amd.infer_batch(lines, style, m, T=4, seed=2)   # the rounds do not change a line
    assert all(np.array_equal(a, b) for a, b in zip(one, strokes))
