"""The vector output on the GPU (include/dhw.h dhw_paths, dhg_amd.stroke_paths / write_page_file(svg=True)) against
tests/paths_ref.py, the numpy float32 statement of the rules whose drawn set comes from vis.strokes_to_polylines.

Inputs (page_ref.make_strokes): offsets are multiples of 1/16, margins and pitch too, so every fp32 prefix sum, box and extent
is exact in any summation order; the scale is the reference's two fp32 divisions; and every later operation is one fp32
operation on both sides.  All five outputs are therefore compared bit for bit: no tolerance, no excluded case.  (Points are
compared as bit patterns, so -0.0 and 0.0 differ and a NaN would equal itself.)"""
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_ref  # noqa: E402
import paths_ref  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("points", "index", "counts", "scale", "boxes")


def bits(x):
    a = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, want, label=""):
    """got: a StrokePaths record or a dict of arrays; want: a dict of arrays.  Prints how many elements differ per field first."""
    diff = {}
    for k in FIELDS:
        g, w = bits(getattr(got, k) if not isinstance(got, dict) else got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, k, g.shape, w.shape, g.dtype, w.dtype)
        diff[k] = int((g != w).sum())
    print(f"{label}: differing elements {diff}")
    assert not any(diff.values()), (label, diff)


def check_against_ref(st, lens, slots, geo, params, scale=None, label=""):
    smooth, tol, rounds = params
    got = dhg_amd.stroke_paths(st, lens, slots, scale=scale, smooth=smooth, tol=tol, rounds=rounds, **geo)
    want = paths_ref.paths_ref(st, lens, slots, scale=scale, smooth=smooth, tol=tol, rounds=rounds, **geo)
    assert got.points.is_cuda and got.points.dtype == torch.float32 and got.index.dtype == torch.int32 and got.counts.dtype == torch.int32
    print(f"{label} {params}: scale {float(want['scale'][0]):.9g}, kept points {want['counts'][:8, 0].tolist()}, polylines {want['counts'][:8, 1].tolist()}")
    same_bits(got, want, label)
    return got, want


# ---------------------------------------------------------------- 1: the basic batch
_page_scale = {}   # (the float64 page reference of the basic batch, computed once)


@pytest.mark.parametrize("params", [(0, 0.0, 0), (2, 0.0, 0), (0, 0.5, 4), (2, 0.5, 4), (8, 1.0, 8)])
def test_basic_matches_the_reference_bit_for_bit(params):
    st, lens, geo = paths_ref.basic_batch(), paths_ref.BASIC_LENS, paths_ref.BASIC_GEO
    got, want = check_against_ref(st, lens, None, geo, params, label="basic")              # NaN past every length, the automatic scale
    assert (want["counts"][:, 0] >= 2).all() and got.pages == 2 and got.slots is None
    if "s" not in _page_scale:
        _page_scale["s"] = page_ref.page_ref(st, lens, **geo)[1]
    assert np.array_equal(bits(got.scale), bits(_page_scale["s"].reshape(1)))              # the page compositor's scale
    again = dhg_amd.stroke_paths(torch.from_numpy(st).cuda(), torch.tensor(lens, device="cuda"), smooth=params[0], tol=params[1], rounds=params[2], **geo)
    same_bits(again, {k: getattr(got, k) for k in FIELDS}, "second call, lengths on the device")


# ---------------------------------------------------------------- 2: thread and wave boundaries
def test_thread_and_wave_boundaries():
    st = paths_ref.boundary_batch()
    got, want = check_against_ref(st, None, None, paths_ref.BOUNDARY_GEO, (2, 0.5, 4), label="boundaries")
    assert st.shape == (2, 1100, 3) and (np.round(st[0, paths_ref.BOUNDARY_LIFTS, 2]) == 1).all() and not np.round(st[1, 990:1061, 2]).any()
    check_against_ref(st, None, None, paths_ref.BOUNDARY_GEO, (0, 0.0, 0), label="boundaries, every point")


# ---------------------------------------------------------------- 3: the maximum length
def test_maximum_length():
    st = page_ref.make_strokes(np.random.default_rng(23), 1, 4096, lift_p=0.02)
    st[0, 4095, 2] = 0.98
    geo = dict(pages=1, height=96, width=2048, lines_per_page=1, margin_left=8.0, margin_top=8.0, pitch=80.0)
    got, want = check_against_ref(st, None, None, geo, (1, 0.25, 8), label="L = 4096")
    rows = want["index"][0, :want["counts"][0, 0], 0]
    assert rows.max() > 4000 and want["counts"][0, 1] > 20 and 2 * want["counts"][0, 0] < 4096


# ---------------------------------------------------------------- 4: many lines, degenerate cases
def test_many_lines_and_degenerate_cases():
    st, lens, slots = paths_ref.degenerate_batch()
    got, want = check_against_ref(st, lens, slots, paths_ref.DEGENERATE_GEO, (2, 0.5, 4), label="70 lines")
    assert len(st) == 70 and want["counts"][:5].tolist() == [[0, 0]] * 5 and (want["counts"][5:, 0] >= 2).all()
    assert not got.boxes[:5].any().item() and got.boxes[5:, 2].min().item() > 0
    check_against_ref(st, lens, slots, paths_ref.DEGENERATE_GEO, (0, 0.5, 4), label="70 lines, no smoothing")   # the hairpin stays one: len2 == 0
    # a batch in which no line takes part: scale 1, nothing else
    none = dhg_amd.stroke_paths(st[:5], lens[:5], slots[:5], **paths_ref.DEGENERATE_GEO)
    assert float(none.scale[0]) == 1.0 and not none.counts.any().item() and not none.points.any().item() and (none.index == -1).all().item()


def test_device_lengths_outside_the_range_are_clamped():
    """Rule 1: a device-side lens entry is not checked on the host; one outside [1, L] is clamped to [0, L] before anything is read.
    (The entries that are too large sit on lines that have a line behind them in the tensor.)"""
    st, geo = paths_ref.basic_batch(), paths_ref.BASIC_GEO
    st = np.nan_to_num(st[:, :30], nan=0.0)                             # L = 30: rows 30.. of a line are the next line's memory
    st[:, 29, 2] = 0.98
    lens = torch.tensor([30 + 7, 0, 2 ** 31 - 1, -5, 30], dtype=torch.int32, device="cuda")
    got = dhg_amd.stroke_paths(st, lens, smooth=2, tol=0.5, rounds=4, **geo)
    want = paths_ref.paths_ref(st, [30, 30, 30, 30, 30], [0, 99, 2, 99, 4], smooth=2, tol=0.5, rounds=4, **geo)   # 0 strokes: as a line that takes no part
    same_bits(got, want, "clamped lengths")
    assert want["counts"][:, 0].tolist()[1::2] == [0, 0] and (want["counts"][::2, 0] >= 2).all()


# ---------------------------------------------------------------- 5: batch independence and line order
def test_a_line_in_a_batch_has_the_bits_of_the_line_alone_and_order_does_not_matter():
    st, lens, geo = paths_ref.basic_batch(), paths_ref.BASIC_LENS, paths_ref.BASIC_GEO
    kw = dict(smooth=2, tol=0.5, rounds=4)
    whole = dhg_amd.stroke_paths(st, lens, **kw, **geo)
    s = float(whole.scale[0])
    for n, ln in enumerate(lens):
        alone = dhg_amd.stroke_paths(st[n:n + 1, :ln].copy(), None, [n], scale=s, **kw, **geo)      # N = 1, the same slot, the batch's scale
        assert float(alone.scale[0]) == s
        assert torch.equal(alone.points[0], whole.points[n, :ln]) and torch.equal(alone.index[0], whole.index[n, :ln])
        assert torch.equal(alone.counts[0], whole.counts[n]) and torch.equal(alone.boxes[0], whole.boxes[n])
        assert not whole.points[n, ln:].any().item() and (whole.index[n, ln:] == -1).all().item()
    order = [3, 0, 4, 2, 1]
    perm = dhg_amd.stroke_paths(st[order], [lens[i] for i in order], order, **kw, **geo)
    same_bits(perm, dict(points=whole.points[order], index=whole.index[order], counts=whole.counts[order], scale=whole.scale, boxes=whole.boxes[order]),
              "permuted lines")


# ---------------------------------------------------------------- 6: graph capture
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
        dhg_amd.stroke_paths(static, None, slots, **geo)               # warm-up: the workspace is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = dhg_amd.stroke_paths(static, None, slots, **geo)
    for t in batches[1:]:
        static.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        got = {k: getattr(out, k).clone() for k in FIELDS}
        eager = dhg_amd.stroke_paths(t, None, slots, **geo)
        torch.cuda.synchronize()
        same_bits(eager, got, "replay")
        assert got["counts"][:, 0].min().item() >= 2


# ---------------------------------------------------------------- 7: the vector page lies on the raster page
def test_every_path_point_lies_on_the_ink_of_the_raster_page():
    """smooth = 0, rounds = 0: every path point is an endpoint of a drawn segment, so render_page (line_width 2) has ink there.
    The point lies at most 0.7072 px from the centre of the pixel that contains it (half a diagonal, and room for the two
    entries' roundings of the placement), so that pixel's coverage is at least 1.5 - 0.7072 = 0.7928 and its value at most
    255 (1 - 0.7928) = 52.9; with the 0.5 grey levels of tests/test_gpu_page.py: below 64."""
    st, lens, geo = paths_ref.basic_batch(), paths_ref.BASIC_LENS, paths_ref.BASIC_GEO
    paths = dhg_amd.stroke_paths(st, lens, smooth=0, rounds=0, **geo)
    pages, sc, boxes = dhg_amd.render_page(st, lens, line_width=2.0, **geo)
    assert torch.equal(sc, paths.scale)
    im, pts, counts = pages.cpu().numpy()[:, 0], paths.points.cpu().numpy(), paths.counts.cpu().numpy()
    checked, worst = 0, 0.0
    for n in range(len(lens)):
        p = pts[n, :counts[n, 0], :2]
        col, row = np.floor(p[:, 0]).astype(int), np.floor(p[:, 1]).astype(int)
        inside = (col >= 0) & (col < geo["width"]) & (row >= 0) & (row < geo["height"])
        v = im[n // geo["lines_per_page"], row[inside], col[inside]]
        checked, worst = checked + len(v), max(worst, float(v.max()))
        assert (v < 64).all(), (n, v.max())
    print(f"{checked} path points inside the pages, darkest-pixel bound 64, largest value {worst:.2f}")
    assert checked > 100


# ---------------------------------------------------------------- 8: write_page_file(svg=True) end to end
def test_write_page_file_svg_end_to_end(tmp_path, monkeypatch):
    """Two short lines of a synthetic two-layer model through the file front end (which builds its model from a config and a
    checkpoint, as tests/test_gpu_render.py's file test does), four deterministic steps."""
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}
    (tmp_path / "config.yml").write_text("training_args:\n  att_layers_num: 2\n  channels: 128\n  dropout: 0.0\n")
    torch.save({"state_dict": sd}, tmp_path / "checkpoint_2000.pth")
    np.save(tmp_path / "style.npy", spec.synthetic_inputs(1, 8, 1, seed=9)["style"][0])
    monkeypatch.chdir(tmp_path)
    geo = dict(height=256, width=384, lines_per_page=4, margin_left=8.0, margin_top=8.0, pitch=56.0)
    strokes = dhg_amd.write_page_file("Hello there\n\nwhite rabbit", str(tmp_path / "style.npy"), experiment_path=str(tmp_path), output="letter",
                                      seed=2, steps=4, svg=True, **geo)
    assert len(strokes) == 2 and (tmp_path / "letter_p0.png").exists() and not (tmp_path / "letter_p1.svg").exists()
    root = ET.fromstring((tmp_path / "letter_p0.svg").read_text())
    assert root.tag == "{http://www.w3.org/2000/svg}svg" and root.get("width") == "384" and root.get("height") == "256" and root.get("viewBox") == "0 0 384 256"
    direct = dhg_amd.stroke_paths(dhg_amd.pad_strokes(strokes), [len(s) for s in strokes], [0, 2], pages=1, **geo)
    drawn = [n for n in range(2) if int(direct.counts[n, 0]) > 0]
    assert drawn                                                       # (the synthetic model lifts the pen: there is something to check)
    paths = list(root)
    assert [p.get("id") for p in paths] == [f"line{n}" for n in drawn] and all(p.tag.endswith("}path") for p in paths)
    for p in paths:
        assert p.get("fill") == "none" and p.get("stroke-width") == "2.00" and p.get("d").startswith("M ")
        nums = np.array([float(t) for t in p.get("d").split() if t not in "MCL"])
        assert len(nums) >= 4 and np.isfinite(nums).all()
        assert nums.min() >= -geo["pitch"] and nums.max() <= max(geo["width"], geo["height"]) + geo["pitch"]   # the page widened by pitch
        xs, ys = nums[0::2], nums[1::2]
        assert xs.max() <= geo["width"] + geo["pitch"] and ys.max() <= geo["height"] + geo["pitch"]
    print(f"lines drawn {drawn}, kept points {direct.counts[:, 0].tolist()}")
    assert (tmp_path / "letter_p0.svg").read_text() == dhg_amd.page_svg(direct, 0)
