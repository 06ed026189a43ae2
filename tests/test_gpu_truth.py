"""The page ground truth on the GPU (include/dhw.h dhw_truth, dhg_amd.group_boxes / page_truth / write_page_file(truth=True))
against tests/truth_ref.py, the numpy statement of the rules whose drawn set comes from vis.strokes_to_polylines.

Inputs (page_ref.make_strokes): offsets are multiples of 1/16, margins and pitch too, so every fp32 prefix sum, box and extent
is exact in any summation order; the scale is the reference's two fp32 divisions; and every operation of the placement is one
fp32 operation on both sides.  Boxes, spans and the scale are therefore compared bit for bit in every case: no tolerance, no
excluded case.

Labels are compared by the accept-set rule, which excludes no pixel.  With R = line_width / 2 + 0.5, eps = 1e-3 px and d_min the
float64 reference's distance to the nearest ink: the device's id must be an id whose reference distance is <= d_min + eps; where
d_min > R + eps it must be 0; and 0 is also accepted where d_min >= R - eps.  (eps: DESIGN.md §24 measured the same
tile-relative arithmetic at 0.0033 grey levels = 1.3e-5 px from the float64 reference; 1e-3 px is 75 times that.  Acceptance,
not exclusion: pixels behind a joint of two groups are at the same distance from both in exact arithmetic, and they are not
rare.  tests/test_truth_cpu.py checks on the reference alone that these inputs leave at least 90 % of the ink pixels a single
answer.)"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import page_ref  # noqa: E402
import truth_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
_refs = {}   # every reference is computed once and shared


def ref(name, *args, **kw):
    if name not in _refs:
        _refs[name] = truth_ref.truth_ref(*args, **kw)
    return _refs[name]


def bits(x):
    a = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, want, label="", fields=("boxes", "spans", "scale")):
    """got: a GroupBoxes record or a dict; want: a dict of arrays.  Prints how many elements differ per field first."""
    diff = {}
    for k in fields:
        g, w = bits(getattr(got, k) if not isinstance(got, dict) else got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, k, g.shape, w.shape, g.dtype, w.dtype)
        diff[k] = int((g != w).sum())
    print(f"{label}: differing elements {diff}")
    assert not any(diff.values()), (label, diff)


def labels_accepted(got, want, label=""):
    bad = truth_ref.label_errors(got.labels.cpu().numpy()[:, 0], want)
    ink, size = truth_ref.accept_set_sizes(want)
    differ = int((got.labels.cpu().numpy()[:, 0] != want["labels"]).sum())
    print(f"{label}: ink pixels {int(ink.sum())}, pixels with more than one accepted answer {int((size > 1).sum())}, "
          f"pixels that differ from the float64 labels {differ}, outside the accept set {int(bad.sum())}")
    assert got.labels.dtype == torch.int32 and not bad.any(), (label, int(bad.sum()))


def check(name, st, g, G, lens, slots, geo, labels, label=""):
    want = ref(name, st, g, G, lens, slots, labels=labels, **geo)   # (a case that is run with labels first keeps that reference)
    got = dhg_amd.group_boxes(st, g, G, lens, slots, labels=labels, **geo)
    assert got.boxes.is_cuda and got.boxes.dtype == torch.float32 and got.spans.dtype == torch.int32 and tuple(got.boxes.shape) == (len(st), G, 4)
    same_bits(got, want, label or name)
    if labels:
        labels_accepted(got, want, label or name)
    else:
        assert got.labels is None
    return got, want


# ---------------------------------------------------------------- 1: the basic batch
@pytest.mark.parametrize("scale", [None, 1.5])
def test_basic_matches_the_reference(scale):
    (st, g), lens, geo = truth_ref.basic_batch(), truth_ref.BASIC_LENS, dict(truth_ref.BASIC_GEO, scale=scale)
    with_labels, want = check(f"basic{scale}", st, g, 5, lens, None, geo, True)
    without, _ = check(f"basic{scale}", st, g, 5, lens, None, geo, False)
    same_bits(without, {k: getattr(with_labels, k) for k in ("boxes", "spans", "scale")}, "labels_out NULL: the same bits")
    assert (want["spans"][..., 2] > 0).sum() >= 15 and with_labels.pages == 2 and with_labels.slots is None
    s = page_ref.page_ref(st, lens, **geo)[1] if scale is None else np.float32(scale)
    assert np.array_equal(bits(with_labels.scale), bits(np.array([s], np.float32)))        # the page compositor's scale
    again = dhg_amd.group_boxes(torch.from_numpy(st).cuda(), torch.from_numpy(g).cuda().long(), 5, torch.tensor(lens, device="cuda"), labels=True, **geo)
    same_bits(again, {k: getattr(with_labels, k) for k in ("boxes", "spans", "scale", "labels")}, "second call, everything on the device",
              ("boxes", "spans", "scale", "labels"))


# ---------------------------------------------------------------- 2: thread and wave boundaries
def test_thread_and_wave_boundaries():
    st, g = truth_ref.boundary_batch()
    got, want = check("boundary", st, g, truth_ref.BOUNDARY_G, None, None, truth_ref.BOUNDARY_GEO, True)
    assert want["spans"][0, 1:4, :2].tolist() == [[15, 16], [16, 17], [17, 31]] and want["spans"][0, 9, :2].tolist() == [1023, 1025]
    assert want["spans"][1, 8, :2].tolist() == [1000, 1050]                              # one group across the wave boundary


# ---------------------------------------------------------------- 3: G = 1, G = 256, unassigned ids, interleaved groups
def test_one_group_and_ids_outside_the_range():
    (st, _), lens, geo = truth_ref.basic_batch(), truth_ref.BASIC_LENS, truth_ref.BASIC_GEO
    rng = np.random.default_rng(3)
    g = rng.choice(np.array([0, 0, 0, -1, 1, INT32_MIN, INT32_MAX], np.int64), (5, 40)).astype(np.int32)     # G = 1: only 0 is a group
    got, want = check("G1", st, g, 1, lens, None, geo, True)
    assert want["ids"][0] == 0 and len(want["ids"]) >= 5 and (want["spans"][:, 0, 2] > 0).sum() >= 4
    nothing = np.where(g == 0, 1, g)                                                       # every row unassigned
    got, want = check("unassigned", st, nothing, 1, lens, None, geo, True)
    assert not got.boxes.any().item() and not got.spans.any().item() and not got.labels.any().item() and want["ids"].tolist() == [0]


def test_256_groups_interleaved_and_one_row_groups():
    geo = dict(pages=1, height=96, width=384, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=44.0)
    rng = np.random.default_rng(33)
    st = page_ref.make_strokes(rng, 2, 300, lift_p=0.03)
    st[:, 299, 2] = 0.98
    pool = np.array([0, 255, 3, 128, 17, 254, 256, -1], np.int32)                         # (256 and -1: unassigned)
    g = pool[rng.integers(0, len(pool), (2, 75))].repeat(4, axis=1)                       # runs of 4 rows; groups come back later in the line
    got, want = check("G256", st, g, 256, None, None, geo, True)
    spans = want["spans"][0]
    assert ((spans[:, 1] - spans[:, 0]) > spans[:, 2]).any()                               # a span that holds other groups' rows: interleaved
    assert (want["spans"][..., 2] > 0).sum() >= 10 and 0 in want["ids"]
    rows = np.tile(np.arange(300, dtype=np.int32), (2, 1))                                # one row per group (the first 256 rows), boxes only
    got, want = check("rows", st, rows, 256, None, None, geo, False)
    assert (want["spans"][..., 2] == 1).sum() > 400 and want["spans"][..., 2].max() == 1


# ---------------------------------------------------------------- 4: device lengths
def test_device_lengths_outside_the_range_are_clamped():
    """Rule 1: a device-side lens entry is not checked on the host; one outside [1, L] is clamped to [0, L] before anything is
    read.  (The entries that are too large sit on lines that have a line behind them in the tensor.)"""
    (st, g), geo = truth_ref.clamped_batch(), truth_ref.BASIC_GEO      # L = 30: rows 30.. of a line are the next line's memory
    lens = torch.tensor([30 + 7, 0, 2 ** 31 - 1, -5, 30], dtype=torch.int32, device="cuda")
    got = dhg_amd.group_boxes(st, g, 5, lens, labels=True, **geo)
    want = ref("clamped", st, g, 5, truth_ref.CLAMPED_LENS, None, labels=True, **geo)
    same_bits(got, want, "clamped lengths")
    labels_accepted(got, want, "clamped lengths")
    assert (want["spans"][::2, :3, 2] > 0).all() and not want["spans"][1::2].any()


# ---------------------------------------------------------------- 5: lines that take no part
def test_lines_that_take_no_part_give_zeros():
    (st, g), slots, geo = truth_ref.nopart_batch(), truth_ref.NOPART_SLOTS, truth_ref.BASIC_GEO   # no lift, all lifts, off the pages, two that draw
    got, want = check("nopart", st, g, 5, None, slots, geo, True)
    assert not got.boxes[:3].any().item() and not got.spans[:3].any().item() and (got.spans[3:, :, 2] > 0).all().item()
    alone = dhg_amd.group_boxes(st[3:], g[3:], 5, None, slots[3:], **geo)
    assert torch.equal(alone.scale, got.scale) and torch.equal(alone.boxes, got.boxes[3:])        # the others took no part in the scale
    assert set(np.unique(got.labels.cpu().numpy()).tolist()) <= {0, *range(1 + 3 * 5, 1 + 5 * 5)}


# ---------------------------------------------------------------- 6: batch independence and line order
def test_a_line_in_a_batch_has_the_bits_of_the_line_alone_and_order_does_not_matter():
    (st, g), lens = truth_ref.basic_batch(), truth_ref.BASIC_LENS
    geo = dict(truth_ref.BASIC_GEO, pages=3)
    slots = [0, 2, 4, 6, 8]                                             # every other slot: no two lines' ink comes within R
    whole, want = check("spread", st, g, 5, lens, slots, geo, True)
    s = float(whole.scale[0])
    lab = whole.labels.cpu().numpy()
    for n, ln in enumerate(lens):
        alone = dhg_amd.group_boxes(st[n:n + 1, :ln].copy(), g[n:n + 1, :ln].copy(), 5, None, [slots[n]], labels=True, scale=s, **geo)
        assert float(alone.scale[0]) == s and torch.equal(alone.boxes[0], whole.boxes[n]) and torch.equal(alone.spans[0], whole.spans[n])
        mine = (lab >= 1 + n * 5) & (lab < 1 + (n + 1) * 5)
        assert mine.sum() > 50 and np.array_equal(alone.labels.cpu().numpy()[mine], lab[mine] - n * 5)
    order = [3, 0, 4, 2, 1]
    perm = dhg_amd.group_boxes(st[order], g[order], 5, [lens[i] for i in order], [slots[i] for i in order], labels=True, **geo)
    same_bits(perm, dict(boxes=whole.boxes[order], spans=whole.spans[order], scale=whole.scale), "permuted lines")
    inv = np.zeros(1 + 5 * 5, np.int64)
    for k, n in enumerate(order):
        inv[1 + k * 5:1 + (k + 1) * 5] = np.arange(1 + n * 5, 1 + (n + 1) * 5)
    assert np.array_equal(inv[perm.labels.cpu().numpy()], lab)          # the same map once the ids are named back


# ---------------------------------------------------------------- 7: overlapping lines
def test_overlapping_lines_under_an_explicit_scale():
    st, g = truth_ref.overlap_batch()
    got, want = check("overlap", st, g, 6, None, None, truth_ref.OVERLAP_GEO, True)
    lab = want["labels"]
    both = ((lab[0] > 0) & (lab[0] <= 6)).any(1) & (lab[0] > 6).any(1)
    assert both.sum() >= 4                                              # rows of the page that hold ink of both lines


# ---------------------------------------------------------------- 8: graph capture
def test_graph_capture_on_a_side_stream_equals_the_eager_call():
    geo = dict(pages=1, height=96, width=128, lines_per_page=2, margin_left=4.0, margin_top=4.0, pitch=44.0)
    rng = np.random.default_rng(16)
    batches = [torch.from_numpy(page_ref.make_strokes(rng, 3, 48)).cuda() for _ in range(3)]
    for t in batches:
        t[:, 47, 2] = 0.98
    slots = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    groups = (torch.arange(48, device="cuda", dtype=torch.int32) // 8).repeat(3, 1)
    fields = ("boxes", "spans", "scale", "labels")
    for scale in (None, 1.25):                                          # three launches, and two
        static = batches[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dhg_amd.group_boxes(static, groups, 6, None, slots, labels=True, scale=scale, **geo)     # warm-up: the workspace is allocated outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = dhg_amd.group_boxes(static, groups, 6, None, slots, labels=True, scale=scale, **geo)
        for t in batches[1:]:
            static.copy_(t)
            graph.replay()
            torch.cuda.synchronize()
            got = {k: getattr(out, k).clone() for k in fields}
            eager = dhg_amd.group_boxes(t, groups, 6, None, slots, labels=True, scale=scale, **geo)
            torch.cuda.synchronize()
            same_bits(eager, got, f"replay, scale {scale}", fields)
            assert (got["spans"][..., 2] > 0).sum().item() >= 12 and got["labels"].any().item()


# ---------------------------------------------------------------- 9: the label map covers the ink of the raster page
def test_labels_cover_the_ink_of_render_page():
    """Every row assigned: a pixel has a label iff render_page has ink there, but for the pixels whose distance is within eps of
    R, which the reference counts."""
    (st, g), lens, geo = truth_ref.basic_batch(), truth_ref.BASIC_LENS, truth_ref.BASIC_GEO
    want = ref("basicNone", st, g, 5, lens, None, labels=True, **dict(geo, scale=None))
    got = dhg_amd.group_boxes(st, g, 5, lens, labels=True, **geo)
    pages, sc, _ = dhg_amd.render_page(st, lens, line_width=2.0, **geo)
    assert torch.equal(sc, got.scale) and 0 not in want["ids"]
    disagree = int(((got.labels > 0) != (pages < 255)).sum())
    dmin = want["dist"].min(0)
    near = int((np.abs(dmin - want["radius"]) <= truth_ref.EPS).sum())
    print(f"labelled pixels {int((got.labels > 0).sum())}, ink pixels of render_page {int((pages < 255).sum())}, they disagree on {disagree}; "
          f"the reference has {near} pixels within eps of R")
    assert (got.labels > 0).sum().item() > 500 and disagree <= near


# ---------------------------------------------------------------- 10: write_page_file(truth=True) end to end
def test_write_page_file_truth_end_to_end(tmp_path, monkeypatch):
    """Two short lines of a synthetic two-layer model through the file front end (which builds its model from a config and a
    checkpoint, as tests/test_gpu_paths.py's file test does), four deterministic steps."""
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}
    (tmp_path / "config.yml").write_text("training_args:\n  att_layers_num: 2\n  channels: 128\n  dropout: 0.0\n")
    torch.save({"state_dict": sd}, tmp_path / "checkpoint_2000.pth")
    np.save(tmp_path / "style.npy", spec.synthetic_inputs(1, 8, 1, seed=9)["style"][0])
    monkeypatch.chdir(tmp_path)
    geo = dict(height=256, width=384, lines_per_page=4, margin_left=8.0, margin_top=8.0, pitch=56.0)
    strokes = dhg_amd.write_page_file("Hello there\n\nwhite rabbit", str(tmp_path / "style.npy"), experiment_path=str(tmp_path), output="letter",
                                      seed=2, steps=4, truth=True, truth_labels=True, **geo)
    assert len(strokes) == 2 and (tmp_path / "letter_p0.png").exists() and not (tmp_path / "letter_p1.json").exists()
    doc = json.loads((tmp_path / "letter_p0.json").read_text())
    assert (doc["page"], doc["width"], doc["height"], doc["level"], doc["groups"]) == (0, 384, 256, "word", 2)
    assert [(ln["line"], ln["slot"], ln["text"]) for ln in doc["lines"]] == [(0, 0, "Hello there"), (1, 2, "white rabbit")]
    assert [[i["text"] for i in ln["items"]] for ln in doc["lines"]] == [["Hello", "there"], ["white", "rabbit"]]
    _, _, boxes = dhg_amd.render_page(dhg_amd.pad_strokes(strokes), [len(s) for s in strokes], [0, 2], pages=1, **geo)
    boxes, drew = boxes.cpu().numpy(), 0
    labels = np.load(tmp_path / "letter_p0_labels.npy")
    assert labels.shape == (256, 384) and labels.dtype == np.int32
    for ln in doc["lines"]:
        end = 0
        for it in ln["items"]:
            a, b = it["rows"]
            if it["empty"]:
                assert (a, b) == (0, 0) and it["box"] == [0, 0, 0, 0] and not (labels == it["id"]).any()
                continue
            drew += 1
            assert end <= a < b <= len(strokes[ln["line"]])                                # contiguous spans, in text order
            end = b
            # 0.01: the file holds two decimals; and render_page may fuse the operations of its line box, which dhw_truth's
            # boxes keep apart (include/dhw.h, rule 9 of dhw_paths): the two can differ in the last bit where a word ends the line
            lb = boxes[ln["line"]]
            assert lb[0] - 0.01 <= it["box"][0] <= it["box"][2] <= lb[2] + 0.01 and lb[1] - 0.01 <= it["box"][1] <= it["box"][3] <= lb[3] + 0.01
            ys, xs = np.nonzero(labels == it["id"])
            assert len(ys) == 0 or (xs.min() >= it["box"][0] - 3 and xs.max() <= it["box"][2] + 3 and ys.min() >= it["box"][1] - 3 and ys.max() <= it["box"][3] + 3)
    print(f"items that drew something: {drew} of 4; label ids on the page: {np.unique(labels).tolist()}")
    assert drew >= 1                                                    # (the synthetic model lifts the pen: there is something to check)
