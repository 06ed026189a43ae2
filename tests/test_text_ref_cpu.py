"""CPU tests behind the text-shape cases of tests/test_gpu_blocks.py (BW.TEXT_CASES) and tests/test_gpu_text_plane.py:
  * the float64 text references (TextStyleEncoder, the text half and the cross-attention of an EncoderLayer) reproduce the fp32
    oracle at the extreme prompt and style shapes;
  * the slot -> (step, schedule index, prompt) mapping of the all-steps plane (tests/plane_ref.py) against literals;
  * the bound table of every text case: the rounding model's error per text-side tap, and no floor rows from the reference alone;
  * the bound discriminates: wrong variants of the style attention's mask, the position row clamp, the plane's FiLM row / prompt /
    pair placement, and the cross-attention's key blocks, padding bits and V^T stride exceed the GPU bound tenfold.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as R  # noqa: E402
import blocks_worker as BW  # noqa: E402
import plane_ref as P  # noqa: E402

from dhg_amd import spec  # noqa: E402
from oracle import ref_cpu  # noqa: E402

FACTOR = 2.0      # tests/test_gpu_blocks.py
TOL_F32 = 5e-5    # tests/test_gpu_blocks.py
NL = 2
LAYERS = BW.layer_names(NL)
_W = {}


def weights(prec, name=None):
    if (prec, name) not in _W:
        _W[prec, name] = R.Weights(BW.state_dict_for(NL, name), prec)
    return _W[prec, name]


# ---------------------------------------------------------------- (a) tie to the oracle
@pytest.mark.parametrize("Lt,S,pad", [(1, 1, 0), (33, 17, 1), (64, 16, 32), (97, 14, 0)])
def test_text_references_reproduce_the_oracle(Lt, S, pad):
    sdn = spec.synthetic_state_dict(NL)
    sd = {k: torch.from_numpy(v) for k, v in sdn.items()}
    B, L = 2, 16
    inp = spec.synthetic_inputs(B, L, Lt, S=S, seed=7, pad=pad)
    sg = torch.tensor([[0.25], [0.85]])
    taps = {}
    with torch.no_grad():
        ref_cpu.forward(sd, torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg, torch.from_numpy(inp["style"]), taps=taps)
    t64 = {k: v.double() for k, v in taps.items()}
    for k in ("enc1", "enc3", "enc5"):
        t64[k + ".pool"] = torch.nn.functional.avg_pool1d(taps[k].transpose(1, 2), 2).transpose(1, 2).double()
    W = weights("fp32")
    inputs = dict(strokes=torch.from_numpy(inp["strokes"]), text=torch.from_numpy(inp["text"]), sigma=sg, style=torch.from_numpy(inp["style"]))
    seen = set()
    for name in ["text_style_model"] + LAYERS:
        for k, v in R.block_output(W, name, t64.__getitem__, inputs, R.exact).items():
            err = R.max_error(v.reshape(t64[k].shape), t64[k])
            print(f"ORACLE Lt={Lt} S={S} pad={pad} {k:24s} {err:.2e}")
            assert err < 1e-5, (k, err)
            seen.add(k)
    assert {"text_style_model", "text_style_model.style", "text_style_model.t2"} | {l + s for l in LAYERS for s in ("", ".x2", ".k1", ".v1")} <= seen


# ---------------------------------------------------------------- (b) the plane's slots
def test_plane_slots_against_literals():
    """T = 70, B = 2: chunks of 64 and 6 steps; the second chunk rewrites slots 0..11 with steps 64..69 (schedule index 5..0), slots
    12..127 keep steps 6..63 of the first.  A conditioned call with t_start = 3 of T = 5 runs iterations 2..4 at indices 2, 1, 0."""
    s = P.plane_slots(70, 2)
    assert len(s) == 128
    assert s[:4] == [(64, 5, 0), (64, 5, 1), (65, 4, 0), (65, 4, 1)] and s[10:14] == [(69, 0, 0), (69, 0, 1), (6, 63, 0), (6, 63, 1)]
    assert s[126:] == [(63, 6, 0), (63, 6, 1)]
    assert all(st + i == 69 for st, i, _ in s) and sorted({st for st, _, _ in s}) == list(range(6, 70))
    assert P.plane_slots(5, 3, first=2) == [(2, 2, 0), (2, 2, 1), (2, 2, 2), (3, 1, 0), (3, 1, 1), (3, 1, 2), (4, 0, 0), (4, 0, 1), (4, 0, 2)]
    assert P.plane_slots(64, 1) == [(k, 63 - k, 0) for k in range(64)]
    # a conditioned long call: 66 iterations of T = 70 from first = 4: chunks of 64 and 2
    c = P.plane_slots(70, 1, first=4)
    assert len(c) == 64 and c[:3] == [(68, 1, 0), (69, 0, 0), (6, 63, 0)]
    # the schedule behind it: the golden 60-step table
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sched.npz"))
    assert np.array_equal(P.sigmas(60), np.sqrt(g["alpha"].astype(np.float32)))


# ---------------------------------------------------------------- (c) the bound table of the text cases
def _shape(c):
    return (c["B"], c["Lt"], c["pad"], c["S"], c.get("seed") or 0, c["weights"] or "", c["style"] or "")


TEXT_SHAPES = sorted({_shape(c) for c in BW.TEXT_CASES})
_TAB = {}


def text_table(shape):
    """(inputs, stand-in taps, {tap: (model row, model max, floor share, rows)}) of the text side at one text-case shape: the rounding
    model's chain as stand-in for the device's taps, every text-side block's model against its exact reference on the same inputs."""
    if shape not in _TAB:
        case = next(c for c in BW.TEXT_CASES if _shape(c) == shape)
        W = weights("bf16", case["weights"])
        inp = {k: torch.from_numpy(v) for k, v in BW.case_inputs(case).items()}
        taps = {}
        for name in ("sigma_ffn", "text_style_model"):
            taps.update(R.block_output(W, name, taps.__getitem__, inp, R.bf16_round))
        tab = {}

        def add(k, mo, ex):
            row, share = R.row_error(mo, ex)
            tab[k] = (row, R.max_error(mo, ex), share, ex.reshape(-1, ex.shape[-1]).shape[0])

        ex, mo = (R.block_output(W, "text_style_model", taps.__getitem__, inp, r) for r in (R.exact, R.bf16_round))
        for k in ex:
            add(k, mo[k], ex[k])
        for l in LAYERS:
            (ek, ev), (mk, mv) = (R.text_half(W, l, taps["text_style_model"], taps["sigma_ffn"], r) for r in (R.exact, R.bf16_round))
            add(l + ".k1", mk, ek)
            add(l + ".v1", mv, ev)
        _TAB[shape] = (inp, taps, tab)
    return _TAB[shape]


def test_text_bound_table():
    """Per text case and text-side tap: the rounding model's worst row and max error (what FACTOR x bounds on the GPU), in the range
    of tests/test_block_ref_cpu.py::test_bound_table, and the share of rows the REFERENCE puts under the row floor: none where a tap has
    fewer than 100 rows (with Lt = 1, B = 2 a tap has two rows: one floor row would be half of them), at most 1 % otherwise.  A case that
    broke this would get another seed (the `seed` field of the case), never another cap."""
    print()
    for shape in TEXT_SHAPES:
        _, _, tab = text_table(shape)
        for k, (row, mx, share, rows) in tab.items():
            print(f"BOUND text B{shape[0]}-Lt{shape[1]}-pad{shape[2]}-S{shape[3]}{shape[5] and '-' + shape[5]}{shape[6] and '-' + shape[6]} {k:24s} rows {rows:4d} row {row:.3e}  max {mx:.3e}  floor {share:.4f}")
            assert (share == 0) if rows < 100 else (share <= 0.01), (shape, k, share, rows)
            assert 3e-4 < row < 1e-2, (shape, k, row)
            assert 3e-4 < mx < 2e-2, (shape, k, mx)


# ---------------------------------------------------------------- (d) the bound discriminates
_FULL = {}


def full_table(Lt, pad, S=14, B=2, weights_name=None, style=None):
    """The whole model chain at a text-case shape (L = 64): (W, inputs, stand-in taps)."""
    key = (Lt, pad, S, B, weights_name, style)
    if key not in _FULL:
        case = BW._text_case(Lt, pad, S, B=B, weights=weights_name, style=style)
        W = weights("bf16", weights_name)
        inp = {k: torch.from_numpy(v) for k, v in BW.case_inputs(case).items()}
        _FULL[key] = (W, inp, R.forward_taps(W, inp, R.bf16_round))
    return _FULL[key]


def _ratio(name, where, bad, ex, mo):
    row, _ = R.row_error(bad, ex)
    bound = FACTOR * R.row_error(mo, ex)[0]
    print(f"MUTATION text {name} {where}: worst row {row:.3e}, GPU bound {bound:.3e}, ratio {row / bound:.1f}")
    return row / bound


def _block(W, block, taps, inp, key, mut):
    ex = R.block_output(W, block, taps.__getitem__, inp, R.exact)[key]
    mo = R.block_output(W, block, taps.__getitem__, inp, R.bf16_round)[key]
    bad = R.block_output(W, block, taps.__getitem__, inp, R.exact, mut=mut)[key]
    return bad, ex, mo


# The inputs under which a variant is ASSERTED: "synthetic" = spec.synthetic_state_dict and the synthetic style rows; "chosen" =
# BW.WEIGHT_SETS["peaky"] (and "flat_last" style rows for the style attention), the inputs of the text cases "..._peaky[_flat_last]",
# where the piece the variant breaks carries weight (tests/test_block_ref_cpu.py chooses inputs for its variants the same way).
# A variant that does not reach tenfold on the synthetic inputs is measured and printed there and asserted on the chosen ones; the
# synthetic ratios are in DESIGN 46.
STYLE_WRONG = [("style_last_key_left_out", {"drop_last_key": True}, S) for S in (3, 13, 16)] + \
              [("style_mask_dropped", {"unmasked_pad": True}, S) for S in (3, 4, 13)]


@pytest.mark.parametrize("name,mut,S", STYLE_WRONG, ids=[f"{n}-S{S}" for n, _, S in STYLE_WRONG])
def test_wrong_style_attention_exceeds_the_gpu_bound_tenfold(name, mut, S):
    """On the output of the TextStyleEncoder (the one tap the fused kernel leaves), at (Lt, pad) = (23, 3).  On the synthetic inputs
    the style attention is nearly uniform over its keys and weak against the residual: one key of 15 - 80 left out, or one zero-valued
    key let in, moves the output by 0.2 - 2.8 x the bf16 bound - the GPU test would miss it - so the variants are asserted on the
    chosen inputs, which the GPU cases "text_Lt23_pad3_S*_peaky_flat_last" run."""
    print()
    W, inp, taps = full_table(23, 3, S)
    _ratio(name, f"S={S} synthetic text_style_model", *_block(W, "text_style_model", taps, inp, "text_style_model", mut))
    W, inp, taps = full_table(23, 3, S, weights_name="peaky", style="flat_last")
    r = _ratio(name, f"S={S} chosen text_style_model", *_block(W, "text_style_model", taps, inp, "text_style_model", mut))
    assert r >= 10, (name, S, r)


@pytest.mark.parametrize("Lt", [2, 17, 32])
def test_wrong_position_row_of_the_last_token_exceeds_the_gpu_bound_tenfold(Lt):
    """Token Lt - 1 with the position row of token Lt - 2: visible in "<layer>.k1" itself (behind the cross-attention's softmax one
    key of Lt only moves x2 by a fraction of it)."""
    W, inp, taps = full_table(Lt, 0)
    print()
    for l in LAYERS:
        r = _ratio("pe_row_of_the_token_before", f"Lt={Lt} {l}.k1", *_block(W, l, taps, inp, l + ".k1", {"text": {"pe_clamp": True}}))
        assert r >= 10, (l, Lt, r)


CROSS_WRONG = [("last_key_dropped", {"drop_key": -1}, Lt, 0) for Lt in (32, 33, 65)] + [
    ("first_key_of_block_2_dropped", {"drop_key": 32}, 64, 0),
    ("padding_ignored_from_block_2", {"unmask_from": 32}, 64, 32), ("padding_ignored_from_block_2", {"unmask_from": 32}, 33, 1),
    ("block_2_reads_block_1", {"alias": 32}, 64, 0)]
SYNTHETIC_REACHES = {("last_key_dropped", 32), ("last_key_dropped", 33), ("padding_ignored_from_block_2", 64), ("padding_ignored_from_block_2", 33), ("block_2_reads_block_1", 64)}


@pytest.mark.parametrize("name,mut,Lt,pad", CROSS_WRONG, ids=[f"{n}-Lt{Lt}-pad{pad}" for n, _, Lt, pad in CROSS_WRONG])
def test_wrong_cross_attention_exceeds_the_gpu_bound_tenfold(name, mut, Lt, pad):
    """On "<layer>.x2", the first tap behind the cross-attention, for every layer; one kernel template serves them all (enc_a_tile), so
    the variant counts as told apart where the best layer reaches tenfold.  On the synthetic inputs one key of 64 / 65 moves a row by
    5 - 7 x the bound only (near-uniform attention): those shapes are asserted on the chosen inputs ("text_Lt*_peaky" on the GPU), the
    others on both."""
    print()
    W, inp, taps = full_table(Lt, pad)
    syn = {l: _ratio(name, f"Lt={Lt} pad={pad} synthetic {l}.x2", *_block(W, l, taps, inp, l + ".x2", {"cross": mut})) for l in LAYERS}
    W, inp, taps = full_table(Lt, pad, weights_name="peaky")
    cho = {l: _ratio(name, f"Lt={Lt} pad={pad} chosen {l}.x2", *_block(W, l, taps, inp, l + ".x2", {"cross": mut})) for l in LAYERS}
    assert max(cho.values()) >= 10, (name, Lt, pad, cho)
    if (name, Lt) in SYNTHETIC_REACHES:
        assert max(syn.values()) >= 10, (name, Lt, pad, syn)


@pytest.mark.parametrize("Lt", [17, 32, 47])
def test_fp32_values_read_with_the_stride_of_the_calls_own_length_exceed_the_bound_tenfold(Lt):
    """fp32 handles keep V^T [d][lpadT], lpadT = pad32(max_Lt) of the HANDLE; a loose handle has max_Lt = Lt + 24.  Read with
    pad32(Lt) as row stride every channel but the first reads another channel's values.  The bound of an fp32 handle is absolute.
    (At Lt = 33 a loose handle has lpadT = pad32(57) = 64 = pad32(33): the wrong stride is the right one there - ratio 0 - so the
    variant is measured where the two differ.)"""
    lpad, wrong = BW.pad32(Lt + BW.LOOSE_LT), BW.pad32(Lt)
    assert lpad != wrong and BW.pad32(33 + BW.LOOSE_LT) == BW.pad32(33)
    W = weights("fp32")
    _, inp, taps = full_table(Lt, 0)
    print()
    for l in LAYERS:
        ex = R.block_output(W, l, taps.__getitem__, inp, R.exact)[l + ".x2"]
        bad = R.block_output(W, l, taps.__getitem__, inp, R.exact, mut={"cross": {"vt_stride": (lpad, wrong)}})[l + ".x2"]
        err = (bad - ex).abs().max().item()
        print(f"MUTATION text vt_row_stride_of_the_call Lt={Lt} {l}.x2: max abs {err:.3e}, fp32 bound {TOL_F32:.1e}, ratio {err / TOL_F32:.0f}")
        assert err >= 10 * TOL_F32, (l, err)


PLANE_WRONG = [("film_row_of_the_next_step", {"film_next": True}, ("text_style_model", "enc3.k1"), ()),
               ("film_row_stride_positive", {"film_mirror": True}, ("text_style_model", "enc3.k1"), (70,)),   # (T = 5: 5.6 x; five steps leave k <= 4 rows to be off by)
               ("prompt_of_the_next_pair", {"prompt_next": True}, ("text_style_model",), (5, 70)),
               ("pairs_of_a_workgroup_swapped", {"swap_pairs": True}, ("enc3.k1", "att_layers.1.k1"), (5, 70))]


@pytest.mark.parametrize("T", [5, 70])
@pytest.mark.parametrize("name,mut,keys,reaches", PLANE_WRONG, ids=[m[0] for m in PLANE_WRONG])
def test_wrong_plane_placement_exceeds_the_gpu_bound_tenfold(name, mut, keys, reaches, T):
    """At the shapes of P1 (T = 5) and P3 (T = 70) of tests/test_gpu_text_plane.py, measured over the whole plane as that test does.
    The FiLM row of the NEXT step does not reach tenfold: neighbouring steps' sigmas are close (4.6 x the bound at T = 5, 0.4 x at
    T = 70, where the GPU test could not tell it apart) - it is printed, and the way the launch would actually go wrong, the row stride
    with the wrong sign (step k of a chunk reads the row k steps EARLIER in the schedule instead of later), is asserted beside it."""
    W = weights("bf16")
    inp = spec.synthetic_inputs(2, 16, 9, seed=21, pad=2, T=1)
    slots = P.plane_slots(T, 2)
    stand_in = P.plane_reference(W, inp["text"], inp["style"], T, slots, R.bf16_round)["text_style_model"]   # for the device's text_out plane
    ex, mo, bad = (P.plane_reference(W, inp["text"], inp["style"], T, slots, r, stand_in, m) for r, m in ((R.exact, None), (R.bf16_round, None), (R.exact, mut)))
    print()
    for k in keys:
        r = _ratio(name, f"T={T} {k}", bad[k], ex[k], mo[k])
        assert r >= 10 or T not in reaches, (name, T, k, r)
