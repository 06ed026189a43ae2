"""The all-steps text plane of dhw_sample, pair by pair, against float64 (tests/plane_ref.py).  Runs on the MI355X only (-m gpu).

dhw_sample evaluates the text side for every step of the schedule in one batched pass per chunk of 64 steps: n = steps x prompts
(step, prompt) pairs, a FiLM row per step read through a NEGATIVE row stride, one or two pairs per workgroup of text_layer_kernel.
dhw_debug_read skips these launches (their buffers are not the per-call ones); dhw_debug_read_plane copies out what the last call
left in them: "text_style_model", "<layer>.k1" and "<layer>.v1" for every pair slot the call's chunking wrote.

Each slot is checked against the float64 reference of ITS step and prompt (plane_ref.plane_slots: which step a slot holds after the
call; sigma from the project's Python statement of the schedule, never read back from the library): TextStyleEncoder from the
call's own prompts and styles, the layers' text keys and values from the device's own text_out of that slot.  Measures and bounds
are those of tests/test_gpu_blocks.py, over all checked slots of a buffer at once: fp32 handles 5e-5 absolute, bf16 handles within
FACTOR = 2 of the rounding model in the per-row and the max measure, at most 1 % of rows against the row floor.  Every figure is
printed before it is asserted: "PLANE <case> <prec> <buffer> gpu_row model_row ratio gpu_max model_max ratio".
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
from test_gpu_blocks import FACTOR, FLOOR_SHARE, TOL_F32, weights  # noqa: E402

pytestmark = pytest.mark.gpu

NL, L = 2, 16
LAYERS = BW.layer_names(NL)
BUFFERS = ["text_style_model"] + [l + s for l in LAYERS for s in (".k1", ".v1")]


def make_model(prec, B, Lt, S):
    import dhg_amd
    m = dhg_amd.DiffusionModel(NL, precision=prec, max_B=B, max_L=L, max_Lt=Lt, style_rows=S).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in BW.state_dict_for(NL).items()}, strict=True)
    return m


def inputs(B, Lt, S, T, pad, seed=21):
    from dhg_amd import spec
    return spec.synthetic_inputs(B, L, Lt, S=S, seed=seed, pad=pad, T=T)


def sample_and_read(m, env, inp, T):
    """One dhw_sample with given noise on m (its handle is created by the first call, under env) -> {buffer: float32 [pairs, rows, cols]}
    as stored.  The samples themselves are not looked at: the text side does not depend on the strokes."""
    import dhg_amd
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    with BW.environ(env):
        dhg_amd.sample(m, tx, sv, L=L, T=T, noise=nz)
    return {k: m.debug_read_plane(k).numpy() for k in BUFFERS}


def as_rows(planes, Lt):
    """Every "<layer>.v1" as rows [pairs, Lt, d] (the handles here have max_Lt = Lt: lpadT = pad32(Lt))."""
    out = dict(planes)
    for l in LAYERS:
        out[l + ".v1"] = BW.values_as_rows(planes[l + ".v1"], Lt, BW.LAYER_WIDTH.get(l, 384), BW.pad32(Lt))[0]
    return out


def check_plane(tag, prec, planes, inp, T, B, sel=None, first=0):
    """planes: as_rows() of one call.  sel: the slots to check (default: all)."""
    slots = P.plane_slots(T, B, first)
    Lt = inp["text"].shape[1]
    for k in BUFFERS:
        assert planes[k].shape[:2] == (len(slots), Lt), (tag, k, planes[k].shape, len(slots))
        assert np.isfinite(planes[k]).all(), (tag, k, "not finite")
    sel = list(range(len(slots))) if sel is None else sel
    W = weights(NL, prec)
    dev = {k: torch.from_numpy(v[sel]).double() for k, v in planes.items()}
    chosen = [slots[i] for i in sel]
    ref = P.plane_reference(W, inp["text"], inp["style"], T, chosen, R.exact, dev["text_style_model"])
    mod = P.plane_reference(W, inp["text"], inp["style"], T, chosen, R.bf16_round, dev["text_style_model"]) if prec == "bf16" else None
    failures = []
    for k in BUFFERS:
        have, want = dev[k], ref[k]
        if prec == "fp32":
            amax = (have - want).abs().max().item()
            print(f"PLANE {tag} {prec} {k} abs {amax:.3e}")
            if not amax <= TOL_F32:
                failures.append((k, "abs", amax, TOL_F32))
            continue
        g_row, share = R.row_error(have, want)
        m_row, _ = R.row_error(mod[k], want)
        g_max, m_max = R.max_error(have, want), R.max_error(mod[k], want)
        per_pair = ((have - want).reshape(len(sel), -1).norm(dim=1) / want.reshape(len(sel), -1).norm(dim=1))
        print(f"PLANE {tag} {prec} {k} {g_row:.3e} {m_row:.3e} {g_row / m_row:.2f} {g_max:.3e} {m_max:.3e} {g_max / m_max:.2f} floor {share:.4f} "
              f"worst slot {sel[int(per_pair.argmax())]}")
        if not g_row <= FACTOR * m_row:
            failures.append((k, "row", g_row, m_row))
        if not g_max <= FACTOR * m_max:
            failures.append((k, "max", g_max, m_max))
        if not share <= FLOOR_SHARE:
            failures.append((k, "floor share", share, FLOOR_SHARE))
    assert not failures, (tag, prec, failures)


def assert_same_bits(a, b, what):
    for k in BUFFERS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


_P1 = {}


def p1():
    """P1: B = 2, Lt = 9, pad 2, S = 14, T = 5 on two handles, one pair and two pairs per workgroup forced."""
    if not _P1:
        inp = inputs(2, 9, 14, 5, 2)
        for pairs in ("1", "2"):
            m = make_model("bf16", 2, 9, 14)
            _P1[pairs] = (m, sample_and_read(m, {"DHW_TEXT_PAIRS": pairs}, inp, 5))
        _P1["inp"] = inp
    return _P1


def test_p1_every_pair_in_both_launch_forms():
    d = p1()
    for pairs in ("1", "2"):
        check_plane(f"P1_pairs{pairs}", "bf16", as_rows(d[pairs][1], 9), d["inp"], 5, 2)
    assert_same_bits(d["1"][1], d["2"][1], "one pair vs two pairs per workgroup")


def test_p2_odd_batch_keeps_one_pair_per_workgroup():
    inp = inputs(3, 17, 14, 4, 1)
    got = {}
    for pairs in ("1", "2"):
        got[pairs] = sample_and_read(make_model("bf16", 3, 17, 14), {"DHW_TEXT_PAIRS": pairs}, inp, 4)
    check_plane("P2_B3", "bf16", as_rows(got["2"], 17), inp, 4, 3)
    assert_same_bits(got["1"], got["2"], "forced two pairs at an odd batch vs one pair")


def test_p3_two_chunks_of_64_and_6_steps():
    """After the call slots 0..11 hold steps 64..69 and slots 12..127 steps 6..63 of the first chunk: the negative FiLM row stride,
    the chunk's offset into the schedule and the short last chunk."""
    inp = inputs(2, 9, 14, 70, 2)
    planes = as_rows(sample_and_read(make_model("bf16", 2, 9, 14), {}, inp, 70), 9)
    check_plane("P3_T70", "bf16", planes, inp, 70, 2)


def test_p4_the_launchers_own_choice_of_two_pairs_at_1024_pairs():
    """n = 64 x 16 = 1024: text_layer_kernel runs two pairs per workgroup by the launcher's own rule, both halves of every 64-row tile
    full (Lt = 32), at the full 80 style keys."""
    B, T, Lt, S = 16, 64, 32, 16
    inp = inputs(B, Lt, S, T, 0)
    own = sample_and_read(make_model("bf16", B, Lt, S), {}, inp, T)
    one = sample_and_read(make_model("bf16", B, Lt, S), {"DHW_TEXT_PAIRS": "1"}, inp, T)
    assert_same_bits(own, one, "the launcher's choice vs one pair per workgroup")
    sel = [k * B + b for k in (0, 31, 63) for b in range(B)]
    check_plane("P4_n1024", "bf16", as_rows(own, Lt), inp, T, B, sel)


@pytest.mark.parametrize("Lt,S", [(32, 1), (17, 16), (1, 14)])
def test_p5_two_pairs_at_the_shape_corners(Lt, S):
    inp = inputs(2, Lt, S, 3, 0)
    planes = as_rows(sample_and_read(make_model("bf16", 2, Lt, S), {"DHW_TEXT_PAIRS": "2"}, inp, 3), Lt)
    check_plane(f"P5_Lt{Lt}_S{S}", "bf16", planes, inp, 3, 2)


@pytest.mark.parametrize("prec,env", [("fp32", {}), ("bf16", {"DHW_FUSE_TEXT": "0"})], ids=["fp32", "bf16_fuse_text0"])
def test_p6_the_generic_plane(prec, env):
    """P1's shape where the plane runs through the generic GEMMs and attn.hip (gp_text, csrc/sampler/denoiser.cpp)."""
    inp = p1()["inp"]
    planes = as_rows(sample_and_read(make_model(prec, 2, 9, 14), env, inp, 5), 9)
    check_plane(f"P6_{prec}", prec, planes, inp, 5, 2)


def test_p7_a_second_call_reuses_the_plane_and_the_hook_leaves_its_tag_alone():
    d = p1()
    m, first = d["2"]
    again = sample_and_read(m, {}, d["inp"], 5)
    last, calls, reused = m.plane_reuse()
    print(f"REUSE P7 last {last} calls {calls} reused {reused}")
    assert last == 1 and calls >= 2 and reused >= 1, (last, calls, reused)
    assert_same_bits(first, again, "the plane of the first call vs the plane after a call that reused it")


def test_the_hook_refuses_a_handle_without_a_sample_call():
    from dhg_amd import _lib
    from dhg_amd import spec
    m = make_model("bf16", 2, 9, 14)
    i = spec.synthetic_inputs(2, L, 9, seed=1)
    m(torch.from_numpy(i["strokes"]).cuda(), torch.from_numpy(i["text"]).cuda(), torch.full((2, 1), 0.5).cuda(), torch.from_numpy(i["style"]).cuda())
    with pytest.raises(_lib.DhwError, match="no all-steps text plane"):
        m.debug_read_plane("text_style_model")
