"""CPU tests of tests/block_ref.py, the float64 per-block references behind tests/test_gpu_blocks.py:
  * every block reproduces the fp32 oracle (oracle/ref_cpu.py) from the oracle's own taps;
  * the bf16 rounding helper is torch.bfloat16's rounding, ties and denormals included;
  * the bound table: the rounding model's error against the exact reference, per block, at the shapes of the GPU cases;
  * the bound discriminates: wrong variants of a block (what a subtly broken kernel computes) exceed the GPU bound -
    FACTOR x the rounding model's worst row - by at least 10 x in the per-row measure;
  * the case table of tests/blocks_worker.py, the traced list profiles/block_variants.txt and the library's variant lists
    (convblock_init() / enclayer_init() expand them) agree;
  * the ragged runs: the tile table holds every expected instantiation's tile, the length sets realise every sample-end class
    against every tile height (the unrealisable ones are a literal), the bound table per sample at the chosen lengths, and
    ragged wrong variants (a halo row, key or source row read from past a sample's end) exceed the GPU bound tenfold.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as R  # noqa: E402
import blocks_worker as BW  # noqa: E402

from dhg_amd import spec  # noqa: E402
from oracle import ref_cpu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 2.0   # tests/test_gpu_blocks.py


# ---------------------------------------------------------------- tie to the oracle
@pytest.mark.parametrize("nl", [2, 4])
def test_every_block_reproduces_the_oracle_from_the_oracles_own_taps(nl):
    sdn = spec.synthetic_state_dict(nl)
    sd = {k: torch.from_numpy(v) for k, v in sdn.items()}
    B, L, Lt = 2, 64, 9
    inp = spec.synthetic_inputs(B, L, Lt, seed=5, pad=2)
    sg = torch.tensor([[0.3], [0.8]])
    taps = {}
    with torch.no_grad():
        eps, pen = ref_cpu.forward(sd, torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg, torch.from_numpy(inp["style"]), taps=taps)
    t64 = {k: v.double() for k, v in taps.items()}
    for k in ("enc1", "enc3", "enc5"):   # (the oracle pools in place: AvgPool of its own tap)
        t64[k + ".pool"] = torch.nn.functional.avg_pool1d(taps[k].transpose(1, 2), 2).transpose(1, 2).double()
    t64["eps"], t64["pen"] = eps.double(), pen.double()
    W = R.Weights(sdn, "fp32")
    inputs = dict(strokes=torch.from_numpy(inp["strokes"]), text=torch.from_numpy(inp["text"]), sigma=sg, style=torch.from_numpy(inp["style"]))
    seen = set()
    for fused_up in (True, False):
        for name in R.block_names(nl) + ["skip_conv3+up", "skip_conv2+up", "skip_conv1+up"]:
            if name.endswith("+up"):
                sk = name[:-3]
                low = {"skip_conv3": f"att_layers.{nl - 1}", "skip_conv2": "dec3", "skip_conv1": "dec2"}[sk]
                t64[name] = t64[sk] + R.upsample(t64[low])   # the oracle taps skip_conv alone
            for k, v in R.block_output(W, name, t64.__getitem__, inputs, R.exact, fused_up).items():
                err = R.max_error(v.reshape(t64[k].shape), t64[k])
                assert err < 1e-5, (name, k, err)
                seen.add(k)
    assert {"sigma_ffn", "text_style_model", "text_style_model.style", "text_style_model.t2", "input_dense", "enc1", "enc2", "enc3", "enc3.x2", "enc3.x3",
            "enc4", "enc5", "att_dense", f"att_layers.{nl - 1}", "dec3", "dec2", "dec1", "eps", "pen", "enc1.pool", "skip_conv1+up"} <= seen


def test_float64_position_embeddings_stay_close_to_the_float32_angle_form():
    """The handle's PE.W tables (and the reference) evaluate the angle in float32; at angles up to ~1e3 rad that differs from the
    all-float64 encoding by a few float32 ulps of the angle (6e-5 each): both forms are kept, this bounds their distance."""
    for n, d, pf in ((256, 192, 4.0), (128, 256, 2.0), (64, 384, 1.0)):
        a, b = R.pos_embeddings(n, d, pf, "f32"), R.pos_embeddings(n, d, pf, "f64")
        assert a.dtype == torch.float64 and (a - b).abs().max().item() < 4 * 6.2e-5 * max(1.0, n * pf / 1024)
        assert (a - ref_cpu.pos_embeddings(n, d, pf)[0].double()).abs().max().item() < 2e-6   # (float32 sine / cosine)


# ---------------------------------------------------------------- the rounding helper
def test_bf16_round_is_torch_bfloat16_rounding():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 25)     # every binade down into the denormals
    bf = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()   # every bf16 value
    bf = bf[torch.isfinite(bf)]
    nxt = (bf.view(torch.int32) + (1 << 16)).view(torch.float32)
    ties = ((bf.double() + nxt.double()) / 2)                                                    # exactly half way (float32 values)
    ties = ties[torch.isfinite(nxt)]
    den = torch.tensor([1e-40, -3e-41, 9.1835e-41, 4.6e-41, 2 ** -133, 2 ** -134, 1.5 * 2 ** -133, 2.5 * 2 ** -133, 2 ** -126, 0.0, -0.0])
    for v in (x, bf, ties.float(), den.float()):
        want = v.to(torch.bfloat16).double()
        assert torch.equal(R.bf16_round(v.double()), want)
    assert torch.equal(torch.signbit(R.bf16_round(torch.tensor([-0.0], dtype=torch.float64))), torch.tensor([True]))
    # straight from float64: just above a tie goes UP (through float32 the value would first land on the tie, then go to even)
    tie = 1.0 + 2.0 ** -8
    assert R.bf16_round(torch.tensor([tie, tie + 2.0 ** -40, tie - 2.0 ** -40], dtype=torch.float64)).tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0]
    assert R.bf16_round(torch.tensor([3.4e38, -3.4e38, float("inf")], dtype=torch.float64)).tolist() == [float("inf"), float("-inf"), float("inf")]
    assert torch.isnan(R.bf16_round(torch.tensor([float("nan")], dtype=torch.float64))).all()


def test_weights_are_rounded_exactly_where_the_handle_packs_bf16():
    sd = spec.synthetic_state_dict(2)
    W = R.Weights(sd, "bf16")
    for k, v in sd.items():
        held, raw = W.w(k), torch.from_numpy(v).double()
        f32_kind = (k.endswith(".bias") or ".gamma_emb." in k or ".beta_emb." in k
                    or k.split(".")[0] in ("input_dense", "sigma_ffn", "output_dense", "pen_lifts_dense") or ".emb." in k)
        assert R.packed_as_element_type(k) == (not f32_kind), k
        assert torch.equal(held, raw if f32_kind else raw.float().to(torch.bfloat16).double()), k
    assert all(torch.equal(R.Weights(sd, "fp32").w(k), torch.from_numpy(v).double()) for k, v in sd.items())


# ---------------------------------------------------------------- bound table at the shapes of the GPU cases
def _shape_key(c):
    return (c["B"], c["L"], c["Lt"], c["pad"], c["nl"])


SHAPES = sorted({_shape_key(c) for c in BW.CASES})
_TABLE = {}


def bound_table(shape):
    """{tap: (model worst row error, model max error / max|ref|)} + the stand-in taps, for one GPU case shape: every block's
    rounding model against its exact reference ON THE SAME INPUTS (stand-ins for the device's taps: the model chain itself)."""
    if shape not in _TABLE:
        case = next(c for c in BW.CASES if _shape_key(c) == shape)
        W = R.Weights(spec.synthetic_state_dict(case["nl"]), "bf16")
        inp = {k: torch.from_numpy(v) for k, v in BW.case_inputs(case).items()}
        taps = R.forward_taps(W, inp, R.bf16_round)
        tab = {}
        for name in R.block_names(case["nl"]):
            ex = R.block_output(W, name, taps.__getitem__, inp, R.exact)
            mo = R.block_output(W, name, taps.__getitem__, inp, R.bf16_round)
            for k in ex:
                tab[k] = (R.row_error(mo[k], ex[k])[0], R.max_error(mo[k], ex[k]), R.row_error(mo[k], ex[k])[1])
        _TABLE[shape] = (W, inp, taps, tab)
    return _TABLE[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=["B%d-L%d-Lt%d-pad%d-nl%d" % s for s in SHAPES])
def test_bound_table(shape):
    """The rounding model's own error: what FACTOR x bounds on the GPU.  Sized by the format: one bf16 rounding moves a value by at
    most 2^-9 relative (0.195 %), a row of independently rounded values by ~2^-9 / sqrt(3) = 0.11 % in L2; a block stacks a handful
    of such roundings through O(1)-gain stages, so every block's worst row lies between one rounding of its output alone (0.05 %: rows
    need not sit at the top of their binade) and 1 % (more would mean a rounding point that amplifies: a modelling mistake)."""
    _, _, _, tab = bound_table(shape)
    print()
    for k, (row, mx, share) in tab.items():
        print(f"BOUND {shape} {k:26s} row {row:.3e}  max {mx:.3e}")
        if k in ("sigma_ffn", "eps", "pen"):
            assert row == 0 and mx == 0, k      # no bf16 value between input and output: the float32 bound applies
            continue
        assert 5e-4 < row < 1e-2, (k, row)
        assert 5e-4 < mx < 2e-2, (k, mx)
        assert share <= 0.01, (k, share)


# ---------------------------------------------------------------- the bound discriminates
S488 = next(s for s in SHAPES if s[1] == 488 and s[4] == 2)
S208 = next(s for s in SHAPES if s[1] == 208 and s[2] == 40)


def _boundaries(L, bmo):
    return list(range(bmo, L, bmo))


# (block, shape, mutation).  A tile that starts at m0 = k * BMO reads h1 row m0 - 1 as its first halo row of conv2: a halo one row
# short makes conv2 see zero there, for the output row m0 of every tile but the first.
HALO = [
    ("halo30", "enc2", S208, 30), ("halo32", "enc4", S488, 32), ("halo44", "dec3", S208, 44), ("halo46", "enc4", S208, 46),
    ("halo62", "enc2", S488, 62), ("halo124", "dec1", S488, 124), ("halo126", "enc1", S488, 126),
]
LEVEL = {"enc1": 1, "dec1": 1, "enc2": 2, "dec2": 2, "enc4": 4, "dec3": 4}
# (name, block, shape, mutation, how the block's inputs are chosen).  With the synthetic weights the deep path of a block is weak
# against its residual / skip path (three SiLUs of small values, weights at 1 / sqrt(fan_in)), so on the white-noise stand-in taps
# some wrong variants move a row by only 3 - 4 %: 8 x the bound.  The inputs are therefore chosen where the broken piece carries
# weight - None: the stand-in taps of the GPU case as they are; ("edge", bmo): a step of the signal at every tile boundary;
# ("scale", s): inputs s times larger (SiLU leaves its near-linear half-gain range); ("tail", tap, kb, amp): the keys of the last
# partial block amp times louder than the rest.  The bound is then the larger of the GPU case's and the chosen inputs' own.
MUTATIONS = [(n, blk, shp, {"conv2": {"halo": (_boundaries(shp[1] // LEVEL[blk], bmo), -1)}}, ("edge", bmo)) for n, blk, shp, bmo in HALO] + [
    ("conv1_tap_shift", "enc4", S208, {"conv1": {"shift": 1}}, ("scale", 4.0)),
    ("conv2_tap_shift", "dec2", S488, {"conv2": {"shift": 1}}, ("scale", 4.0)),
    ("film_rows_swapped", "enc1", S488, {"film": {"film_swap": True}}, None),
    ("film_rows_swapped_enc2", "enc2", S488, {"film": {"film_swap": True}}, None),
    ("pool_pairs_off_by_one", "enc1.pool", S488, {"pool_off": True}, None),
    ("pool_pairs_off_by_one_enc5", "enc5.pool", S208, {"pool_off": True}, None),
    ("self_attention_last_partial_block", "enc3", S488, {"self": {"drop_tail": 64}}, ("tail", "enc2", 64, 8.0)),               # 244 keys = 3 x 64 + 52
    ("self_attention_last_partial_block_att", "att_layers.1", S488, {"self": {"drop_tail": 32}}, ("tail", "att_layers.0", 32, 8.0)),   # 61 = 32 + 29
    ("masked_text_key_attended", "enc5", S208, {"cross": {"unmask": True}}, None),
    ("upsample_rounds_up", "dec2", S488, {"up": {"up_round": True}}, None),
    ("upsample_rounds_up_dec1", "dec1", S208, {"up": {"up_round": True}}, None),
    ("pos_factor_of_another_layer", "enc3", S488, {"pos_factor": 2.0}, None),            # enc5's
    ("pos_factor_of_another_layer_att", "att_layers.0", S488, {"pos_factor": 4.0}, None),   # enc3's
]


def _edge_envelope(L, bmo, loud=4.0, quiet=0.0):
    """[1,L,1] amplitude envelope with a step at every tile boundary k * bmo: four rows at `loud` in front of it, four rows at `quiet`
    behind it (a stroke that ends there)."""
    l = torch.arange(L)
    e = torch.ones(L, dtype=torch.float64)
    e[(l >= bmo) & (l % bmo < 4)] = quiet
    e[((l + 4) % bmo < 4) & (l + 4 >= bmo)] = loud
    return e[None, :, None]


def _chosen_taps(taps, prep, L):
    out = dict(taps)
    if prep[0] == "edge":
        # A halo that is one row short costs conv2 ONE of three taps in ONE row per tile: on white noise that row moves by 3.5 - 4 %;
        # where the signal is strong in front of the boundary and silent behind it - the missing row carries most of what the
        # first row of the tile sees - by 4.8 - 10 %.
        env = _edge_envelope(L, prep[1])
        for k, v in taps.items():
            if v.dim() == 3 and k not in ("sigma_ffn", "text_style_model") and v.shape[1] in (L, L // 2):
                out[k] = R.bf16_round(v * (env if v.shape[1] == L else R.avg_pool(env)))
    elif prep[0] == "scale":
        for k, v in taps.items():
            if k not in ("sigma_ffn", "text_style_model"):
                out[k] = R.bf16_round(v * prep[1])
    elif prep[0] == "tail":
        _, tap, kb, amp = prep
        Lk = taps[tap].shape[1]
        e = torch.ones(Lk, dtype=torch.float64)
        e[Lk - Lk % kb:] = amp
        out[tap] = R.bf16_round(taps[tap] * e[None, :, None])
    return out


@pytest.mark.parametrize("name,block,shape,mut,prep", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_wrong_variants_exceed_the_gpu_bound_tenfold(name, block, shape, mut, prep):
    W, inp, taps, tab = bound_table(shape)
    model_row = tab[block][0]
    if prep:
        taps = _chosen_taps(taps, prep, shape[1] // LEVEL.get(block, 1))
    ex = R.block_output(W, block, taps.__getitem__, inp, R.exact)[block]
    if prep:
        model_row = max(model_row, R.row_error(R.block_output(W, block, taps.__getitem__, inp, R.bf16_round)[block], ex)[0])
    bad = R.block_output(W, block, taps.__getitem__, inp, R.exact, mut=mut)[block]
    row, _ = R.row_error(bad, ex)
    bound = FACTOR * model_row
    print(f"\nMUTATION {name} {block} L={shape[1]}: worst row {row:.3e}, GPU bound {bound:.3e}, ratio {row / bound:.1f}")
    assert row >= 10 * bound, (name, row, bound)


# ---------------------------------------------------------------- case table <-> traced list <-> the instantiations compiled in
def _norm(kind, args):
    """trailing default template arguments dropped: convblock_kernel<T, BM, CO, NW, OCC = 1, UPC = 0, CH = 0, CIN = 0, TIGHT = 0, PP = 0>."""
    a = [int(x) for x in args]
    if kind == "cb":
        a += [1, 0, 0, 0, 0, 0][len(a) - 3:]
        dflt = [None, None, None, 1, 0, 0, 0, 0, 0]
        while len(a) > 3 and a[-1] == dflt[len(a) - 1]:
            a.pop()
    return f"{kind}<{','.join(map(str, a))}>"


def compiled_in():
    """The bf16 instantiations convblock_init() / enclayer_init() name: the library's own variant lists (DHW_CONV_VARIANTS /
    DHW_ENC_VARIANTS, csrc/plan/tile_plan.h) through dhw_debug_tile_variants, which for an EncoderLayer row also reports the chain
    modes has_chain() gives it (csrc/enclayer.hip)."""
    import ctypes as C
    from dhg_amd import _lib
    lib, row, out = _lib.lib(), (C.c_int * 11)(), set()
    for i in range(lib.dhw_debug_tile_variants(0, 0, row)):
        assert lib.dhw_debug_tile_variants(0, i, row) > i
        if not row[0]:
            out.add(_norm("cb", row[1:10]))
    for i in range(lib.dhw_debug_tile_variants(1, 0, row)):
        assert lib.dhw_debug_tile_variants(1, i, row) > i
        f32, dm, bm, _, modes = row[:5]
        if not f32:
            out |= {f"a<{dm},{bm}>", f"bc<{dm},{bm},0>"} | {f"bc<{dm},{bm},{m}>" for m in (1, 2) if modes >> (m - 1) & 1}
    return out


# named in the init lists, selected by no non-ragged default-store-policy launch (reasons: DESIGN.md, per-block section)
UNREACHED = {
    "a<384,64>": "lds_a_bytes<bf16, 384, 64> = 165376 B > 160 KiB: fits() is false, attr() registers nothing and pick_bm halves the tile",
    "bc<384,64,0>": "same: fits<bf16, 384, 64>() is false",
}


def traced():
    lines = [l.strip() for l in open(os.path.join(ROOT, "profiles", "block_variants.txt")) if l.strip() and not l.startswith("#")]
    return {l.split()[0] for l in lines}


def test_case_table_traced_list_and_compiled_instantiations_agree():
    """compiled_in() is the library's own report of its variant lists; the traced file is a recording.  When a kernel instantiation
    is added or removed, or has_chain() / fits() change, this fails by design."""
    remedy = ("profiles/block_variants.txt is a RECORDING: do not edit it or the sets here to match.  Add a case that selects the new "
              "instantiation to tests/blocks_worker.py (or an entry with its reason to UNREACHED), trace tests/test_gpu_blocks.py on the "
              "GPU again and regenerate the file with tools/block_variants.py (usage in its docstring).")
    table = {v for c in BW.CASES for v in c["expect"]}
    got = {v for v in traced() if v.startswith(("cb<", "a<", "bc<"))}
    assert table == got, ("case table vs traced list", sorted(table - got), sorted(got - table), remedy)
    comp = compiled_in()
    assert len(comp) >= 45, remedy
    assert comp - got == set(UNREACHED), ("named in convblock_init() / enclayer_init() but not traced", sorted(comp - got), remedy)
    assert got <= comp, ("traced but not named in the init lists", sorted(got - comp), remedy)


# ---------------------------------------------------------------- ragged runs: the tile table and the length sets
RAGGED_CASES = [c for c in BW.CASES if "base" not in c]   # (a store-policy case runs one set of its base case: no coverage of its own)


def test_tile_table_holds_the_tiles_of_every_expected_instantiation():
    """tile_table() asks the library's tile plan; every bf16 instantiation a case's `expect` list names must run at a height the
    table has for its level, and the table has no height beyond the ones the kernels are compiled for.  The literal tables pin one
    case per tiling family (worked out by hand from the rule: the comments)."""
    for c in BW.CASES:
        tab = BW.tile_table(c, "bf16")
        for lv, h in BW.expect_heights(c):
            assert h in tab[lv], (c["id"], lv, h, tab)
        for prec in ("bf16", "fp32"):
            for lv, hs in BW.tile_table(c, prec).items():
                assert hs and set(hs) <= {16, 30, 32, 44, 46, 62, 64, 124, 126}, (c["id"], prec, lv, hs)
    assert BW.tile_table(BW.CASE["default_L208"], "bf16") == {1: [62], 2: [32, 62], 4: [32, 44, 46], 8: [16]}
    assert BW.tile_table(BW.CASE["wgs2_L488"], "bf16") == {1: [124, 126], 2: [32, 62], 4: [32, 62], 8: [16]}
    assert BW.tile_table(BW.CASE["enc_bm64_L488"], "bf16") == {1: [62], 2: [62, 64], 4: [32, 64], 8: [32]}
    assert BW.tile_table(BW.CASE["default_L488"], "fp32") == {1: [30], 2: [30, 32], 4: [16, 30], 8: [16]}
    assert BW.tile_table(BW.CASE["pol42_wgs2_L488"], "bf16") == BW.tile_table(BW.CASE["wgs2_L488"], "bf16")
    # DHW_CONV_BM=64: 62-row tiles at every level; enc3 / enc5 on 32 rows (fewer than 256 tiles; bm_min = 32), the attention layers on 16
    assert BW.tile_table(BW.CASE["bm64_L488"], "bf16") == {1: [62], 2: [32, 62], 4: [32, 62], 8: [16]}
    # DHW_CONV_BM=48 at L / 4 = 92: two full 46-row tiles; 44-row tiles would need a third, so dec3 stays at 46
    assert BW.tile_table(BW.CASE["bm48_L368"], "bf16") == {1: [62], 2: [32, 62], 4: [32, 46], 8: [16]}
    # DHW_CONV_OCC=2 changes residency, not rows: L / 4 = 52 is two 46-row tiles (enc4) or two 44-row ones (dec3, TIGHT = 1)
    assert BW.tile_table(BW.CASE["occ2_L208"], "bf16") == {1: [62], 2: [32, 62], 4: [32, 44, 46], 8: [16]}
    # DHW_CONV_BM=32 without the fused input stage: the run-time-width 30-row tiles for enc4 and dec3 alike
    assert BW.tile_table(BW.CASE["noup_bm32_L208"], "bf16") == {1: [62], 2: [32, 62], 4: [30, 32], 8: [16]}
    # DHW_FUSE=0: gemm_tile_for's 64 rows from 48 rows per sample up (208, 104, 52), 32 below (26); attn.hip's 64 query rows
    assert BW.tile_table(BW.CASE["unfused_L208"], "bf16") == {1: [64], 2: [64], 4: [64], 8: [32, 64]}
    assert BW.tile_table(BW.CASE["unfused_L208"], "fp32") == {1: [32], 2: [32, 64], 4: [32, 64], 8: [32, 64]}
    # no asymmetric and no BM - 4 tiles: L / 4 = 122 on three 46-row tiles for enc4 and dec3
    assert BW.tile_table(BW.CASE["cc1_noasym_notight_L488"], "bf16") == {1: [62], 2: [32, 62], 4: [32, 46], 8: [16]}


# The (level / tile height or key block: classes) that NO multiple of 8 in [8, L] realises, per precision and padded length L; a
# case owns the entries whose height its tile table has at that level (classes a b c) and those of its key block (d0 d1 d-1).
# Why: an end at level lv is a multiple of g = 8 / lv, so "c" (1 or 2 rows before k h) never happens for h = 32 or 64 at g >= 4 and
# "d1" / "d-1" (key count = 1 or -1 mod KBS) never at g >= 2; the rest are tiles or key blocks no shorter than the level itself
# (L / 8 = 61 < 64 keys; 4 x 126 = 504; one 124-row tile start inside L = 128 ...).
UNREALISABLE = {
    ("bf16", 128): {"1/124": "a c", "1/126": "a c", "2/32": "c", "2/62": "a", "2/64": "d-1 d1", "4/32": "a b", "4/62": "a b c", "4/64": "d-1 d0 d1", "8/16": "a b", "8/64": "d-1 d0"},
    ("bf16", 136): {"1/62": "a c", "2/32": "c", "2/62": "a", "2/64": "d-1 d1", "4/64": "d-1 d0 d1", "8/64": "d-1 d0"},
    ("bf16", 208): {"1/62": "a", "1/64": "c", "2/32": "c", "2/62": "a", "2/64": "c d-1 d1", "4/64": "a b c d-1 d0 d1", "8/32": "a b c", "8/64": "a b c d-1 d0"},
    ("bf16", 368): {"2/32": "c", "2/64": "d-1 d1", "4/64": "d-1 d1", "8/64": "d-1 d0"},
    ("bf16", 488): {"1/124": "c", "1/126": "a", "2/32": "c", "2/64": "c d-1 d1", "4/64": "d-1 d1", "8/64": "d-1 d0"},
    ("bf16", 504): {"1/126": "a", "2/32": "c", "2/64": "d-1 d1", "4/64": "d-1 d1", "8/64": "d0"},
    ("fp32", 128): {"2/32": "c d-1 d1", "4/32": "d-1 d1", "8/16": "a b", "8/32": "d-1 d0"},
    ("fp32", 136): {"2/32": "c d-1 d1", "4/32": "d-1 d1", "8/32": "d-1 d0"},
    ("fp32", 208): {"1/32": "c", "2/32": "c d-1 d1", "2/64": "c", "4/32": "d-1 d1", "4/64": "a b c", "8/32": "a b c d-1 d0", "8/64": "a b c"},
    ("fp32", 368): {"2/32": "c d-1 d1", "4/32": "d-1 d1"},
    ("fp32", 488): {"2/32": "c d-1 d1", "2/64": "c", "4/32": "d-1 d1"},
    ("fp32", 504): {"2/32": "c d-1 d1", "4/32": "d-1 d1"},
}


def _owned(case, prec):
    tab, out = BW.tile_table(case, prec), set()
    for key, classes in UNREALISABLE[prec, case["L"]].items():
        lv, h = (int(x) for x in key.split("/"))
        for cl in classes.split():
            if (h in tab[lv]) if cl in "abc" else (lv > 1 and h == BW.KEY_BLOCK[prec]):
                out.add((lv, h, cl))
    return out


def test_length_sets_cover_every_tile_class():
    """For every case and precision: the union of the length sets realises every class of BW.end_classes() - an end at a tile
    start, the least distance past one, 1 or 2 rows before one, key counts 0 / 1 / -1 mod the key block - at every level and tile
    height of the case's tile table, except the triples no multiple of 8 realises, which are exactly the literal above."""
    used = set()
    for c in RAGGED_CASES:
        for prec in ("bf16", "fp32"):
            sets = BW.length_sets(c, prec)
            assert 1 <= len(sets) <= 6, (c["id"], prec)
            tallest = max(BW.tile_table(c, prec)[1])
            for s in sets:
                assert len(s) == c["B"] and all(n % 8 == 0 and 8 <= n <= c["L"] for n in s), (c["id"], prec, s)
                # one sample shorter than L by more than a whole full-resolution tile (L = 128 under 124 / 126-row tiles has no
                # such length: there, one that ends at or before the start of the second tile): early-exit tiles exist
                assert min(s) < c["L"] - tallest if c["L"] > 2 * tallest else min(s) <= min(BW.tile_table(c, prec)[1]), (c["id"], prec, s, "no early-exit tile")
            lens = {n for s in sets for n in s}
            assert 8 in lens and c["L"] in lens, (c["id"], prec)
            can, cannot = BW.wanted_classes(c, prec)
            got = set().union(*(BW.end_classes(c, prec, n) for n in lens))
            assert can <= got, (c["id"], prec, sorted(can - got))
            assert cannot == _owned(c, prec), (c["id"], prec, sorted(cannot ^ _owned(c, prec)))
            used |= {(prec, c["L"], lv, h, cl) for lv, h, cl in cannot}
    every = {(p, L, int(k.split("/")[0]), int(k.split("/")[1]), cl) for (p, L), d in UNREALISABLE.items() for k, v in d.items() for cl in v.split()}
    assert used == every, sorted(used ^ every)
    for c in BW.CASES:
        if "base" in c:   # a store-policy case: one set, one of its base case's
            for prec in ("bf16", "fp32"):
                assert BW.length_sets(c, prec) == [BW.length_sets(BW.CASE[c["base"]], prec)[BW.POLICY_SET]]
    # the examples of the classes: 248 ends at a 62-row tile start at full and half resolution; 184 two rows before one; 64 two past one
    d = BW.CASE["default_L488"]
    assert {(1, 62, "a"), (2, 62, "a")} <= BW.end_classes(d, "bf16", 248) and (1, 62, "c") in BW.end_classes(d, "bf16", 184)
    assert (1, 62, "b") in BW.end_classes(d, "bf16", 64) and {(4, 32, "a"), (8, 16, "a"), (2, 64, "d0")} <= BW.end_classes(d, "bf16", 128)
    assert (8, 64, "d1") in BW.end_classes(d, "bf16", 8) and (8, 32, "d-1") in BW.end_classes(d, "fp32", 248)


# ---------------------------------------------------------------- ragged runs: the bound table per sample
_CHAIN = {}


def _level(L, t):
    return L // t.shape[1]


def sample_parts(shape, b, n, ext=None, loud=4.0):
    """(inputs, stand-in taps) of sample b of a GPU case shape cut to n stroke rows - what the ragged reference of
    tests/test_gpu_blocks.py is evaluated on.  ext > n: the taps keep ext rows and the rows past n, which a ragged call must never
    read into a valid row, are `loud` times larger (finite stale workspace contents; the GPU test puts NaN there)."""
    W, inp, taps, _ = bound_table(shape)
    L, m = shape[1], ext or n
    i = {k: v[b:b + 1] for k, v in inp.items()}
    i["strokes"] = i["strokes"][:, :m]
    d = {}
    for k, v in taps.items():
        if k in BW.TEXT_SIDE:
            d[k] = v[b:b + 1]
            continue
        lv = _level(L, v)
        t = v[b:b + 1, :m // lv].clone()
        if t.dim() == 3:   # (pen is [B, L])
            t[:, n // lv:] = R.bf16_round(t[:, n // lv:] * loud)
        d[k] = t
    return W, i, d


def ragged_bound(shape, b, n):
    """{tap: (exact rows, model rows)} of sample b at length n: every stroke-path block's rounding model against its exact
    reference on the same cut inputs."""
    if (shape, b, n) not in _CHAIN:
        W, i, d = sample_parts(shape, b, n)
        out = {}
        for name in R.block_names(shape[4]):
            if name in BW.TEXT_SIDE:
                continue
            ex = R.block_output(W, name, d.__getitem__, i, R.exact)
            mo = R.block_output(W, name, d.__getitem__, i, R.bf16_round)
            for k in ex:
                out[k] = (ex[k].reshape(-1, ex[k].shape[-1]) if ex[k].dim() == 3 else ex[k].reshape(-1),
                          mo[k].reshape(-1, mo[k].shape[-1]) if mo[k].dim() == 3 else mo[k].reshape(-1))
        _CHAIN[shape, b, n] = out
    return _CHAIN[shape, b, n]


RAGGED_SHAPES = sorted({(_shape_key(c), tuple(map(tuple, BW.length_sets(c, "bf16")))) for c in RAGGED_CASES})


@pytest.mark.parametrize("shape,sets", RAGGED_SHAPES, ids=["B%d-L%d-Lt%d-pad%d-nl%d-" % s + "+".join("_".join(map(str, x)) for x in ls) for s, ls in RAGGED_SHAPES])
def test_bound_table_ragged(shape, sets):
    """test_bound_table at the ragged shapes: the float64 chain per sample at the chosen lengths, the valid rows of a set
    concatenated as the GPU test does.  The model's error stays in the range of the uniform table, and the reference alone keeps
    the share of rows measured against the floor at or below 1 % (a length that broke that would be replaced, not the cap)."""
    print()
    for r, lens in enumerate(sets):
        per = [ragged_bound(shape, b, n) for b, n in enumerate(lens)]
        for k in per[0]:
            ex, mo = torch.cat([p[k][0] for p in per]), torch.cat([p[k][1] for p in per])
            row, share = R.row_error(mo, ex)
            mx = R.max_error(mo, ex)
            print(f"BOUND {shape} +r{r} {'_'.join(map(str, lens))} {k:18s} row {row:.3e}  max {mx:.3e}  floor {share:.4f}")
            assert share <= 0.01, (k, lens, share)
            if k in ("eps", "pen"):
                assert row == 0 and mx == 0, k
                continue
            assert 5e-4 < row < 1e-2, (k, lens, row)
            assert 5e-4 < mx < 2e-2, (k, lens, mx)


# ---------------------------------------------------------------- ragged runs: the bound discriminates
# (name, block, shape, sample, n, what the broken kernel does).  n is a length of the case's sets whose end lies at / next to a start
# of the tile height named: the broken row is the sample's last one, whatever the height, so the height only picks the length.
#   leak conv1 / conv2 / up : ONE halo row past the end is read from the buffer instead of zero (block_ref.conv_block);
#   ("long", m)             : the whole block runs as if the sample had m > n rows - every halo row, pooled pair, Upsample source and
#                             self-attention key past the end is live - and its first n rows are kept.  m = 2 n: the end taken with
#                             the level shift one off; m = the next sample's length: lens[b + 1] for lens[b]; m = L: all Lk keys;
#   ("drop", KB)            : the last partial block of KB keys of the short sample is left out.
# The rows past the end are the stand-in taps' own rows, 4 x louder (sample_parts): finite stale values; for the key-block variants
# the inputs are chosen as for the uniform ones (tail keys 8 x louder).
RAGGED_WRONG = [
    ("x_halo_past_end_62", "enc1", S488, 1, 184, "conv1"), ("x_halo_past_end_126", "enc1", S488, 1, 376, "conv1"),
    ("x_halo_past_end_62_half", "enc2", S488, 0, 120, "conv1"), ("x_halo_past_end_32", "enc4", S488, 0, 120, "conv1"),
    ("x_halo_past_end_46", "enc4", S208, 1, 176, "conv1"),
    ("h1_halo_past_end_62", "enc1", S488, 1, 248, "conv2"), ("h1_halo_past_end_124", "dec1", S488, 1, 248, "conv2"),
    ("h1_halo_past_end_62_half", "dec2", S488, 1, 248, "conv2"), ("h1_halo_past_end_32", "enc4", S488, 0, 128, "conv2"),
    ("h1_halo_past_end_44", "dec3", S208, 1, 168, "conv2"), ("h1_halo_past_end_30", "enc2", S208, 0, 120, "conv2"),
    ("up_stage_row_past_end_dec3", "dec3", S488, 0, 120, "up"), ("up_stage_row_past_end_dec2", "dec2", S488, 1, 248, "up"),
    ("up_stage_row_past_end_dec1", "dec1", S208, 1, 128, "up"),
    ("self_attention_all_Lk_keys", "att_layers.0", S488, 0, 136, ("long", 488)), ("self_attention_all_Lk_keys_enc3", "enc3", S208, 0, 64, ("long", 208)),
    ("short_sample_last_key_block_dropped", "enc3", S488, 1, 184, ("drop", 64)), ("short_sample_last_key_block_dropped_f32", "att_layers.1", S488, 1, 392, ("drop", 32)),
    ("end_with_the_shift_one_level_off", "enc4", S488, 0, 120, ("long", 240)), ("end_with_the_shift_one_level_off_enc5", "enc5", S488, 0, 64, ("long", 128)),
    ("length_of_the_next_sample", "enc1", S488, 0, 120, ("long", 256)), ("length_of_the_next_sample_dec2", "dec2", S208, 0, 120, ("long", 176)),
    ("length_of_the_next_sample_att", "att_layers.1", S488, 0, 8, ("long", 184)),
]


@pytest.mark.parametrize("name,block,shape,b,n,what", RAGGED_WRONG, ids=[m[0] for m in RAGGED_WRONG])
def test_ragged_wrong_variants_exceed_the_gpu_bound_tenfold(name, block, shape, b, n, what):
    L = shape[1]
    lv = LEVEL.get(block) or _level(L, bound_table(shape)[2][block])
    W, i, d = sample_parts(shape, b, n)
    if isinstance(what, tuple) and what[0] == "drop":
        src = "enc2" if block == "enc3" else f"att_layers.{int(block[-1]) - 1}"
        d = _chosen_taps(d, ("tail", src, what[1], 8.0), n // lv)
        assert (n // lv) % what[1], "no partial key block at this length"
    ex = R.block_output(W, block, d.__getitem__, i, R.exact)[block]
    model_row = max(bound_table(shape)[3][block][0], R.row_error(R.block_output(W, block, d.__getitem__, i, R.bf16_round)[block], ex)[0])
    if isinstance(what, tuple) and what[0] == "drop":
        bad = R.block_output(W, block, d.__getitem__, i, R.exact, mut={"self": {"drop_tail": what[1]}})[block]
    elif isinstance(what, tuple):
        _, i2, d2 = sample_parts(shape, b, n, ext=what[1])
        bad = R.block_output(W, block, d2.__getitem__, i2, R.exact)[block][:, :ex.shape[1]]
    else:
        _, _, d2 = sample_parts(shape, b, n, ext=n + 2 * lv * 2)   # two more rows at the block's level (one at the level below)
        e = n // lv
        if what == "up":
            sk, low, h = {"dec3": ("skip_conv3", "att_layers.1", "enc5"), "dec2": ("skip_conv2", "dec3", "enc3"), "dec1": ("skip_conv1", "dec2", "enc1")}[block]
            mut = {"up_tail": (d2[low][:, e // 2:e // 2 + 1], d2[h][:, e:e + 2])}
        else:
            src = {"enc1": "input_dense", "enc2": "enc1.pool", "enc4": "enc3.pool"}.get(block)
            if src is None:   # a decoder block: the rows its input stage would compute past the end
                sk, low, h = {"dec3": ("skip_conv3", "att_layers.1", "enc5"), "dec2": ("skip_conv2", "dec3", "enc3"), "dec1": ("skip_conv1", "dec2", "enc1")}[block]
                xt = R.up_skip(W, sk, d2[low][:, :e // 2 + 1], d2[h][:, :e + 2], R.bf16_round)[:, e:e + 2]
            else:
                xt = d2[src][:, e:e + 2]
            mut = {"x_tail": xt, "leak": what}
        bad = R.block_output(W, block, d.__getitem__, i, R.exact, mut=mut)[block]
    row, _ = R.row_error(bad, ex)
    bound = FACTOR * model_row
    print(f"\nMUTATION ragged {name} {block} L={L} sample {b} n={n}: worst row {row:.3e}, GPU bound {bound:.3e}, ratio {row / bound:.1f}")
    assert row >= 10 * bound, (name, row, bound)


# ---------------------------------------------------------------- the GPU module's child-process bookkeeping (no GPU, no process)
def test_a_failed_child_is_never_started_again_and_a_fault_stops_the_other_groups(monkeypatch, tmp_path_factory):
    import subprocess
    import test_gpu_blocks as G
    started = []

    def fake_run(status):
        def run(cmd, **kw):
            started.append(cmd[-1])
            if status == "timeout":
                raise subprocess.TimeoutExpired(cmd, kw["timeout"])
            return subprocess.CompletedProcess(cmd, status, "", "boom")
        return run

    for status, stops_others in ((1, False), (-11, True), (134, True), ("timeout", True)):
        monkeypatch.setattr(G, "_CHILD", {})
        monkeypatch.setattr(G, "_ABNORMAL", [])
        monkeypatch.setattr(G.subprocess, "run", fake_run(status))
        del started[:]
        for _ in range(3):   # every test of the group fails from the record
            with pytest.raises(AssertionError):
                G.child_results("A=1", tmp_path_factory)
        assert started == ["A=1"], (status, started)
        with pytest.raises(AssertionError):
            G.child_results("B=1", tmp_path_factory)
        assert started == (["A=1"] if stops_others else ["A=1", "B=1"]), (status, started)
    # the cap counts launches: six failed children, and the seventh group is refused before anything starts
    monkeypatch.setattr(G, "_CHILD", {})
    monkeypatch.setattr(G, "_ABNORMAL", [])
    monkeypatch.setattr(G.subprocess, "run", fake_run(1))
    del started[:]
    for i in range(7):
        with pytest.raises(AssertionError):
            G.child_results(f"G={i}", tmp_path_factory)
    assert len(started) == 6
