"""The cases of tests/test_gpu_blocks.py, the code that runs one of them on the device, and - run as a script - the child
process for the cases whose library switch is frozen at first use.

A CASE is one ``dhw_forward`` at a shape and a set of switches; what comes back is every tap the call set (as float32 arrays,
exactly what ``dhw_debug_read`` returns) plus eps / pen.  Three kinds of switch:
  handle : read at dhw_create (DHW_FUSE, DHW_FUSE_UP, DHW_CHAIN, ...): set while the handle is created;
  launch : read at every launch (DHW_CONV_WGS, DHW_CONV_BM, DHW_CONV_PP, DHW_CONV_OCC, DHW_ENC_BM*, DHW_ENC_WGS): set around the call;
  static : function-static in the library (DHW_CHAIN_CONV, DHW_CONV_TIGHT, DHW_CONV_ASYM, DHW_CONV_RT, DHW_GEMM_W8, DHW_FLAT_TEXT):
           the first launch of the process freezes them, so such a case only means something in a process started with them.

    python tests/blocks_worker.py OUT.npz GROUP [cases-only]      runs every case of static group GROUP in both precisions, uniform and once
                                                     per length set of the case (keys "<case>+r<k>/<prec>/<tap>") (and, for the
                                                     DHW_CHAIN_CONV and DHW_FLAT_TEXT groups, the short sampling run of
                                                     test_conv_chain_switch_... / test_flat_text_switch_does_not_change_the_samples)
                                                     and writes OUT.npz

``expect`` lists the bf16 kernel instantiations the launchers select for the case (the tile plan of csrc/plan/tile_plan.h gives
exactly these: tests/test_tile_plan_cpu.py; profiles/block_variants.txt is the traced list).  Notation: cb<BM,CO,NW,OCC,UPC,CH,CIN,TIGHT,PP> = convblock_kernel<bf16_t, ...> with trailing defaults dropped,
a<DM,BM> = enc_a_kernel, bc<DM,BM,NEXT> = enc_bc_kernel.  The ragged kernels carry the same template names, and the plan sees
B and the padded L only, so a case's list also holds for its ragged runs (run_case(..., lengths=), length_sets()).
"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_B, MAX_L, MAX_LT = 3, 512, 40

# the EncoderLayer launches of an unforced call at B <= 3, L <= 512 (enc_plan_bm: every level has fewer than 256 tiles):
# enc2 continues into enc3.a, enc5.bc into AvgPool + att_dense + att_layers.0.a, every attention layer into the next one's first half
_EL_DEFAULT = ["bc<192,32,0>", "bc<256,32,2>", "bc<384,16,1>", "bc<384,16,0>"]
_EL_NOCHAIN = ["a<192,32>", "bc<192,32,0>", "a<256,16>", "bc<256,16,0>", "a<384,16>", "bc<384,16,0>"]


def _case(id, L, B=2, Lt=23, pad=3, nl=2, handle=None, launch=None, static=None, expect=(), S=14, tight=None, weights=None, style=None):
    """S: style rows of the call (and of the handle: S5 = 5 S keys of the style attention).  tight: the handle's capacity - None: the
    shared handle of CASES (MAX_B, MAX_L, MAX_LT); False ("loose"): max_B = 3, max_Lt = Lt + 24, max_L = L; True: max_B = B,
    max_Lt = Lt, max_L = L (handle_caps).  weights: None = spec.synthetic_state_dict, or a name of WEIGHT_SETS; style: None = the
    synthetic style rows, or "flat_last" (case_inputs)."""
    return dict(id=id, B=B, L=L, Lt=Lt, pad=pad, nl=nl, handle=handle or {}, launch=launch or {}, static=static or {}, expect=list(expect), S=S, tight=tight,
                weights=weights, style=style)


CASES = [
    # ---- the launchers' own choice.  L = 488: 8 tiles of 62 rows (last 54) at full resolution, 4 of 62 (last 58) at L/2, the asymmetric
    # 32-row tiles at L/4 = 122 (4 tiles, last 26) with enc4 -> enc5.a; tile starts 62 k / 32 k against pooling pairs at even rows
    _case("default_L488", 488, expect=["cb<64,128,8,1,0,0,128>", "cb<64,192,8,1,0,1,128>", "cb<32,256,8,1,0,1,192,2>", "cb<32,256,8,1,384,0,384,2>",
                                       "cb<64,192,8,1,256,0,256>", "cb<64,128,8,1,192,0,192>"] + _EL_DEFAULT),
    # L = 208: L/4 = 52 -> 2 tiles of 46 rows (last 6) for enc4, 2 of 44 (TIGHT = 1, last 8) for dec3; generic text side (Lt = 40 > 32)
    _case("default_L208", 208, B=3, Lt=40, pad=11, expect=["cb<64,128,8,1,0,0,128>", "cb<64,192,8,1,0,1,128>", "cb<48,256,8,1,0,0,192>", "cb<48,256,8,1,384,0,384,1>",
                                                          "cb<64,192,8,1,256,0,256>", "cb<64,128,8,1,192,0,192>", "a<256,32>"] + _EL_DEFAULT),
    # four attention layers; L/4 = 34: the asymmetric tiles again (2 per sample, the second with 2 rows)
    _case("default_nl4", 136, B=3, nl=4, Lt=7, pad=2, expect=["cb<64,128,8,1,0,0,128>", "cb<64,192,8,1,0,1,128>", "cb<32,256,8,1,0,1,192,2>", "cb<32,256,8,1,384,0,384,2>",
                                                              "cb<64,192,8,1,256,0,256>", "cb<64,128,8,1,192,0,192>"] + _EL_DEFAULT),
    # ---- DHW_CONV_WGS=2: "more than two workgroups do not fit one round" -> the tall tiles for enc1 / dec1, 62-row tiles for the 256-wide blocks
    # L = 488: enc1 4 tiles of 126 (last 110); dec1 tight(128) holds (4 tiles either way) -> 124-row tiles (last 116)
    _case("wgs2_L488", 488, launch={"DHW_CONV_WGS": "2"}, expect=["cb<128,128,8,1,0,0,128>", "cb<64,192,8,1,0,1,128>", "cb<64,256,8,1,0,0,192>", "cb<64,256,8,1,384,0,384>",
                                                                  "cb<64,192,8,1,256,0,256>", "cb<128,128,8,1,192,0,192,1>", "a<256,32>"] + _EL_DEFAULT),
    # L = 504 = 4 * 126: tight(128) fails (5 tiles of 124) -> 126-row dec1 tiles, all full
    _case("wgs2_L504", 504, launch={"DHW_CONV_WGS": "2"}, expect=["cb<128,128,8,1,0,0,128>", "cb<128,128,8,1,192,0,192>", "cb<64,256,8,1,0,0,192>", "cb<64,256,8,1,384,0,384>"]),
    # L = 128: two 124-row dec1 tiles, the second with 4 rows; two 126-row enc1 tiles, the second with 2
    _case("wgs2_L128", 128, B=3, launch={"DHW_CONV_WGS": "2"}, expect=["cb<128,128,8,1,0,0,128>", "cb<128,128,8,1,192,0,192,1>"]),
    _case("wgs2_pp1_L488", 488, launch={"DHW_CONV_WGS": "2", "DHW_CONV_PP": "1"}, expect=["cb<128,128,8,1,0,0,128,0,1>", "cb<128,128,8,1,192,0,192,1>"]),
    _case("wgs2_pp2_L504", 504, launch={"DHW_CONV_WGS": "2", "DHW_CONV_PP": "2"}, expect=["cb<128,128,8,1,0,0,128>", "cb<128,128,8,1,192,0,192,0,1>"]),
    _case("wgs2_pp3_L488", 488, launch={"DHW_CONV_WGS": "2", "DHW_CONV_PP": "3"}, expect=["cb<128,128,8,1,0,0,128,0,1>", "cb<128,128,8,1,192,0,192,1,1>"]),
    # ---- 62-row tiles everywhere, no ConvBlock -> EncoderLayer chain (convblock_chain_supported refuses a forced tile)
    _case("bm64_L488", 488, launch={"DHW_CONV_BM": "64"}, expect=["cb<64,128,8,1,0,0,128>", "cb<64,192,8,1,0,0,128>", "cb<64,256,8,1,0,0,192>", "cb<64,256,8,1,384,0,384>",
                                                                  "cb<64,192,8,1,256,0,256>", "cb<64,128,8,1,192,0,192>", "a<192,32>", "a<256,32>"] + _EL_DEFAULT),
    # DHW_CONV_BM=48 at L/4 = 92: two full 46-row tiles; tight(48) fails (3 tiles of 44) -> the 46-row dec3 with the fused input stage
    _case("bm48_L368", 368, launch={"DHW_CONV_BM": "48"}, expect=["cb<48,256,8,1,0,0,192>", "cb<48,256,8,1,384,0,384>"]),
    # two co-resident workgroups per CU (DHW_CONV_OCC=2) for the 128- and 192-wide encoder blocks
    _case("occ2_L208", 208, launch={"DHW_CONV_OCC": "2"}, expect=["cb<64,128,8,2,0,0,128>", "cb<64,192,8,2,0,0,128>"]),
    # ---- EncoderLayer row tiles.  64 rows: enc3 4 tiles (last 52), enc5 2 (last 58), the attention layers one partial tile of 61;
    # no chain fits a 64-row tile.  DHW_CHAIN=0 handles: every half as its own launch
    _case("enc_bm64_L488", 488, handle={"DHW_CHAIN": "0"}, launch={"DHW_ENC_BM": "64"}, expect=["a<192,64>", "bc<192,64,0>", "a<256,64>", "bc<256,64,0>", "a<384,32>", "bc<384,32,0>",   # (d = 384 on 64 rows exceeds LDS: enc_plan_bm halves it)
                                                                                              "cb<64,192,8,1,0,0,128>", "cb<32,256,8,1,0,0,192,2>"]),
    _case("enc_bm32_nochain_L488", 488, handle={"DHW_CHAIN": "0"}, launch={"DHW_ENC_BM": "32"}, expect=["a<192,32>", "bc<192,32,0>", "a<256,32>", "bc<256,32,0>", "a<384,32>", "bc<384,32,0>"]),
    _case("enc_nochain_L488", 488, handle={"DHW_CHAIN": "0"}, expect=_EL_NOCHAIN + ["cb<64,192,8,1,0,0,128>", "cb<32,256,8,1,0,0,192,2>"]),
    # chained 32-row attention-layer tiles (mode 1) behind enc5's mode 2, four layers: L/8 = 61 = 32 + 29
    _case("enc_bm32_nl4_L488", 488, nl=4, launch={"DHW_ENC_BM384": "32"}, expect=["bc<256,32,2>", "bc<384,32,1>", "bc<384,32,0>"]),
    # ---- handles without the fused decoder input stage: the run-time-width ConvBlocks (their input width is not an encoder's)
    _case("noup_L488", 488, handle={"DHW_FUSE_UP": "0"}, expect=["cb<48,256,8>", "cb<64,192,8>", "cb<64,128,8>"]),
    _case("noup_wgs2_L488", 488, handle={"DHW_FUSE_UP": "0"}, launch={"DHW_CONV_WGS": "2"}, expect=["cb<64,256,8>", "cb<64,192,8>", "cb<128,128,8>"]),
    _case("noup_bm32_L208", 208, handle={"DHW_FUSE_UP": "0"}, launch={"DHW_CONV_BM": "32"}, expect=["cb<32,256,8>"]),
    # ---- one launch per GEMM + stand-alone attention (gemm.hip, attn.hip): every intermediate is a tap
    _case("unfused_L208", 208, B=3, Lt=40, pad=11, handle={"DHW_FUSE": "0"}, expect=[]),
    # ---- frozen switches: child processes (group = the static environment)
    _case("cc3_L208", 208, B=3, static={"DHW_CHAIN_CONV": "3"}, expect=["cb<64,192,8,1,0,1,128>", "cb<48,256,8,1,0,1,192>"]),
    _case("cc3_wgs2_L488", 488, launch={"DHW_CONV_WGS": "2"}, static={"DHW_CHAIN_CONV": "3"}, expect=["cb<64,192,8,1,0,1,128>", "cb<64,256,8,1,0,1,192>"]),
    _case("cc0_L488", 488, static={"DHW_CHAIN_CONV": "0"}, expect=["cb<64,192,8,1,0,0,128>", "cb<32,256,8,1,0,0,192,2>", "a<192,32>", "a<256,32>"]),
    _case("cc1_noasym_notight_L488", 488, static={"DHW_CHAIN_CONV": "1", "DHW_CONV_ASYM": "0", "DHW_CONV_TIGHT": "0"},
          expect=["cb<64,192,8,1,0,1,128>", "cb<48,256,8,1,0,0,192>", "cb<48,256,8,1,384,0,384>"]),
    _case("cc1_notight_wgs2_L488", 488, launch={"DHW_CONV_WGS": "2"}, static={"DHW_CHAIN_CONV": "1", "DHW_CONV_ASYM": "0", "DHW_CONV_TIGHT": "0"},
          expect=["cb<128,128,8,1,192,0,192>"]),
    _case("cc2_rt_L488", 488, static={"DHW_CHAIN_CONV": "2", "DHW_CONV_RT": "1"}, expect=["cb<64,128,8>", "cb<64,192,8>", "cb<32,256,8,1,0,1,192,2>", "a<192,32>"]),
    _case("cc2_rt_wgs2_L488", 488, launch={"DHW_CONV_WGS": "2"}, static={"DHW_CHAIN_CONV": "2", "DHW_CONV_RT": "1"}, expect=["cb<128,128,8>", "cb<64,256,8,1,0,1,192>"]),
    # (DHW_GEMM_W8=0: the generic GEMM's other wave layout.  DHW_FLAT_TEXT=1 shares the child but acts on no forward: it is checked by
    # the group's sampling run, test_flat_text_switch_does_not_change_the_samples)
    _case("w8off_unfused_L208", 208, B=3, Lt=40, pad=11, handle={"DHW_FUSE": "0"}, static={"DHW_GEMM_W8": "0", "DHW_FLAT_TEXT": "1"}, expect=[]),
]


# ---- the run-time store-policy build (csrc/policy/*_policy.hip; ragged calls: the ragged build reading another word): handles
# created with DHW_STORE_POLICY = 0 (every class plain) / 42 (every class EARLY) at the shapes and switches of a base case.  The
# policy decides how a tile is stored, never what: same tiling, same `expect`, and the base case's bits
def _policy_case(base_id, word):
    b = next(c for c in CASES if c["id"] == base_id)
    return dict(b, id=f"pol{word}_{base_id}", handle=dict(b["handle"], DHW_STORE_POLICY=str(word)), base=base_id)


CASES += [_policy_case(b, w) for b, w in (("default_L488", 0), ("default_L488", 42), ("default_L208", 0), ("default_L208", 42),
                                          ("wgs2_L488", 0), ("wgs2_L488", 42), ("enc_bm64_L488", 0))]
CASE = {c["id"]: c for c in CASES}
SIGMAS = (0.25, 0.85, 0.55)   # one per sample

# the short sampling run of tests/test_gpu_parity.py::test_sampler_switches_do_not_change_the_samples
SAMPLE_SHAPE = dict(B=3, L=80, Lt=9, T=7, seed=12, pad=1)


# ---------------------------------------------------------------- the text-shape cases
# What the text side and the cross-attention compute depends on the prompt length Lt, the padded tail, the style rows S (S5 = 5 S keys
# of the style attention) and the handle's capacity (lpadT = pad32(max_Lt) is the row stride of V^T on the fp32 / generic paths; a
# loose handle leaves foreign prompts' rows behind the call's).  None of it depends on L: L = 64 keeps every block alive (8 rows at the
# bottleneck) and the float64 references cheap.  These cases are not run ragged and carry no `expect`.
TEXT_L = 64
FUSED_MAX_LT, FUSED_MAX_S = 32, 16   # textside_supported (csrc/textside.hip): above either the call runs the generic GEMM + attn.hip path
LOOSE_B, LOOSE_LT = 3, 24            # a loose handle: max_B = 3, max_Lt = Lt + 24

# (Lt, pad): 16-key tiles of the cross-attention fragments (15 | 16 | 17), the 32-key blocks of enc_a_tile - its prologue stages the
# first, attn_stage_kv every later one - (31 | 32 | 33, 63 | 64 | 65, 96 | 97: four blocks, the last with one key), the fused / generic
# switch at 32 | 33, one real token (31 / 30), a later block that is all padding (33 / 1, 64 / 32) or mostly (65 / 40)
LT_SWEEP = [(1, 0), (2, 1), (15, 0), (16, 3), (17, 0), (31, 30), (32, 0), (32, 5), (33, 0), (33, 1), (47, 0), (48, 9), (63, 0), (64, 0),
            (64, 32), (65, 0), (65, 40), (96, 7), (97, 0)]
TIGHT_LT = (1, 32, 33, 64, 65)       # these also run on a handle with no room behind the call's rows
# S: S5 = 5 S against the 10-row strides of the style staging (5 | 15 | 20 | 30 | 35 | 45 | 50), the 16-key tiles of its one-shot softmax
# (15 | 20: one or two tiles; 30 | 35: the odd third tile without a partner; 45 | 50, 60 | 65: the fourth, the odd fifth), the full
# 80 keys and the first generic count 85
S_SWEEP = (1, 3, 4, 6, 7, 9, 10, 12, 13, 16, 17)
S_SWEEP_AT = ((23, 3), (32, 0))
CORNERS = [(1, 1), (1, 16), (1, 17), (32, 16), (33, 16), (32, 17), (33, 17)]   # (Lt, S), pad 0
UNFUSED_ENVS = ({"DHW_FUSE_TEXT": "0"}, {"DHW_FUSE": "0"})                   # bf16 handles created with one of these
UNFUSED_EXTRA = [(16, 3, 14), (33, 0, 14), (64, 32, 14)]                     # (Lt, pad, S) beside the corners


# CHOSEN INPUTS.  With the synthetic weights both attentions of the text side are nearly uniform over their keys, so one key more or
# less moves an output row by ~1 / sqrt(keys) of the attention's share of it: a style key left out or a padded style row let in stays
# UNDER the bf16 bound of text_style_model (ratios 0.2 - 2.8), a text key left out of 65 reaches 5 x where 10 x is asked
# (tests/test_text_ref_cpu.py prints them).  The "peaky" weight set scales the query projections of the style attention and of every
# cross-attention, so that single keys carry rows, and the style attention's output projection, so that it weighs against the
# residual; "flat_last" style rows - every 256-wide style row of a sample equal to its first, except the last - make key S5 - 1 the one
# key that differs and give whole rows negative logits against every real key, which is where a zero-filled key takes over.
WEIGHT_SETS = {"peaky": {"text_style_model.mha.wq.weight": 6.0, "text_style_model.mha.dense.weight": 4.0, ".mha.wq.weight": 4.0}}
PEAKY_LT = [(32, 0), (33, 0), (33, 1), (64, 0), (64, 32), (65, 0)]   # (Lt, pad) under the peaky weights, S = 14


def state_dict_for(nl, weights=None):
    """spec.synthetic_state_dict(nl), with the tensors of WEIGHT_SETS[weights] scaled (a key that starts with "." names that tensor
    of every EncoderLayer)."""
    from dhg_amd import spec
    sd = dict(spec.synthetic_state_dict(nl))
    for k, f in (WEIGHT_SETS[weights] if weights else {}).items():
        for name in ([l + k for l in layer_names(nl)] if k.startswith(".") else [k]):
            sd[name] = (sd[name] * np.float32(f)).astype(np.float32)
    return sd


def _text_case(Lt, pad, S=14, tight=False, B=2, handle=None, weights=None, style=None):
    tag = "".join(f"_{k[4:].lower()}{v}" for k, v in sorted((handle or {}).items())) + (f"_{weights}" if weights else "") + (f"_{style}" if style else "")
    return _case(f"text_Lt{Lt}_pad{pad}_S{S}{'_B3' if B == 3 else ''}{'_tight' if tight else ''}{tag}", TEXT_L, B=B, Lt=Lt, pad=pad, handle=handle, S=S, tight=tight,
                 weights=weights, style=style)


def _text_cases():
    out = [_text_case(Lt, pad) for Lt, pad in LT_SWEEP] + [_text_case(Lt, pad, tight=True) for Lt, pad in LT_SWEEP if Lt in TIGHT_LT]
    out += [_text_case(Lt, pad, S) for Lt, pad in S_SWEEP_AT for S in S_SWEEP]
    out += [_text_case(Lt, 0, S) for Lt, S in CORNERS] + [_text_case(32, 0, 16, B=3)]
    for env in UNFUSED_ENVS:
        out += [_text_case(Lt, 0, S, handle=env) for Lt, S in CORNERS] + [_text_case(Lt, pad, S, handle=env) for Lt, pad, S in UNFUSED_EXTRA]
    out += [_text_case(23, 3, S, weights="peaky", style="flat_last") for S in S_SWEEP if S <= FUSED_MAX_S]
    out += [_text_case(Lt, pad, weights="peaky") for Lt, pad in PEAKY_LT]
    out = list({c["id"]: c for c in out}.values())   # ((32, 0) of the S sweep at S = 16 / 17 are corners too)
    return sorted(out, key=lambda c: (handle_key(c, ""), c["pad"], c["B"]))   # cases of one handle next to each other


def handle_caps(case):
    """(max_B, max_L, max_Lt) of the case's handle."""
    if case["tight"] is None:
        return MAX_B, MAX_L, MAX_LT
    return (case["B"], case["L"], case["Lt"]) if case["tight"] else (LOOSE_B, case["L"], case["Lt"] + LOOSE_LT)


def handle_key(case, prec):
    return (case["nl"], prec, tuple(sorted(case["handle"].items())), case["S"], handle_caps(case), case["weights"] or "")


def text_fused(case, prec):
    """Whether the call runs text_style_kernel / text_layer_kernel (else the generic GEMM + attn.hip text side)."""
    ha = case["handle"]
    return prec == "bf16" and ha.get("DHW_FUSE") != "0" and ha.get("DHW_FUSE_TEXT") != "0" and case["Lt"] <= FUSED_MAX_LT and case["S"] <= FUSED_MAX_S


TEXT_CASES = _text_cases()
TEXT_CASE = {c["id"]: c for c in TEXT_CASES}


# ---------------------------------------------------------------- row tiles per case and level, and the sample ends that probe them
# A level is the divisor of the stroke length: 1 (enc1, dec1), 2 (enc2, enc3, dec2), 4 (enc4, enc5, dec3), 8 (att_dense, att_layers).
# The tiles are the LIBRARY's answer: its tile plan (csrc/plan/tile_plan.h) is pure host logic behind dhw_debug_conv_plan /
# dhw_debug_enc_plan / dhw_debug_gemm_plan, asked here with the case's switches as explicit arguments - no device, no child process.
# The plan's inputs hold B and the PADDED L and no per-sample length, and the uniform, ragged and store-policy launchers all call
# it, so one answer holds for the uniform and the ragged launches alike.
LEVELS = (1, 2, 4, 8)
KEY_BLOCK = {"bf16": 64, "fp32": 32}   # self_kbs<T, DM, BM>() (csrc/enc_bc_core.h:45): 64 keys per block on bf16 handles, 32 on fp32 handles
PREC = {"bf16": 0, "fp32": 1}
# the ConvBlocks of the model per level: (name, Cin, Cout, width of the skip activation of the fused input stage)
CONV_BLOCKS = {1: (("enc1", 128, 128, 0), ("dec1", 192, 128, 128)), 2: (("enc2", 128, 192, 0), ("dec2", 256, 192, 192)), 4: (("enc4", 192, 256, 0), ("dec3", 384, 256, 256))}
ENC_WIDTH = {2: 192, 4: 256, 8: 384}   # enc3, enc5, att_layers


def _tiles(n, h):
    return -(-n // h)


def _forced(env, name):
    """A forced-tile switch as the library reads it: 0 = unset, else its value (-1 for a value that reads as 0)."""
    return 0 if env.get(name) is None else int(env[name]) or -1


def conv_knobs(case):
    """ConvKnobs {wgs, bm, occ, pp, asym, tight, rt} of a case: its launch switches and the ones its process is started with."""
    la, st = case["launch"], case["static"]
    return [int(la.get("DHW_CONV_WGS", 256)), _forced(la, "DHW_CONV_BM"), _forced(la, "DHW_CONV_OCC"), int(la.get("DHW_CONV_PP", 0)),
            int(st.get("DHW_CONV_ASYM", "1") != "0"), int(st.get("DHW_CONV_TIGHT", "1") != "0"), int(st.get("DHW_CONV_RT", "0") != "0")]


def enc_knobs(case, dm):
    la = case["launch"]
    return [int(la.get(f"DHW_ENC_BM{dm}", la.get("DHW_ENC_BM", 0))), int(la.get("DHW_ENC_WGS", 256))]


def conv_plan(prec, B, n, cin, cout, up_cin, chain, knobs):
    """The library's plan for one ConvBlock launch -> ([BM, CO, NW, OCC, UPC, CH, CIN, TIGHT, PP], output rows per tile), or None = refused."""
    import ctypes as C
    from dhg_amd import _lib
    out = (C.c_int * 12)()
    assert _lib.lib().dhw_debug_conv_plan(PREC[prec], B, n, cin, cout, up_cin, int(chain), (C.c_int64 * 7)(*knobs), out) == 0
    assert out[0] < 0 or out[1] == PREC[prec]
    return None if out[0] < 0 else (list(out[2:11]), out[11])


def enc_plan(prec, dm, B, n, bm_min, knobs):
    """The library's row tile for both halves of an EncoderLayer of width dm."""
    import ctypes as C
    from dhg_amd import _lib
    out = (C.c_int * 4)()
    assert _lib.lib().dhw_debug_enc_plan(PREC[prec], dm, B, n, bm_min, (C.c_int64 * 2)(*knobs), out) == 0 and out[0] >= 0
    return out[3]


def _gemm_rows(B, n, width, prec):
    """gemm_tile_for (csrc/gemm.hip): the row tile of the one-launch-per-GEMM path."""
    import ctypes as C
    from dhg_amd import _lib
    out = (C.c_int * 2)()
    assert _lib.lib().dhw_debug_gemm_plan(PREC[prec], B, n, width, width, 0, out) == 0
    return out[0]


def expect_args(v):
    """'cb<64,192,8,1,0,1,128>' -> ('cb', [64, 192, 8, 1, 0, 1, 128, 0, 0]) (trailing defaults filled in); a<...> / bc<...> as they are."""
    kind, args = v[:-1].split("<")
    a = [int(x) for x in args.split(",")]
    if kind == "cb":
        a += [1, 0, 0, 0, 0, 0][len(a) - 3:]
    return kind, a


def conv_chained(case, cout, prec="bf16"):
    """Whether the case's encoder block of width cout continues into the next EncoderLayer.  That is the launch sequence's decision (DHW_CHAIN,
    DHW_CHAIN_CONV, convblock_chain_auto: csrc/sampler/denoiser.cpp), which the `expect` list records.  A block the list does not
    name is asked unchained: the chained and the unchained plan of a shape differ in height only under DHW_CONV_RT, and both cases
    with that switch name their chained block."""
    return prec == "bf16" and any(k == "cb" and a[1] == cout and a[5] == 1 for k, a in map(expect_args, case["expect"]))


def conv_heights(case, prec="bf16"):
    """{level: set of OUTPUT rows per ConvBlock tile} (BMO = BM - 2 - 2 TIGHT, or BM for the asymmetric tiles, TIGHT = 2)."""
    B, L, ha = case["B"], case["L"], case["handle"]
    if ha.get("DHW_FUSE") == "0":
        return {lv: {_gemm_rows(B, L // lv, blocks[0][2], prec)} for lv, blocks in CONV_BLOCKS.items()}
    fused_up = prec == "bf16" and ha.get("DHW_FUSE_UP") != "0"   # (fp32 handles run the decoder's input stage as launches of its own)
    return {lv: {conv_plan(prec, B, L // lv, cin, cout, up if fused_up else 0, name.startswith("enc") and conv_chained(case, cout, prec), conv_knobs(case))[1]
                 for name, cin, cout, up in blocks} for lv, blocks in CONV_BLOCKS.items()}


def enc_bm_min(case, dm, prec="bf16"):
    """EncLayerParams.bm_min: 32 for enc5 where its second half continues into AvgPool + att_dense + att_layers.0.a (mode 2)."""
    return 32 if dm == 256 and prec == "bf16" and case["handle"].get("DHW_CHAIN") != "0" else 0


def enc_heights(case, prec="bf16"):
    """{level: set of rows per EncoderLayer tile} (the plan's row tile; the query tile of attn.hip and the GEMM tile on DHW_FUSE=0 handles)."""
    B, L, ha = case["B"], case["L"], case["handle"]
    if ha.get("DHW_FUSE") == "0":
        return {lv: {_gemm_rows(B, L // lv, dm, prec), 64} for lv, dm in ENC_WIDTH.items()}   # attn.hip: 64 query rows per workgroup
    return {lv: {enc_plan(prec, dm, B, L // lv, enc_bm_min(case, dm, prec), enc_knobs(case, dm))} for lv, dm in ENC_WIDTH.items()}


def tile_table(case, prec):
    """{level: sorted row-tile heights in use at that level} on a handle of precision prec."""
    tab = {lv: set() for lv in LEVELS}
    for d in (conv_heights(case, prec), enc_heights(case, prec)):
        for lv, hs in d.items():
            tab[lv] |= hs
    return {lv: sorted(hs) for lv, hs in tab.items()}


def expect_heights(case):
    """[(level, rows per tile)] of the bf16 instantiations in the case's ``expect`` list."""
    out = []
    for kind, a in map(expect_args, case["expect"]):
        if kind == "cb":
            out.append(({128: 1, 192: 2, 256: 4}[a[1]], a[0] if a[7] == 2 else a[0] - 2 - 2 * a[7]))
        else:
            out.append(({192: 2, 256: 4, 384: 8}[a[0]], a[1]))
    return out


def end_classes(case, prec, n):
    """The (level, tile height, class) triples a sample of n stroke rows realises in this case.  Lengths are multiples of 8, so the
    sample's end at level lv is e = n / lv, a multiple of g = 8 / lv.  With m0 = k h (k >= 1) a tile start:
      "a"  e = m0 < L / lv          the next tile exits early; the previous tile's lower halo rows lie past the end
      "b"  0 < e - m0 = the smallest such distance a multiple of g allows for this h (1 or 2 where g allows, never more than g):
           the tile holding the end has the minimum of valid rows
      "c"  m0 - e in {1, 2}         the x halo (2 rows), the h1 halo (1) and the up-stage halo straddle the end inside a live tile
      "d0" / "d1" / "d-1" at (level, KBS)   the self-attention key count n / lv leaves 0, 1 or KBS - 1 keys in the last key block."""
    out = set()
    for lv, hs in tile_table(case, prec).items():
        e, g, top = n // lv, 8 // lv, case["L"] // lv
        for h in hs:
            if e % h == 0 and e < top:
                out.add((lv, h, "a"))
            if e > h and e % h and e % h == _least_past(h, g, top):
                out.add((lv, h, "b"))
            if any((e + d) % h == 0 and e + d <= top for d in (1, 2)):
                out.add((lv, h, "c"))
        if lv > 1:
            kb = KEY_BLOCK[prec]
            if e % kb in (0, 1, kb - 1):
                out.add((lv, kb, "d%d" % (e % kb if e % kb < 2 else -1)))
    return out


def _least_past(h, g, top):
    d = [e - e // h * h for e in range(g, top + 1, g) if e > h and e % h]
    return min(d) if d else None


def wanted_classes(case, prec):
    """(realisable, unrealisable): every (level, tile height, class) triple of the case, split by whether ANY multiple of 8 in
    [8, L] realises it."""
    every = set()
    for lv, hs in tile_table(case, prec).items():
        every |= {(lv, h, c) for h in hs for c in "abc"}
        if lv > 1:
            every |= {(lv, KEY_BLOCK[prec], c) for c in ("d0", "d1", "d-1")}
    can = set()
    for n in range(8, case["L"] + 1, 8):
        can |= end_classes(case, prec, n)
    return can & every, every - can


# The LENGTH SETS of the ragged runs: (cases, precision, sets), each set one length per sample.  Chosen against the tile table of that
# precision's launches (a sample end only probes the tiling of the launch that runs it): the union of a case's sets realises every
# realisable class of end_classes() for every (level, tile height) of tile_table(), holds the extremes 8 and L, and every set has a
# sample shorter than L by more than the tallest full-resolution tile, so early-exit tiles exist
# (tests/test_block_ref_cpu.py::test_length_sets_cover_every_tile_class).  The lists are the smallest covers a search found: 8 - 11
# lengths where B = 2, hence up to six sets there.
_LENGTH_SETS = [
    (("default_L488", "enc_nochain_L488", "cc0_L488", "cc2_rt_L488"), "bf16", [[8, 184], [64, 248], [120, 256], [128, 480], [136, 488]]),
    (("default_L488", "wgs2_L488", "wgs2_pp1_L488", "wgs2_pp3_L488", "bm64_L488", "enc_bm64_L488", "enc_bm32_nochain_L488", "enc_nochain_L488",
      "enc_bm32_nl4_L488", "noup_L488", "noup_wgs2_L488", "cc3_wgs2_L488", "cc0_L488", "cc1_noasym_notight_L488", "cc1_notight_wgs2_L488",
      "cc2_rt_L488", "cc2_rt_wgs2_L488"), "fp32", [[8, 120], [56, 248], [64, 256], [88, 392], [112, 488]]),
    (("default_L208", "cc3_L208"), "bf16", [[8, 128, 184], [64, 136, 192], [104, 168, 200], [120, 176, 208]]),
    (("default_L208", "cc3_L208"), "fp32", [[8, 88, 128], [32, 104, 136], [56, 112, 200], [64, 120, 208]]),
    (("default_nl4",), "bf16", [[8, 64, 128], [16, 120, 136]]),
    (("default_nl4",), "fp32", [[8, 64, 120], [32, 88, 128], [56, 112, 136]]),
    (("wgs2_L488", "wgs2_pp1_L488", "wgs2_pp3_L488", "noup_wgs2_L488", "cc3_wgs2_L488", "cc1_notight_wgs2_L488", "cc2_rt_wgs2_L488"), "bf16",
     [[8, 248], [120, 256], [128, 376], [136, 480], [240, 488]]),
    (("wgs2_L504", "wgs2_pp2_L504"), "bf16", [[8, 248], [120, 256], [128, 376], [136, 496], [240, 504]]),
    (("wgs2_L504", "wgs2_pp2_L504"), "fp32", [[8, 120], [56, 128], [64, 256], [88, 392], [112, 504]]),
    (("wgs2_L128",), "bf16", [[8, 72, 120], [64, 112, 128]]),
    (("wgs2_L128",), "fp32", [[8, 64, 112], [32, 72, 120], [56, 88, 128]]),
    (("bm64_L488",), "bf16", [[8, 184], [64, 240], [120, 248], [128, 256], [136, 488]]),
    (("bm48_L368",), "bf16", [[8, 184], [64, 192], [120, 248], [128, 256], [136, 360], [176, 368]]),
    (("bm48_L368",), "fp32", [[8, 120], [32, 136], [56, 248], [64, 256], [88, 360], [112, 368]]),
    (("occ2_L208",), "bf16", [[8, 168], [64, 176], [120, 184], [128, 192], [136, 208]]),
    (("occ2_L208", "noup_bm32_L208"), "fp32", [[8, 112], [32, 120], [56, 128], [64, 136], [88, 208]]),
    (("enc_bm64_L488", "enc_bm32_nochain_L488", "enc_bm32_nl4_L488"), "bf16", [[8, 248], [64, 256], [120, 264], [128, 480], [184, 488]]),
    (("noup_L488", "cc1_noasym_notight_L488"), "bf16", [[8, 248], [64, 256], [136, 368], [176, 376], [184, 488]]),
    (("noup_bm32_L208",), "bf16", [[8, 128], [64, 136], [112, 184], [120, 208]]),
    (("unfused_L208", "w8off_unfused_L208"), "bf16", [[8, 128, 200], [104, 136, 208]]),
    (("unfused_L208", "w8off_unfused_L208"), "fp32", [[8, 128, 200], [120, 136, 208]]),
]
POLICY_SET = 1   # a store-policy case runs ONE of its base case's sets


def length_sets(case, prec):
    """The case's length sets on a handle of precision prec: [[length of sample 0, ...], ...]."""
    base = case.get("base", case["id"])
    sets = next(s for ids, p, s in _LENGTH_SETS if p == prec and base in ids)
    return [sets[POLICY_SET]] if "base" in case else sets


def static_group(case) -> str:
    return ",".join(f"{k}={v}" for k, v in sorted(case["static"].items()))


def static_groups():
    out = []
    for c in CASES:
        g = static_group(c)
        if g and g not in out:
            out.append(g)
    return out


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_MODELS = {}


def model_for(nl, prec, handle_env):
    """One handle per (depth, precision, create-time switches), shared by the cases."""
    import dhg_amd
    from dhg_amd import spec
    key = (nl, prec, tuple(sorted(handle_env.items())))
    if key not in _MODELS:
        m = dhg_amd.DiffusionModel(nl, precision=prec, max_B=MAX_B, max_L=MAX_L, max_Lt=MAX_LT).eval()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(nl).items()}, strict=True)
        with environ(handle_env):   # the handle is created by the first call
            i = spec.synthetic_inputs(1, 8, 2, seed=1)
            m(torch.from_numpy(i["strokes"]).cuda(), torch.from_numpy(i["text"]).cuda(), torch.full((1, 1), 0.5).cuda(), torch.from_numpy(i["style"]).cuda())
        _MODELS[key] = m
    return _MODELS[key]


_TEXT_MODEL = {}   # at most one handle of the text cases is alive: they are ordered by handle key


def text_model_for(case, prec):
    """The handle of a text case: one per (depth, precision, create-time switches, style rows, capacity), created at first use -
    by the first forward on it, under the case's handle switches - and kept until a case asks for another one."""
    import dhg_amd
    key = handle_key(case, prec)
    if key not in _TEXT_MODEL:
        for m in _TEXT_MODEL.values():
            m._destroy()
        _TEXT_MODEL.clear()
        mb, ml, mlt = handle_caps(case)
        m = dhg_amd.DiffusionModel(case["nl"], precision=prec, max_B=mb, max_L=ml, max_Lt=mlt, style_rows=case["S"]).eval()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict_for(case["nl"], case["weights"]).items()}, strict=True)
        _TEXT_MODEL[key] = m
    return _TEXT_MODEL[key]


def case_inputs(case):
    from dhg_amd import spec
    inp = spec.synthetic_inputs(case["B"], case["L"], case["Lt"], S=case["S"], seed=case.get("seed", 4000 + case["L"]), pad=case["pad"])
    inp.pop("noise")
    if case["style"] == "flat_last":   # every 256-wide style row of a sample equal to its first, except the last (WEIGHT_SETS)
        st = inp["style"].reshape(case["B"], case["S"] * 5, 256).copy()
        st[:, :-1] = st[:, :1]
        inp["style"] = st.reshape(inp["style"].shape)
    inp["sigma"] = np.array(SIGMAS[:case["B"]], np.float32).reshape(-1, 1)
    return inp


def tap_names(nl):
    n = ["sigma_ffn", "text_style_model", "text_style_model.style", "text_style_model.t2", "input_dense", "att_dense", "enc1.pool", "enc3.pool", "enc5.pool",
         "skip_conv3+up", "skip_conv2+up", "skip_conv1+up", "enc1", "enc2", "enc4", "dec3", "dec2", "dec1"]
    for l in ["enc3", "enc5"] + [f"att_layers.{i}" for i in range(nl)]:
        n += [l, l + ".x2", l + ".x3"]
    return n


TEXT_SIDE = ("sigma_ffn", "text_style_model", "text_style_model.style", "text_style_model.t2")   # no stroke length: checked by the uniform run


def run_case(case, prec, lengths=None):
    """One dhw_forward under the case's handle / launch switches -> {tap name: float32 array} + eps, pen.

    lengths (one per sample): the ragged call.  Immediately before it a UNIFORM forward at the case's B, L, Lt with NaN in every
    stroke row runs on the same handle, so every row of every stroke-path workspace buffer holds NaN - the rows the ragged call's
    early-exit tiles never touch included - and the ragged call's strokes are NaN past each sample's end: whatever a valid row reads
    from past its sample's end makes it NaN.  "poisoned" says that the uniform forward did come out all NaN.  The stroke-path taps
    of a ragged run are cut to the rows of its longest sample (rows past a sample's end are stale by design and never inspected);
    eps / pen stay whole (they are exactly 0 past each end)."""
    from dhg_amd import _lib
    m = model_for(case["nl"], prec, case["handle"])
    inp = case_inputs(case)
    tx, sg, sv = (torch.from_numpy(inp[k]).cuda() for k in ("text", "sigma", "style"))
    out = {}
    with environ(case["launch"]):
        if lengths is None:
            eps, pen, _ = m(torch.from_numpy(inp["strokes"]).cuda(), tx, sg, sv)
        else:
            assert len(lengths) == case["B"]
            e0, p0, _ = m(torch.full(inp["strokes"].shape, float("nan")).cuda(), tx, sg, sv)
            out["poisoned"] = np.array(bool(torch.isnan(e0).all() and torch.isnan(p0).all()))
            st = inp["strokes"].copy()
            for b, n in enumerate(lengths):
                st[b, n:] = np.nan
            eps, pen, _ = m(torch.from_numpy(st).cuda(), tx, sg, sv, lengths=list(lengths))
    out.update(eps=eps.cpu().numpy(), pen=pen.cpu().numpy())
    for name in tap_names(case["nl"]):
        try:
            a = m.debug_read(name).numpy()
        except _lib.DhwError:   # the call did not set this tap
            continue
        if lengths is not None and name not in TEXT_SIDE:
            a = a[:, :max(lengths) * a.shape[1] // case["L"]]
        out[name] = a
    return out


def layer_names(nl):
    return ["enc3", "enc5"] + [f"att_layers.{i}" for i in range(nl)]


LAYER_WIDTH = {"enc3": 192, "enc5": 256}   # att_layers.*: 384


def text_tap_names(nl):
    """The taps of a text case: every tap of tap_names() and the text keys / values of every EncoderLayer."""
    return tap_names(nl) + [l + s for l in layer_names(nl) for s in (".k1", ".v1")]


def values_as_rows(a, Lt, d, lpadT):
    """"<layer>.v1" as dhw_debug_read reports it -> (rows [B, Lt, d], the stored form).  The tap's shape says which form the handle
    keeps: rows [B, Lt, d] (fused bf16 EncoderLayer kernels) or V^T [B, d, lpadT], of which columns [0, Lt) belong to the call."""
    if tuple(a.shape[1:]) == (Lt, d):
        return a, "rows"
    assert tuple(a.shape[1:]) == (d, lpadT), (a.shape, Lt, d, lpadT)
    return np.ascontiguousarray(np.swapaxes(a[:, :, :Lt], 1, 2)), "vt"


def pad32(n):
    return (n + 31) // 32 * 32


def run_text_case(case, prec):
    """One dhw_forward of a text case -> {tap: float32 array} + eps, pen, with every "<layer>.v1" as rows [B, Lt, d].

    Immediately before it a forward at the HANDLE's max_B and max_Lt (the case's L) with a style tensor of NaN runs on the same
    handle: the style rows, hence the style attention's keys and values, hence every row of text_out and of every layer's k1 / v1
    - the rows behind the call's prompts and tokens included - hold NaN afterwards.  "poisoned" says that the poison call's
    text_style_model, k1 and v1 taps did come out all NaN.  Whatever the case's call reads from a row it did not write is NaN."""
    from dhg_amd import _lib
    m = text_model_for(case, prec)
    mb, _, mlt = handle_caps(case)
    nl, L, Lt = case["nl"], case["L"], case["Lt"]
    inp = case_inputs(case)
    out = {}
    with environ(case["handle"]):   # (the handle is created by the first call on it)
        m(torch.zeros(mb, L, 2).cuda(), torch.ones(mb, mlt, dtype=torch.int64).cuda(), torch.full((mb, 1), 0.5).cuda(),
          torch.full((mb, case["S"], 1280), float("nan")).cuda())
        nan = []
        for l in layer_names(nl):
            d = LAYER_WIDTH.get(l, 384)
            nan += [np.isnan(m.debug_read(l + ".k1").numpy()).all(), np.isnan(values_as_rows(m.debug_read(l + ".v1").numpy(), mlt, d, pad32(mlt))[0]).all()]
        nan.append(np.isnan(m.debug_read("text_style_model").numpy()).all())
        out["poisoned"] = np.array(all(nan))
        eps, pen, _ = m(*(torch.from_numpy(inp[k]).cuda() for k in ("strokes", "text", "sigma", "style")))
    out.update(eps=eps.cpu().numpy(), pen=pen.cpu().numpy())
    for name in text_tap_names(nl):
        try:
            a = m.debug_read(name).numpy()
        except _lib.DhwError:   # the call did not set this tap
            continue
        if name.endswith(".v1"):
            a, out[name + ".stored"] = values_as_rows(a, Lt, LAYER_WIDTH.get(name[:-3], 384), pad32(mlt))
        out[name] = a
    return out


# DHW_FLAT_TEXT only acts on the all-steps text plane of dhw_sample, and only where that plane runs through the generic GEMMs
# (gp_text, csrc/sampler/denoiser.cpp): the fp32 handles, and bf16 handles created with DHW_FUSE_TEXT=0
FLAT_TEXT_HANDLE = {"DHW_FUSE_TEXT": "0"}


def run_sample(prec, handle_env=None):
    """The short sampling run on a fresh handle created under handle_env -> samples [B, L, 3] as float32."""
    import dhg_amd
    from dhg_amd import spec
    s = SAMPLE_SHAPE
    inp = spec.synthetic_inputs(s["B"], s["L"], s["Lt"], seed=s["seed"], pad=s["pad"], T=s["T"])
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    m = dhg_amd.DiffusionModel(2, precision=prec, max_B=s["B"], max_L=s["L"], max_Lt=s["Lt"]).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}, strict=True)
    with environ(handle_env or {}):   # (the handle is created by the first call)
        return dhg_amd.sample(m, tx, sv, L=s["L"], T=s["T"], noise=nz).cpu().numpy()


def main():
    out_path, group = sys.argv[1], sys.argv[2]
    env = dict(kv.split("=") for kv in group.split(","))
    os.environ.update(env)   # before the library's first launch
    torch.set_num_threads(4)
    res = {}
    for c in CASES:
        if static_group(c) != group:
            continue
        for prec in ("fp32", "bf16"):
            for k, v in run_case(c, prec).items():
                res[f"{c['id']}/{prec}/{k}"] = v
            for r, lens in enumerate(length_sets(c, prec)):   # the ragged runs of the case, in the same child
                for k, v in run_case(c, prec, lens).items():
                    res[f"{c['id']}+r{r}/{prec}/{k}"] = v
    if sys.argv[3:] != ["cases-only"]:
        if list(env) == ["DHW_CHAIN_CONV"]:
            for prec in ("fp32", "bf16"):
                res[f"sample/{prec}"] = run_sample(prec)
        if env.get("DHW_FLAT_TEXT") == "1":
            for prec in ("fp32", "bf16"):
                res[f"sample_flat/{prec}"] = run_sample(prec, FLAT_TEXT_HANDLE)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
