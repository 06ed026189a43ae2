"""The cases of tests/test_gpu_blocks.py, the code that runs one of them on the device, and - run as a script - the child
process for the cases whose library switch is frozen at first use.

A CASE is one ``dhw_forward`` at a shape and a set of switches; what comes back is every tap the call set (as float32 arrays,
exactly what ``dhw_debug_read`` returns) plus eps / pen.  Three kinds of switch:
  handle : read at dhw_create (DHW_FUSE, DHW_FUSE_UP, DHW_CHAIN, ...): set while the handle is created;
  launch : read at every launch (DHW_CONV_WGS, DHW_CONV_BM, DHW_CONV_PP, DHW_CONV_OCC, DHW_ENC_BM*, DHW_ENC_WGS): set around the call;
  static : function-static in the library (DHW_CHAIN_CONV, DHW_CONV_TIGHT, DHW_CONV_ASYM, DHW_CONV_RT, DHW_GEMM_W8, DHW_FLAT_TEXT):
           the first launch of the process freezes them, so such a case only means something in a process started with them.

    python tests/blocks_worker.py OUT.npz GROUP [cases-only]      runs every case of static group GROUP in both precisions (and, for the
                                                     DHW_CHAIN_CONV and DHW_FLAT_TEXT groups, the short sampling run of
                                                     test_conv_chain_switch_... / test_flat_text_switch_does_not_change_the_samples)
                                                     and writes OUT.npz

``expect`` lists the bf16 kernel instantiations the launchers select for the case (worked out from launch_convblock /
launch_convblock_chain in csrc/convblock.hip and pick_bm / launch_pair in csrc/enclayer.hip; profiles/block_variants.txt is the
traced list).  Notation: cb<BM,CO,NW,OCC,UPC,CH,CIN,TIGHT,PP> = convblock_kernel<bf16_t, ...> with trailing defaults dropped,
a<DM,BM> = enc_a_kernel, bc<DM,BM,NEXT> = enc_bc_kernel.
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

# the EncoderLayer launches of an unforced call at B <= 3, L <= 512 (pick_bm: every level has fewer than 256 tiles):
# enc2 continues into enc3.a, enc5.bc into AvgPool + att_dense + att_layers.0.a, every attention layer into the next one's first half
_EL_DEFAULT = ["bc<192,32,0>", "bc<256,32,2>", "bc<384,16,1>", "bc<384,16,0>"]
_EL_NOCHAIN = ["a<192,32>", "bc<192,32,0>", "a<256,16>", "bc<256,16,0>", "a<384,16>", "bc<384,16,0>"]


def _case(id, L, B=2, Lt=23, pad=3, nl=2, handle=None, launch=None, static=None, expect=()):
    return dict(id=id, B=B, L=L, Lt=Lt, pad=pad, nl=nl, handle=handle or {}, launch=launch or {}, static=static or {}, expect=list(expect))


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
    _case("enc_bm64_L488", 488, handle={"DHW_CHAIN": "0"}, launch={"DHW_ENC_BM": "64"}, expect=["a<192,64>", "bc<192,64,0>", "a<256,64>", "bc<256,64,0>", "a<384,32>", "bc<384,32,0>",   # (d = 384 on 64 rows exceeds LDS: pick_bm halves it)
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
CASE = {c["id"]: c for c in CASES}
SIGMAS = (0.25, 0.85, 0.55)   # one per sample

# the short sampling run of tests/test_gpu_parity.py::test_sampler_switches_do_not_change_the_samples
SAMPLE_SHAPE = dict(B=3, L=80, Lt=9, T=7, seed=12, pad=1)


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


def case_inputs(case):
    from dhg_amd import spec
    inp = spec.synthetic_inputs(case["B"], case["L"], case["Lt"], seed=4000 + case["L"], pad=case["pad"])
    inp.pop("noise")
    inp["sigma"] = np.array(SIGMAS[:case["B"]], np.float32).reshape(-1, 1)
    return inp


def tap_names(nl):
    n = ["sigma_ffn", "text_style_model", "text_style_model.style", "text_style_model.t2", "input_dense", "att_dense", "enc1.pool", "enc3.pool", "enc5.pool",
         "skip_conv3+up", "skip_conv2+up", "skip_conv1+up", "enc1", "enc2", "enc4", "dec3", "dec2", "dec1"]
    for l in ["enc3", "enc5"] + [f"att_layers.{i}" for i in range(nl)]:
        n += [l, l + ".x2", l + ".x3"]
    return n


def run_case(case, prec):
    """One dhw_forward under the case's handle / launch switches -> {tap name: float32 array} + eps, pen."""
    from dhg_amd import _lib
    m = model_for(case["nl"], prec, case["handle"])
    inp = case_inputs(case)
    with environ(case["launch"]):
        eps, pen, _ = m(*(torch.from_numpy(inp[k]).cuda() for k in ("strokes", "text", "sigma", "style")))
    out = {"eps": eps.cpu().numpy(), "pen": pen.cpu().numpy()}
    for name in tap_names(case["nl"]):
        try:
            out[name] = m.debug_read(name).numpy()
        except _lib.DhwError:   # the call did not set this tap
            pass
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
