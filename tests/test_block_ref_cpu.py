"""CPU tests of tests/block_ref.py, the float64 per-block references behind tests/test_gpu_blocks.py:
  * every block reproduces the fp32 oracle (oracle/ref_cpu.py) from the oracle's own taps;
  * the bf16 rounding helper is torch.bfloat16's rounding, ties and denormals included;
  * the bound table: the rounding model's error against the exact reference, per block, at the shapes of the GPU cases;
  * the bound discriminates: wrong variants of a block (what a subtly broken kernel computes) exceed the GPU bound -
    FACTOR x the rounding model's worst row - by at least 10 x in the per-row measure;
  * the case table of tests/blocks_worker.py, the traced list profiles/block_variants.txt and the instantiations named in
    convblock_init() / enclayer_init() agree.
"""
import os
import re
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
    """The bf16 instantiations convblock_init() / enclayer_init() name (fits() / has_chain() decide which EncoderLayer ones exist)."""
    csrc = os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc")
    src = open(os.path.join(csrc, "convblock.hip")).read()
    body = src[src.index("hipError_t convblock_init()"):src.index("#undef A")]
    out = {_norm("cb", m.split(",")) for m in re.findall(r"A\(bf16_t,\s*([0-9,\s]+)\)", body)}
    src = open(os.path.join(csrc, "enclayer.hip")).read()
    body = src[src.index("hipError_t enclayer_init()"):src.index("bool enclayer_supported")]
    for dm, bm in re.findall(r"attr<bf16_t,\s*(\d+),\s*(\d+)>", body):
        dm, bm = int(dm), int(bm)
        out |= {f"a<{dm},{bm}>", f"bc<{dm},{bm},0>"}
        if dm == 384 and bm <= 32:
            out.add(f"bc<{dm},{bm},1>")     # has_chain(1)
        if dm == 256 and bm == 32:
            out.add(f"bc<{dm},{bm},2>")     # has_chain(2)
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
    """A tripwire: compiled_in() reads the init lists with regular expressions and restates has_chain() by hand, and the traced file
    is a recording.  When a kernel instantiation is added or removed, or has_chain() / fits() change, this fails by design."""
    remedy = ("profiles/block_variants.txt is a RECORDING: do not edit it or the sets here to match.  Add a case that selects the new "
              "instantiation to tests/blocks_worker.py (or an entry with its reason to UNREACHED), trace tests/test_gpu_blocks.py on the "
              "GPU again and regenerate the file with tools/block_variants.py (usage in its docstring); if has_chain() / fits() "
              "changed, bring compiled_in() in line with csrc/enclayer.hip.")
    table = {v for c in BW.CASES for v in c["expect"]}
    got = {v for v in traced() if v.startswith(("cb<", "a<", "bc<"))}
    assert table == got, ("case table vs traced list", sorted(table - got), sorted(got - table), remedy)
    comp = compiled_in()
    assert len(comp) >= 45, remedy
    assert comp - got == set(UNREACHED), ("named in convblock_init() / enclayer_init() but not traced", sorted(comp - got), remedy)
    assert got <= comp, ("traced but not named in the init lists", sorted(got - comp), remedy)


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
