"""Every sampler block, in every row-tile / chain / input-stage variant the launchers can select, against a float64 reference of
that ONE block evaluated on the inputs the launch itself read (tests/block_ref.py).  Runs on the MI355X only (-m gpu).

One test = one ``dhw_forward`` of a case of tests/blocks_worker.py (B = 2 or 3 with a different sigma per sample, L <= 512,
padded tokens) + float64 blocks at a few hundred rows.  For every block the device's own taps of the producing blocks are
the reference's inputs, so an error cannot hide behind - or be blamed on - what came before it.

Tolerances
  fp32 handles: the project's per-block bound TOL["fp32"]["tap"] = 5e-5 absolute (tests/test_gpu_parity.py).
  bf16 handles: measured against the reference's ROUNDING MODEL (block_ref: the same float64 arithmetic with bf16 rounding at
      the kernel's own store / staging points), never against the kernel: the worst per-row relative L2 error of the device
      output against the exact reference stays within FACTOR = 2 x the model's worst row for the same inputs, and
      max|err| / max|ref| within 2 x the model's.  Rows whose norm is below 1e-3 of the block's largest row norm are measured
      against that floor; at most 1 % of a block's rows may be such rows.
      Outputs that no bf16 value enters between input and output (sigma_ffn, the heads on the float32 dec1 activation) keep
      the absolute float32 bound in both precisions.
Every figure is printed before it is asserted (pytest -s): "BLOCKS <case> <prec> <tap> gpu_row model_row ratio gpu_max model_max ratio".

Ragged runs ("<case>+r<k>"): every case also runs with per-sample lengths - the ragged build, csrc/ragged/*_ragged.hip, in the same
tiling, because the launchers pick tiles from B and the padded L only - once per length set of BW.length_sets(), the lengths chosen
so that sample ends fall at, just past and just before tile starts and key blocks.  The contract is "row b computes what prompt b
computes alone at L = lengths[b]": the reference is evaluated PER SAMPLE on the taps cut to that sample's rows, the valid rows of
all samples are concatenated, and the measures and bounds above apply unchanged.  Before each ragged call a uniform all-NaN forward
fills every stroke-path workspace row with NaN, and the ragged call's strokes are NaN past each end: anything read from past a
sample's end into a valid row makes it NaN (0 x NaN does not hide).  Every valid row must be finite; eps / pen past each end are
exactly 0; taps past an end are stale by design and not inspected.  The store-policy cases ("pol<word>_<base case>") are also tied
bit for bit to their base case's default-policy run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_ref as R  # noqa: E402
import blocks_worker as BW  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_F32 = 5e-5     # tests/test_gpu_parity.py TOL["fp32"]["tap"]
FACTOR = 2.0       # device error / rounding-model error, per block and case
FLOOR_SHARE = 0.01
F32_EXACT = ("sigma_ffn", "eps", "pen")   # float32 arithmetic on float32 inputs on every handle

INPROC = [c for c in BW.CASES if not c["static"]]
STATIC = [c for c in BW.CASES if c["static"]]
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blocks_worker.py")

_WEIGHTS = {}


def weights(nl, prec, name=None):
    """The weights as a handle of precision prec holds them: the synthetic state dict, or a named set of BW.WEIGHT_SETS."""
    if (nl, prec, name) not in _WEIGHTS:
        _WEIGHTS[nl, prec, name] = R.Weights(BW.state_dict_for(nl, name), prec)
    return _WEIGHTS[nl, prec, name]


def _parts(case, got, lengths):
    """[(inputs, taps)] the references are evaluated on.  Uniform: the whole batch at once.  Ragged: one part PER SAMPLE b - the
    contract is "row b computes what prompt b computes alone at L = lengths[b]" - with every stroke-path tap cut to
    [b : b + 1, : lengths[b] >> level], the strokes to lengths[b] rows, and text, style and sigma the rows of sample b."""
    inp = {k: torch.from_numpy(v) for k, v in BW.case_inputs(case).items()}
    dev = {k: torch.from_numpy(np.asarray(v)).to(torch.float64) for k, v in got.items()}
    if lengths is None:
        return [(inp, dev)]
    parts = []
    for b, n in enumerate(lengths):
        d = {}
        for k, v in dev.items():
            if k in BW.TEXT_SIDE:
                d[k] = v[b:b + 1]
            elif k in ("eps", "pen"):
                d[k] = v[b:b + 1, :n]
            else:
                lv = max(lengths) // v.shape[1]   # (BW.run_case cut the tap to the longest sample's rows at its level)
                assert lv in BW.LEVELS and v.shape[1] * lv == max(lengths), (k, v.shape, lengths)
                d[k] = v[b:b + 1, :n // lv]
        i = {k: v[b:b + 1] for k, v in inp.items()}
        i["strokes"] = i["strokes"][:, :n]
        parts.append((i, d))
    return parts


def check_case(case, prec, got, lengths=None, tag=None):
    """got: {tap name: float32 array} of one dhw_forward.  Every block of the call against its float64 reference.  With lengths
    (a ragged call behind a NaN-poisoned workspace, BW.run_case): the stroke-path blocks per sample, the valid rows of all samples
    concatenated along the row axis under the SAME measures and bounds; every valid row finite; eps / pen exactly 0 past each end."""
    nl = case["nl"]
    W = weights(nl, prec, case["weights"])
    tag = tag or case["id"]
    ragged = lengths is not None
    if ragged:
        assert bool(got["poisoned"]), "the all-NaN uniform forward in front of the ragged call did not come out all NaN"
        for b, n in enumerate(lengths):
            assert not np.asarray(got["eps"])[b, n:].any() and not np.asarray(got["pen"])[b, n:].any(), (tag, b, "eps / pen past the end")
    parts = _parts(case, {k: v for k, v in got.items() if k != "poisoned"}, lengths)
    dev = parts[0][1]

    fused_up = "skip_conv3+up" not in dev
    names = R.block_names(nl)
    if not fused_up:
        names = names[:names.index("dec3")] + ["skip_conv3+up", "dec3", "skip_conv2+up", "dec2", "skip_conv1+up", "dec1", "heads"]
    seen, failures = set(), []

    def rows_of(t):   # [1 or B, rows, C] -> [rows, C]; pen [B, rows] -> [rows]
        return t.reshape(-1, t.shape[-1]) if t.dim() == 3 else t.reshape(-1)

    for name in names:
        if ragged and name in BW.TEXT_SIDE:
            continue
        refs = [R.block_output(W, name, d.__getitem__, i, R.exact, fused_up) for i, d in parts]
        models = [R.block_output(W, name, d.__getitem__, i, R.bf16_round, fused_up) for i, d in parts] if prec == "bf16" else None
        for key in refs[0]:
            if key not in dev:
                # sub-taps exist only where the launch writes them (`must` below names the cases in which it does)
                # (".k1" / ".v1", the layers' text keys and values, are read by the text cases only: BW.run_text_case)
                assert key.endswith((".x3", ".style", ".t2", ".k1", ".v1")), f"{tag}: the call left no tap '{key}'"
                continue
            seen.add(key)
            want = torch.cat([rows_of(r[key]) for r in refs])
            have = torch.cat([rows_of(d[key].reshape(r[key].shape)) for (_, d), r in zip(parts, refs)])
            assert torch.isfinite(have).all(), (tag, key, "a valid row is not finite")
            amax = (have - want).abs().max().item()
            if prec == "fp32" or key in F32_EXACT:
                print(f"BLOCKS {tag} {prec} {key} abs {amax:.3e}")
                if not amax <= TOL_F32:
                    failures.append((key, "abs", amax, TOL_F32))
                continue
            mod = torch.cat([rows_of(m[key].reshape(r[key].shape)) for m, r in zip(models, refs)])
            g_row, share = R.row_error(have, want)
            m_row, _ = R.row_error(mod, want)
            g_max, m_max = R.max_error(have, want), R.max_error(mod, want)
            print(f"BLOCKS {tag} {prec} {key} {g_row:.3e} {m_row:.3e} {g_row / m_row:.2f} {g_max:.3e} {m_max:.3e} {g_max / m_max:.2f} floor {share:.4f}")
            if not g_row <= FACTOR * m_row:
                failures.append((key, "row", g_row, m_row))
            if not g_max <= FACTOR * m_max:
                failures.append((key, "max", g_max, m_max))
            if not share <= FLOOR_SHARE:
                failures.append((key, "floor share", share, FLOOR_SHARE))
    # all 14 blocks of the existing tap test (+ the deeper model's layers), the pooled side outputs, the x2 sub-taps, the heads
    must = {"sigma_ffn", "text_style_model", "input_dense", "enc1", "enc2", "enc3", "enc4", "enc5", "att_dense", "dec3", "dec2", "dec1",
            "enc1.pool", "enc3.pool", "enc5.pool", "enc3.x2", "enc5.x2", "eps", "pen"} | {f"att_layers.{i}" for i in range(nl)} | {f"att_layers.{i}.x2" for i in range(nl)}
    # the sub-taps of the paths that write them: x3 is a buffer of the one-launch-per-GEMM EncoderLayer (DHW_FUSE=0 handles); the
    # FiLM'd style rows and t2 are buffers of the generic text side (fp32 handles, Lt > 32, DHW_FUSE=0 handles)
    unfused = case["handle"].get("DHW_FUSE") == "0"
    if unfused:
        must |= {"enc3.x3", "enc5.x3"} | {f"att_layers.{i}.x3" for i in range(nl)} | {"skip_conv3+up", "skip_conv2+up", "skip_conv1+up"}
    if unfused or prec == "fp32" or case["Lt"] > 32:
        must |= {"text_style_model.style", "text_style_model.t2"}
    if case["handle"].get("DHW_FUSE_UP") == "0" or prec == "fp32":
        must |= {"skip_conv3+up", "skip_conv2+up", "skip_conv1+up"}
    if ragged:
        must -= set(BW.TEXT_SIDE)   # (the text side has no stroke length: the uniform run of the case checks it)
    assert must <= seen, sorted(must - seen)
    assert not failures, (tag, prec, failures)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", INPROC, ids=[c["id"] for c in INPROC])
def test_every_block_matches_its_float64_reference(case, prec):
    check_case(case, prec, BW.run_case(case, prec))


def _ragged_params(cases):
    return [pytest.param(c, prec, r, id=f"{c['id']}+r{r}-{prec}") for c in cases for prec in ("fp32", "bf16") for r in range(len(BW.length_sets(c, prec)))]


@pytest.mark.parametrize("case,prec,r", _ragged_params(INPROC))
def test_every_block_of_a_ragged_call_matches_its_float64_reference_per_sample(case, prec, r):
    """The ragged build (csrc/ragged/*_ragged.hip) in the case's tiling, one length set: sample ends at, just past and just before
    tile starts and key blocks (BW.end_classes), behind a workspace poisoned with NaN."""
    lens = BW.length_sets(case, prec)[r]
    check_case(case, prec, BW.run_case(case, prec, lens), lens, f"{case['id']}+r{r}")


# ---------------------------------------------------------------- the text side and the cross-attention at every prompt / style edge
def _text_params():
    """(case, precision) ordered by handle, so that each handle is created once (BW.text_model_for keeps one alive).  Every case runs
    on a default bf16 handle - or the bf16 handle its switches name - and, the cases without switches, on an fp32 handle too."""
    ps = [(c, p) for c in BW.TEXT_CASES for p in (("bf16", "fp32") if not c["handle"] else ("bf16",))]
    return sorted(ps, key=lambda cp: (BW.handle_key(*cp), cp[0]["pad"], cp[0]["B"]))


@pytest.mark.parametrize("case,prec", [pytest.param(c, p, id=f"{c['id']}-{p}") for c, p in _text_params()])
def test_text_side_and_cross_attention_at_every_prompt_and_style_edge(case, prec):
    """BW.TEXT_CASES: prompt lengths around the 16-key tiles, the 32-key blocks and the fused / generic switch, style rows around the
    staging strides and the softmax tiles, loose and tight handles; every block of the call, the layers' text keys and values
    included, against float64 under the bounds of check_case - behind text-side buffers poisoned with NaN."""
    got = BW.run_text_case(case, prec)
    assert bool(got.pop("poisoned")), "the poison call's text_style_model / k1 / v1 taps did not come out all NaN"
    stored = {k[:-7]: got.pop(k) for k in [k for k in got if k.endswith(".stored")]}
    fused = BW.text_fused(case, prec)
    rows_kernels = prec == "bf16" and case["handle"].get("DHW_FUSE") != "0"   # the fused bf16 EncoderLayer kernels read v1 as rows
    layers = BW.layer_names(case["nl"])
    assert set(stored) == {l + ".v1" for l in layers} and set(stored.values()) == {"rows" if rows_kernels else "vt"}, (stored, fused)
    assert all(l + ".k1" in got for l in layers)
    # the generic text side writes the FiLM'd style rows and t2; the fused kernels keep them in LDS
    assert ("text_style_model.t2" in got) == (not fused) and ("text_style_model.style" in got) == (not fused), (sorted(got), fused)
    for k, v in got.items():
        assert np.isfinite(v).all(), (case["id"], prec, k, "not finite behind the poison")
    check_case(case, prec, got)


POLICY = [c for c in INPROC if "base" in c]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", POLICY, ids=[c["id"] for c in POLICY])
def test_store_policy_build_stores_the_bits_of_the_default_build(case, prec):
    """The policy decides how tiles are stored, never what: every tap the base case shares, uniform and ragged, bit for
    bit against the base case's default-policy run in this process (ragged: the valid rows; eps / pen whole)."""
    base = BW.CASE[case["base"]]
    for lens in (None, BW.length_sets(case, prec)[0]):
        a, b = BW.run_case(base, prec, lens), BW.run_case(case, prec, lens)
        shared = (set(a) & set(b)) - {"poisoned"}
        assert {"input_dense", "enc1", "enc1.pool", "enc2", "enc3", "enc3.x2", "enc4", "enc5", "enc5.pool", "att_dense", "att_layers.0", "att_layers.1",
                "dec3", "dec2", "dec1", "eps", "pen", "text_style_model"} <= shared and set(a) == set(b), sorted(set(a) ^ set(b))
        for k in sorted(shared):
            if lens is None or k in BW.TEXT_SIDE or k in ("eps", "pen"):
                assert np.array_equal(a[k], b[k]), (case["id"], prec, lens, k)
                continue
            lv = max(lens) // a[k].shape[1]
            for s, n in enumerate(lens):
                assert np.array_equal(a[k][s, :n // lv], b[k][s, :n // lv]), (case["id"], prec, lens, k, s)


# ---------------------------------------------------------------- switches frozen at first use: fresh child processes
_CHILD = {}      # group -> ("ok", results) or ("failed", what happened): every group's child is started at most once
_ABNORMAL = []   # set by the first child that faulted, aborted or ran into its time limit: no further child is started


def child_results(group, tmp_path_factory):
    """The worker's results for one static environment.  One child process per group, one at a time, started ONCE whatever its
    outcome: a failure is recorded and every later test of the group fails from the record without starting anything.  After a
    child that did not end by itself with a Python-level status (killed by a signal - fault, abort, segmentation fault - or by its
    time limit) no other group's child is started either: what has faulted or hung on the device is not followed by more work on it.
    The six-children cap counts launches, not successes."""
    if group not in _CHILD:
        if _ABNORMAL:
            _CHILD[group] = ("failed", f"not started: the child of group {_ABNORMAL[0]}")
        else:
            assert len(_CHILD) < 6, "at most six child processes per module"
            out = str(tmp_path_factory.mktemp("blocks") / "taps.npz")
            env = {k: v for k, v in os.environ.items() if not k.startswith("DHW_")}
            _CHILD[group] = ("failed", "the child was started and left no record")   # (stands if anything below raises)
            try:
                r = subprocess.run([sys.executable, WORKER, out, group], env=env, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired as e:
                _ABNORMAL.append(f"{group!r} ran into its time limit")
                _CHILD[group] = ("failed", f"time limit of {e.timeout:.0f} s; stderr: {(e.stderr or b'')[-2000:]!r}")
            else:
                if r.returncode == 0:
                    with np.load(out) as z:
                        _CHILD[group] = ("ok", {k: z[k] for k in z.files})
                else:
                    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                        _ABNORMAL.append(f"{group!r} ended with status {r.returncode}")
                    _CHILD[group] = ("failed", f"exit status {r.returncode}; stdout: {r.stdout[-2000:]}; stderr: {r.stderr[-4000:]}")
    state, value = _CHILD[group]
    assert state == "ok", (group, value)
    return value


def test_static_groups_fit_six_children():
    assert len(BW.static_groups()) <= 6, BW.static_groups()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", STATIC, ids=[c["id"] for c in STATIC])
def test_every_block_under_a_frozen_switch_matches_its_float64_reference(case, prec, tmp_path_factory):
    res = child_results(BW.static_group(case), tmp_path_factory)
    pre = f"{case['id']}/{prec}/"
    check_case(case, prec, {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)})


@pytest.mark.parametrize("case,prec,r", _ragged_params(STATIC))
def test_every_block_of_a_ragged_call_under_a_frozen_switch_matches_its_float64_reference_per_sample(case, prec, r, tmp_path_factory):
    """The ragged runs of the frozen-switch cases, from the SAME child of their group (the worker adds them to its .npz)."""
    res = child_results(BW.static_group(case), tmp_path_factory)
    pre = f"{case['id']}+r{r}/{prec}/"
    check_case(case, prec, {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}, BW.length_sets(case, prec)[r], f"{case['id']}+r{r}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_chain_switch_does_not_change_the_samples(prec, tmp_path_factory):
    """The conv_chain / no_conv_chain comparisons of test_gpu_parity.py::test_sampler_switches_do_not_change_the_samples, run where the
    switch takes effect: DHW_CHAIN_CONV is function-static in stroke_path (csrc/sampler/denoiser.cpp), so the first launch of a
    process freezes it and a handle created later under another value computes the default's outputs.  Same shapes, same assertion,
    same tolerance: fused vs unfused block kernels round intermediates to bf16 at different points; |x| reaches ~9 after these 7
    steps (<= 0.03 for every pair of the in-process switches; these two measure 0)."""
    default = torch.from_numpy(BW.run_sample(prec))          # this process: no DHW_CHAIN_CONV (enc2 -> enc3.a, enc4 -> enc5.a where it pays)
    tol = 1e-4 if prec == "fp32" else 0.06
    for name, group in (("conv_chain", "DHW_CHAIN_CONV=3"), ("no_conv_chain", "DHW_CHAIN_CONV=0")):
        other = torch.from_numpy(child_results(group, tmp_path_factory)[f"sample/{prec}"])
        assert torch.isfinite(other).all() and other.shape == default.shape
        d = (default - other).abs().max().item()
        print(f"BLOCKS sample {prec} {name} {d:.3e}")
        assert d < tol, (name, d)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_flat_text_switch_does_not_change_the_samples(prec, tmp_path_factory):
    """DHW_FLAT_TEXT=1 (function-static in gp_text, csrc/sampler/denoiser.cpp): the row-local GEMMs of the all-steps text plane see each
    sampler step as one long sample of B * Lt rows under one FiLM row, so their 64-row tiles run across prompts.  Only dhw_sample
    reaches it, and only where the plane runs through the generic GEMMs: fp32 handles, and bf16 handles created with DHW_FUSE_TEXT=0.
    The child's samples (with DHW_GEMM_W8=0 beside it, the other switch of its group) against this process's samples on a handle
    created the same way: the same per-row arithmetic in another tiling, so the bound of the other evaluation-order switches holds
    (test_gpu_parity.py::test_sampler_switches_do_not_change_the_samples: 1e-4 in fp32, 0.06 in bf16 at |x| ~ 9 after 7 steps)."""
    here = torch.from_numpy(BW.run_sample(prec, BW.FLAT_TEXT_HANDLE))
    group = next(g for g in BW.static_groups() if "DHW_FLAT_TEXT=1" in g.split(","))
    other = torch.from_numpy(child_results(group, tmp_path_factory)[f"sample_flat/{prec}"])
    assert torch.isfinite(other).all() and other.shape == here.shape
    d = (here - other).abs().max().item()
    print(f"BLOCKS sample {prec} flat_text {d:.3e}")
    assert d < (1e-4 if prec == "fp32" else 0.06), d


def test_dec1_tap_is_refused_when_the_heads_are_fused_into_dec1():
    """In the sampling loop dec1 evaluates the heads from its fp32 tile in LDS and writes no activation (conv_block: q.out = nullptr);
    the tap must not name the buffer nobody wrote.  A forward on the same handle sets it again."""
    import dhg_amd
    from dhg_amd import _lib, spec
    m = BW.model_for(2, "bf16", {})
    inp = spec.synthetic_inputs(2, 64, 5, seed=3, T=2)
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    out = dhg_amd.sample(m, tx, sv, L=64, T=2, noise=nz)
    assert torch.isfinite(out).all()
    with pytest.raises(_lib.DhwError, match="no activation named dec1"):
        m.debug_read("dec1")
    m(torch.from_numpy(inp["strokes"]).cuda(), tx, torch.full((2, 1), 0.5).cuda(), sv)
    assert m.debug_read("dec1").shape == (2, 64, 128)
