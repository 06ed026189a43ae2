"""Ragged batches: prompts of different stroke lengths in one call (``sample(..., lengths=)``, ``forward(..., lengths=)``,
``infer_batch``, the C-ABI's dhw_forward_ragged / dhw_sample_ragged).  Runs on the MI355X only (-m gpu).

Contract: row b equals prompt b alone at L = lengths[b] (first_sample + b; external noise noise[:, b, :lengths[b]]); every
output past lengths[b] is exactly 0; inputs there are ignored, NaN included; all lengths == L is bit-identical to the uniform
call.  Tolerances are the suite's (tests/test_gpu_parity.py): fp32 forward 2e-5, fp32 trajectory 1e-3 with identical rounded
pen bits; bf16 forward 2e-2 (eps) / 5e-3 (pen), bf16 trajectory 2 % of max|x|.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [8, 488, 136, 64, 248, 16, 488, 200]
TOKENS = [1, 30, 8, 3, 15, 1, 29, 12]   # prompt b has TOKENS[b] tokens, padded with 0 to 30
_MODELS = {}


def _sd(nl, c2=192):
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(nl, c2=c2).items()}


def _model(prec, nl=2, c2=192, B=8, L=488, Lt=30):
    key = (prec, nl, c2, B, L, Lt)
    if key not in _MODELS:
        m = dhg_amd.DiffusionModel(nl, c2=c2, precision=prec, max_B=B, max_L=L, max_Lt=Lt).eval()
        m.load_state_dict(_sd(nl, c2), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def _mixed_inputs(seed=5, T=60):
    inp = spec.synthetic_inputs(len(LENS), max(LENS), max(TOKENS), seed=seed, T=T)
    for b, n in enumerate(TOKENS):
        inp["text"][b, n:] = 0
    return inp


def _alone_text(inp, b):
    return torch.from_numpy(inp["text"][b:b + 1, :TOKENS[b]].copy()).cuda()


def _cuda(*arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def _fwd(m, strokes, text, sigma, style, lengths=None):
    with torch.no_grad():
        kw = {} if lengths is None else {"lengths": lengths}
        eps, pen, _ = m(strokes, text, sigma, style, **kw)
    return eps.cpu().numpy(), pen.cpu().numpy()


# ---------------------------------------------------------------- 1. uniform lengths == the uniform call, bit for bit
@pytest.mark.parametrize("B,L,Lt", [(5, 136, 7), (64, 488, 30)])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_uniform_lengths_are_bit_identical(prec, B, L, Lt):
    m = _model(prec, B=64, L=488, Lt=30)
    T = 3
    inp = spec.synthetic_inputs(B, L, Lt, seed=11, pad=2, T=T)
    tx, sv, st, nz = _cuda(inp["text"], inp["style"], inp["strokes"], inp["noise"])
    lens = [L] * B
    for mode in ("new", "standard"):
        for noise in (None, nz):
            a = dhg_amd.sample(m, tx, sv, L=L, T=T, diffusion_mode=mode, noise=noise, seed=3).cpu()
            b = dhg_amd.sample(m, tx, sv, T=T, diffusion_mode=mode, noise=noise, seed=3, lengths=lens).cpu()
            assert torch.equal(a, b), (mode, noise is None)
    sg = torch.linspace(0.1, 0.9, B).reshape(B, 1).cuda()
    e0, p0 = _fwd(m, st, tx, sg, sv)
    e1, p1 = _fwd(m, st, tx, sg, sv, lengths=torch.tensor(lens))
    assert np.array_equal(e0, e1) and np.array_equal(p0, p1)


# ---------------------------------------------------------------- 2. mixed lengths == the alone runs
def test_mixed_lengths_fp32_match_alone_runs():
    m = _model("fp32")
    inp = _mixed_inputs()
    tx, sv, st = _cuda(inp["text"], inp["style"], inp["strokes"])
    sg = torch.linspace(0.15, 0.95, len(LENS)).reshape(-1, 1).cuda()
    eps, pen = _fwd(m, st, tx, sg, sv, lengths=LENS)
    out = dhg_amd.sample(m, tx, sv, seed=9, lengths=LENS).cpu().numpy()
    assert out.shape == (8, 488, 3)
    worst = {"fwd": 0.0, "traj": 0.0}
    for b, n in enumerate(LENS):
        assert not eps[b, n:].any() and not pen[b, n:].any() and not out[b, n:].any()
        e1, p1 = _fwd(m, st[b:b + 1, :n].contiguous(), _alone_text(inp, b), sg[b:b + 1], sv[b:b + 1].contiguous())
        d = max(np.abs(eps[b, :n] - e1[0]).max(), np.abs(pen[b, :n] - p1[0]).max())
        assert d <= 2e-5, (b, d)
        worst["fwd"] = max(worst["fwd"], float(d))
        alone = dhg_amd.sample(m, _alone_text(inp, b), sv[b:b + 1].contiguous(), L=n, seed=9, first_sample=b).cpu().numpy()[0]
        d = np.abs(out[b, :n, :2] - alone[:, :2]).max()
        assert d <= 1e-3, (b, d)
        assert np.array_equal(np.round(out[b, :n, 2]), np.round(alone[:, 2])), b
        worst["traj"] = max(worst["traj"], float(d))
    print("largest fp32 difference from the alone runs:", worst)


def test_mixed_lengths_fp32_match_oracle():
    m = _model("fp32")
    T = 8
    inp = _mixed_inputs(seed=6, T=T)
    tx, sv, st, nz = _cuda(inp["text"], inp["style"], inp["strokes"], inp["noise"])
    sg = torch.linspace(0.2, 0.9, len(LENS)).reshape(-1, 1)
    eps, pen = _fwd(m, st, tx, sg.cuda(), sv, lengths=LENS)
    out = dhg_amd.sample(m, tx, sv, T=T, noise=nz, lengths=LENS).cpu().numpy()
    sd = _sd(2)
    for b, n in enumerate(LENS):
        text_b = torch.from_numpy(inp["text"][b:b + 1, :TOKENS[b]].copy())
        style_b = torch.from_numpy(inp["style"][b:b + 1])
        with torch.no_grad():
            e_ref, p_ref = ref_cpu.forward(sd, torch.from_numpy(inp["strokes"][b:b + 1, :n].copy()), text_b, sg[b:b + 1], style_b)
        assert np.abs(eps[b, :n] - e_ref.numpy()[0]).max() <= 2e-5, b
        assert np.abs(pen[b, :n] - p_ref.numpy()[0]).max() <= 2e-5, b
        if b in (0, 2, 4, 7):   # (the CPU oracle's 8-step trajectory at four lengths: 8, 136, 248, 200)
            ref, _ = ref_cpu.sample(sd, text_b, style_b, n, torch.from_numpy(inp["noise"][:, b:b + 1, :n].copy()), T=T)
            ref = ref.numpy()[0]
            assert np.abs(out[b, :n, :2] - ref[:, :2]).max() <= 1e-3, b
            assert np.array_equal(np.round(out[b, :n, 2]), np.round(ref[:, 2])), b


def test_mixed_lengths_bf16_track_fp32_alone_runs():
    m16, m32 = _model("bf16"), _model("fp32")
    inp = _mixed_inputs(seed=7)
    tx, sv, st = _cuda(inp["text"], inp["style"], inp["strokes"])
    sg = torch.linspace(0.15, 0.95, len(LENS)).reshape(-1, 1).cuda()
    eps, pen = _fwd(m16, st, tx, sg, sv, lengths=LENS)
    out = dhg_amd.sample(m16, tx, sv, seed=4, lengths=LENS).cpu().numpy()
    assert np.isfinite(out).all()
    for b, n in enumerate(LENS):
        e1, p1 = _fwd(m32, st[b:b + 1, :n].contiguous(), _alone_text(inp, b), sg[b:b + 1], sv[b:b + 1].contiguous())
        assert np.abs(eps[b, :n] - e1[0]).max() < 2e-2, b
        assert np.abs(pen[b, :n] - p1[0]).max() < 5e-3, b
        ref = dhg_amd.sample(m32, _alone_text(inp, b), sv[b:b + 1].contiguous(), L=n, seed=4, first_sample=b).cpu().numpy()[0]
        assert np.abs(out[b, :n, :2] - ref[:, :2]).max() < 0.02 * np.abs(ref[:, :2]).max(), b


# ---------------------------------------------------------------- 3. padding isolation
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_padding_rows_are_ignored_and_zero(prec):
    m = _model(prec)
    T = 3
    inp = _mixed_inputs(seed=8, T=T)
    tx, sv = _cuda(inp["text"], inp["style"])
    sg = torch.linspace(0.15, 0.95, len(LENS)).reshape(-1, 1).cuda()
    # a uniform call at the full length with large values first: the workspace then holds stale data
    big = torch.from_numpy(inp["strokes"] * 1e4).cuda()
    _fwd(m, big, tx, sg, sv)
    dhg_amd.sample(m, tx, sv, L=488, T=T, noise=torch.from_numpy(inp["noise"] * 1e4).cuda())
    st0, st1 = inp["strokes"].copy(), inp["strokes"].copy()
    nz0, nz1 = inp["noise"].copy(), inp["noise"].copy()
    for b, n in enumerate(LENS):
        st0[b, n:] = 0
        st1[b, n:] = np.nan
        nz0[:, b, n:] = 0
        nz1[:, b, n:] = np.nan
    e0, p0 = _fwd(m, *_cuda(st0, inp["text"]), sg, sv, lengths=LENS)
    e1, p1 = _fwd(m, *_cuda(st1, inp["text"]), sg, sv, lengths=LENS)
    o0 = dhg_amd.sample(m, tx, sv, T=T, noise=_cuda(nz0)[0], lengths=LENS).cpu().numpy()
    o1 = dhg_amd.sample(m, tx, sv, T=T, noise=_cuda(nz1)[0], lengths=LENS).cpu().numpy()
    assert np.array_equal(e0, e1) and np.array_equal(p0, p1) and np.array_equal(o0, o1)
    assert np.isfinite(o1).all() and np.isfinite(e1).all() and np.isfinite(p1).all()
    for b, n in enumerate(LENS):
        assert not e1[b, n:].any() and not p1[b, n:].any() and not o1[b, n:].any(), b


# ---------------------------------------------------------------- 4. one captured graph serves every set of lengths
def test_one_graph_serves_many_length_sets():
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=8, max_L=488, max_Lt=30).eval()
    m.load_state_dict(_sd(2), strict=True)
    inp = _mixed_inputs(seed=10, T=4)
    tx, sv = _cuda(inp["text"], inp["style"])
    A, B_ = LENS, [488, 8, 200, 16, 64, 488, 136, 248]
    got = [dhg_amd.sample(m, tx, sv, L=488, T=4, seed=2, lengths=x).cpu() for x in (A, B_, A)]
    _lib.lib().dhw_set_graph(m._handle, 0)
    try:
        eager = [dhg_amd.sample(m, tx, sv, L=488, T=4, seed=2, lengths=x).cpu() for x in (A, B_)]
    finally:
        _lib.lib().dhw_set_graph(m._handle, 1)
    assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1])
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[1])


# ---------------------------------------------------------------- 5. shard invariance
def test_shard_of_a_ragged_batch_equals_its_rows():
    m = _model("bf16")
    inp = _mixed_inputs(seed=12)
    tx, sv = _cuda(inp["text"], inp["style"])
    full = dhg_amd.sample(m, tx, sv, seed=5, lengths=LENS).cpu()
    shard = dhg_amd.sample(m, tx[3:8].contiguous(), sv[3:8].contiguous(), L=488, seed=5, first_sample=3, lengths=LENS[3:8]).cpu()
    assert torch.equal(shard, full[3:8])


# ---------------------------------------------------------------- 6. other widths and depths
@pytest.mark.parametrize("nl,c2", [(2, 96), (4, 192)])
def test_mixed_lengths_other_widths_and_depths(nl, c2):
    m = _model("fp32", nl=nl, c2=c2)
    inp = _mixed_inputs(seed=13, T=8)
    tx, sv, st = _cuda(inp["text"], inp["style"], inp["strokes"])
    sg = torch.linspace(0.15, 0.95, len(LENS)).reshape(-1, 1).cuda()
    eps, pen = _fwd(m, st, tx, sg, sv, lengths=LENS)
    out = dhg_amd.sample(m, tx, sv, T=8, seed=1, lengths=LENS).cpu().numpy()
    for b, n in enumerate(LENS):
        e1, p1 = _fwd(m, st[b:b + 1, :n].contiguous(), _alone_text(inp, b), sg[b:b + 1], sv[b:b + 1].contiguous())
        assert max(np.abs(eps[b, :n] - e1[0]).max(), np.abs(pen[b, :n] - p1[0]).max()) <= 2e-5, b
        alone = dhg_amd.sample(m, _alone_text(inp, b), sv[b:b + 1].contiguous(), L=n, T=8, seed=1, first_sample=b).cpu().numpy()[0]
        assert np.abs(out[b, :n, :2] - alone[:, :2]).max() <= 1e-3, b
        assert np.array_equal(np.round(out[b, :n, 2]), np.round(alone[:, 2])), b
        assert not out[b, n:].any()


# ---------------------------------------------------------------- 7. full size: the bench_ragged mix
def _bench_mix():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_ragged
    finally:
        sys.path.pop(0)
    return bench_ragged.mix()


def test_full_size_bf16_mix():
    tokens, lens = _bench_mix()
    B = len(lens)
    m = _model("bf16", B=64, L=488, Lt=30)
    inp = spec.synthetic_inputs(B, max(lens), max(tokens), seed=21, T=1)
    for b, n in enumerate(tokens):
        inp["text"][b, n:] = 0
    tx, sv = _cuda(inp["text"], inp["style"])
    a = dhg_amd.sample(m, tx, sv, seed=1, lengths=lens).cpu().numpy()
    b2 = dhg_amd.sample(m, tx, sv, seed=1, lengths=lens).cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b2)
    m32 = _model("fp32", B=8, L=488, Lt=30)
    for b in (0, 17, 40, 63):
        n = lens[b]
        pen = a[b, :n, 2]
        assert ((pen > 0) & (pen < 1)).all() and not a[b, n:].any()
        text_b = torch.from_numpy(inp["text"][b:b + 1, :tokens[b]].copy()).cuda()
        ref = dhg_amd.sample(m32, text_b, sv[b:b + 1].contiguous(), L=n, seed=1, first_sample=b).cpu().numpy()[0]
        assert np.abs(a[b, :n, :2] - ref[:, :2]).max() < 0.02 * np.abs(ref[:, :2]).max(), b


# ---------------------------------------------------------------- 8. errors at the C-ABI
def test_c_abi_rejects_bad_lengths_and_keeps_the_handle():
    m = _model("bf16")
    inp = spec.synthetic_inputs(2, 64, 4, seed=3, T=2)
    tx, sv, st = _cuda(inp["text"], inp["style"], inp["strokes"])
    sg = torch.full((2,), 0.5).cuda()
    out = torch.empty((2, 64, 3), device="cuda")
    eps, pen = torch.empty((2, 64, 2), device="cuda"), torch.empty((2, 64), device="cuda")
    ref = dhg_amd.sample(m, tx, sv, L=64, T=2, seed=1).cpu()
    dhg_amd.sample(m, tx, sv, L=64, T=2, seed=1)   # (make sure the handle exists at this size)
    l, h = _lib.lib(), m._handle
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad, what in (([8, 12], "lens[1] = 12"), ([0, 64], "lens[0] = 0"), ([64, 72], "lens[1] = 72"), (None, "NULL")):
        arr = (C.c_int32 * 2)(*bad) if bad else None
        rc = l.dhw_sample_ragged(h, tx.data_ptr(), sv.data_ptr(), 2, 64, 4, arr, 2, 0, None, 1, 0, out.data_ptr(), s)
        assert rc == -1 and what in l.dhw_last_error(h).decode()
        rc = l.dhw_forward_ragged(h, st.data_ptr(), tx.data_ptr(), sg.data_ptr(), sv.data_ptr(), 2, 64, 4, arr, eps.data_ptr(), pen.data_ptr(), s)
        assert rc == -1 and what in l.dhw_last_error(h).decode()
    assert torch.equal(dhg_amd.sample(m, tx, sv, L=64, T=2, seed=1).cpu(), ref)


def test_persistent_step_with_lengths_is_refused_or_correct():
    old = os.environ.get("DHW_PERSIST")
    os.environ["DHW_PERSIST"] = "1"
    try:
        m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=8, max_L=488, max_Lt=30).eval()
        m.load_state_dict(_sd(2), strict=True)
        inp = _mixed_inputs(seed=14, T=2)
        tx, sv = _cuda(inp["text"], inp["style"])
        dhg_amd.sample(m, tx[:1].contiguous(), sv[:1].contiguous(), L=8, T=1)   # handle created under the switch
    finally:
        if old is None:
            os.environ.pop("DHW_PERSIST")
        else:
            os.environ["DHW_PERSIST"] = old
    try:
        got = dhg_amd.sample(m, tx, sv, T=2, seed=3, lengths=LENS).cpu()
    except _lib.DhwError as e:
        assert e.code == -1 and "DHW_PERSIST" in str(e)
    else:
        ref = dhg_amd.sample(_model("bf16"), tx, sv, T=2, seed=3, lengths=LENS).cpu()
        assert torch.equal(got, ref)
    assert torch.isfinite(dhg_amd.sample(m, tx, sv, L=488, T=2, seed=3).cpu()).all()   # the handle still works


# ---------------------------------------------------------------- 9. end to end
def test_infer_batch_and_prompts_file_end_to_end(tmp_path):
    (tmp_path / "config.yml").write_text("training_args:\n  att_layers_num: 2\n  channels: 128\n  dropout: 0.0\n")
    torch.save({"state_dict": _sd(2)}, tmp_path / "checkpoint_100.pth")
    style = spec.synthetic_inputs(1, 8, 1, seed=9)["style"][0]
    np.save(tmp_path / "style.npy", style)
    prompts = ["Follow the White Rabbit", "Hi", "down the rabbit hole"]
    (tmp_path / "lines.txt").write_text("\n".join(prompts) + "\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--prompts-file", str(tmp_path / "lines.txt"), str(tmp_path / "style.npy"),
                        "--experiment-path", str(tmp_path), "--output", "page", "--seed", "3"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=3, max_L=392, max_Lt=24).eval()
    m.load_state_dict(_sd(2))
    sv = torch.from_numpy(style)[None].cuda()
    got = dhg_amd.infer_batch(prompts, sv, m, seed=3)
    tok = dhg_amd.Tokenizer()
    for i, p in enumerate(prompts):
        ids = torch.tensor([tok.encode(p)]).cuda()
        L = dhg_amd.stroke_length(ids.shape[1])
        ref = dhg_amd.sample(m, ids, sv, L=L, seed=3, first_sample=i).cpu().numpy()[0]
        assert got[i].shape == (L, 3) and np.array_equal(got[i], ref), i
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    for i in range(3):
        assert (tmp_path / f"page_{i}.png").stat().st_size > 0
