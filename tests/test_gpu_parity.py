"""Parity of the HIP path (through the C-ABI library) against (a) the golden vectors captured from the
real reference and (b) the CPU oracle on seeded inputs.  Runs on the MI355X only (-m gpu).

Stated tolerances
  fp32 mode (exact-f32 MFMA): single forward 2e-5 abs on eps/pen (measured ~1e-6); 60-step trajectory
      1e-3 abs on |x| up to ~1e2 (measured ~6e-5); rounded pen bits identical to the reference.
  bf16 mode (bf16 weights + activations, fp32 accumulate / LayerNorm / softmax / sampler state):
      single forward 2e-2 abs on eps (|eps| ~ 1, measured ~4e-3), 5e-3 on pen; 60-step trajectory within
      2 % of max|x| (measured ~0.6 %); a rounded pen bit may differ only where the reference's own
      probability is within 0.02 of 0.5 (with these fixtures: no flips at all).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

# tap: absolute for fp32; for bf16 relative to the block output's own magnitude max|ref| (post-LayerNorm/FiLM outputs reach
# |x| ~ 3.6, where ONE bf16 ulp is 0.0156): 1.5e-2 * max|ref| = ~4 bf16 ulps.  Measured (tools/measure_parity.py, r2):
# 0.0033 .. 0.0097 * max|ref| over the 14 blocks.
TOL = {"fp32": dict(eps=2e-5, pen=2e-5, tap=5e-5), "bf16": dict(eps=2e-2, pen=5e-3, tap_rel=1.5e-2)}
_MODELS = {}


def _sd(nl):
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(nl).items()}


def get_model(nl, prec, S=14):
    key = (nl, prec, S)
    if key not in _MODELS:
        m = dhg_amd.DiffusionModel(nl, precision=prec, max_B=8, max_L=488, max_Lt=40, style_rows=S).eval()
        m.load_state_dict(_sd(nl), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def fwd(m, inp, sigma):
    eps, pen, none = m(torch.from_numpy(inp["strokes"]).cuda(), torch.from_numpy(inp["text"]).cuda(), sigma.cuda(),
                       torch.from_numpy(inp["style"]).cuda())
    assert none is None and eps.dtype == torch.float32 and pen.dtype == torch.float32
    return eps.cpu().numpy(), pen.cpu().numpy()


def test_native_library_is_loaded():
    l = _lib.lib()
    assert os.path.samefile(l._name, _lib.LIB_PATH)
    maps = open("/proc/self/maps").read()
    assert "libdhw_hip.so" in maps


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("fname,nl", [("fwd_main.npz", 2), ("fwd_pad.npz", 2), ("fwd_s1.npz", 2), ("fwd_nl4.npz", 4)])
def test_forward_matches_reference_golden(golden_dir, prec, fname, nl):
    g = np.load(os.path.join(golden_dir, fname))
    B, L, Lt, S = int(g["B"]), int(g["L"]), int(g["Lt"]), int(g["S"])
    m = get_model(nl, prec, S)
    inp = spec.synthetic_inputs(B, L, Lt, S=S, seed=int(g["seed"]), pad=int(g["pad"]))
    if "text" in g.files:
        inp["text"] = g["text"]
    alpha = dhg_amd.get_alpha_set()
    tol = TOL[prec]
    for i in (59, 30, 0):
        eps, pen = fwd(m, inp, torch.sqrt(alpha[i]) * torch.ones((B, 1, 1)))
        assert np.abs(eps - g[f"eps_i{i}"]).max() < tol["eps"]
        assert np.abs(pen - g[f"pen_i{i}"]).max() < tol["pen"]
    eps, pen = fwd(m, inp, torch.from_numpy(g["sigma_rand"]))   # per-row sigma, [B,1] as in training
    assert np.abs(eps - g["eps_rand"]).max() < tol["eps"]
    assert np.abs(pen - g["pen_rand"]).max() < tol["pen"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("c2", [48, 96, 24])
def test_other_model_widths_match_reference_golden(golden_dir, prec, c2):
    """The reference's constructor takes any c2 divisible by 12 (model.py:64-71; SURVEY's tiny case c = (128, 48, 256)): such a
    model is embedded into the c2 = 192 kernels with zero-padded channels (dhw_api.cpp pad_weights).  Fixtures: the real reference
    at that width (oracle/make_golden_c2.py): single forwards at three schedule points and per-row sigma, and a 6-step reverse loop."""
    g = np.load(os.path.join(golden_dir, f"fwd_c2_{c2}.npz"))
    B, L, Lt, T = int(g["B"]), int(g["L"]), int(g["Lt"]), int(g["T"])
    m = dhg_amd.DiffusionModel(2, 128, c2, 256, precision=prec, max_B=B, max_L=L, max_Lt=Lt).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2, 128, c2, 256).items()}, strict=True)
    inp = spec.synthetic_inputs(B, L, Lt, seed=int(g["seed"]), pad=int(g["pad"]), T=T)
    alpha = dhg_amd.get_alpha_set()
    tol = TOL[prec]
    for i in (59, 30, 0):
        eps, pen = fwd(m, inp, torch.sqrt(alpha[i]) * torch.ones((B, 1, 1)))
        assert np.abs(eps - g[f"eps_i{i}"]).max() < tol["eps"], i
        assert np.abs(pen - g[f"pen_i{i}"]).max() < tol["pen"], i
    eps, pen = fwd(m, inp, torch.from_numpy(g["sigma_rand"]))
    assert np.abs(eps - g["eps_rand"]).max() < tol["eps"]
    assert np.abs(pen - g["pen_rand"]).max() < tol["pen"]
    out = dhg_amd.sample(m, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=L, T=T,
                         noise=torch.from_numpy(inp["noise"]).cuda()).cpu().numpy()
    ref = g["loop_out"]
    xmax = np.abs(ref[..., :2]).max()
    assert np.abs(out[..., :2] - ref[..., :2]).max() < (1e-3 if prec == "fp32" else 0.02 * xmax)
    assert np.abs(out[..., 2] - ref[..., 2]).max() < (1e-4 if prec == "fp32" else 2e-2)
    # the oracle at the same width agrees too (it restates the reference for any constructor arguments)
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2, 128, c2, 256).items()}
    sg = torch.from_numpy(g["sigma_rand"])
    with torch.no_grad():
        e_o, p_o = ref_cpu.forward(sd, torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg, torch.from_numpy(inp["style"]))
    assert np.abs(e_o.numpy() - g["eps_rand"]).max() < 2e-5 and np.abs(p_o.numpy() - g["pen_rand"]).max() < 2e-5


def test_other_width_with_class_default_depth_matches_oracle():
    """c = (128, 60, 256) with num_layers = 4 (the class default depth, model.py:66) — a width no fixture covers (head dims 20 and 15)
    and ragged shapes — against the CPU oracle, which tests/test_oracle_golden.py pins to the reference at three other widths."""
    c2, nl, B, L, Lt = 60, 4, 3, 72, 7
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(nl, 128, c2, 256, seed=3).items()}
    m = dhg_amd.DiffusionModel(nl, 128, c2, 256, precision="fp32", max_B=B, max_L=L, max_Lt=Lt).eval()
    m.load_state_dict(sd, strict=True)
    inp = spec.synthetic_inputs(B, L, Lt, seed=77, pad=2)
    sg = torch.linspace(0.2, 0.9, B).reshape(B, 1)
    eps, pen = fwd(m, inp, sg)
    with torch.no_grad():
        e_o, p_o = ref_cpu.forward(sd, torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg, torch.from_numpy(inp["style"]))
    assert np.abs(eps - e_o.numpy()).max() < TOL["fp32"]["eps"] and np.abs(pen - p_o.numpy()).max() < TOL["fp32"]["pen"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_every_block_matches_reference_taps(golden_dir, prec):
    g = np.load(os.path.join(golden_dir, "taps.npz"))
    B, L, Lt = int(g["B"]), int(g["L"]), int(g["Lt"])
    m = get_model(2, prec)
    inp = spec.synthetic_inputs(B, L, Lt, seed=int(g["seed"]), pad=int(g["pad"]))
    alpha = dhg_amd.get_alpha_set()
    fwd(m, inp, torch.sqrt(alpha[int(g["sigma_index"])]) * torch.ones((B, 1, 1)))
    for name in ("sigma_ffn", "text_style_model", "input_dense", "enc1", "enc2", "enc3", "enc4", "enc5", "att_dense",
                 "att_layers.0", "att_layers.1", "dec3", "dec2", "dec1"):
        ref = g["tap_" + name]
        got = m.debug_read(name).numpy().reshape(ref.shape)
        tol = TOL[prec]["tap"] if prec == "fp32" else TOL[prec]["tap_rel"] * np.abs(ref).max()
        assert np.abs(got - ref).max() < tol, (name, np.abs(got - ref).max(), tol)
    if prec == "fp32":
        # the skip convolutions (model.py:169-175): the fp32 path keeps `Upsample(x) + skip_conv(h)` as its own launch and
        # exposes the sum; minus the up-sampled predecessor it is the reference's skip_conv module output
        for skip, prev in (("skip_conv3", "att_layers.1"), ("skip_conv2", "dec3"), ("skip_conv1", "dec2")):
            ref = g["tap_" + skip]
            up = np.repeat(m.debug_read(prev).numpy(), 2, axis=1)
            got = m.debug_read(skip + "+up").numpy().reshape(ref.shape) - up.reshape(ref.shape)
            assert np.abs(got - ref).max() < TOL["fp32"]["tap"], skip


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("fname,mode", [("loop_new.npz", "new"), ("loop_std.npz", "standard")])
def test_sampling_loop_matches_reference_golden(golden_dir, prec, fname, mode):
    g = np.load(os.path.join(golden_dir, fname))
    B, L, Lt = int(g["B"]), int(g["L"]), int(g["Lt"])
    m = get_model(2, prec)
    inp = spec.synthetic_inputs(B, L, Lt, seed=int(g["seed"]))
    out = dhg_amd.sample(m, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=L,
                         diffusion_mode=mode, noise=torch.from_numpy(inp["noise"]).cuda()).cpu().numpy()
    assert out.shape == (B, L, 3)
    ref = g["out"]
    xmax = np.abs(ref[..., :2]).max()
    err = np.abs(out[..., :2] - ref[..., :2]).max()
    bits = np.round(out[..., 2]).astype(np.uint8)
    if prec == "fp32":
        assert err < 1e-3
        assert np.abs(out[..., 2] - ref[..., 2]).max() < 1e-4
        assert np.array_equal(bits, g["pen_bits"])          # pen-lift decisions bit-exact after rounding
    else:
        assert err < 0.02 * xmax
        flipped = bits != g["pen_bits"]
        assert np.all(np.abs(ref[..., 2][flipped] - 0.5) < 0.02)
        assert flipped.sum() <= 0.02 * bits.size


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,L,Lt,pad", [(3, 72, 7, 2), (1, 8, 1, 0), (2, 64, 40, 39), (5, 200, 33, 0)])
def test_forward_matches_oracle_on_seeded_inputs(prec, B, L, Lt, pad):
    """Ragged / edge shapes: row tails inside tiles, the minimum L, a single token, an all-but-one padded text."""
    m = get_model(2, prec)
    inp = spec.synthetic_inputs(B, L, Lt, seed=100 + L, pad=pad)
    sg = torch.linspace(0.15, 0.95, B).reshape(B, 1)
    with torch.no_grad():
        e_ref, p_ref = ref_cpu.forward(_sd(2), torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg,
                                       torch.from_numpy(inp["style"]))
    eps, pen = fwd(m, inp, sg)
    assert np.abs(eps - e_ref.numpy()).max() < TOL[prec]["eps"]
    assert np.abs(pen - p_ref.numpy()).max() < TOL[prec]["pen"]


def test_fully_padded_text_row_matches_oracle():
    """All keys masked: the reference's additive -1e9 mask degenerates to uniform attention (attention.py:44)."""
    m = get_model(2, "fp32")
    B, L, Lt = 2, 32, 6
    inp = spec.synthetic_inputs(B, L, Lt, seed=77)
    inp["text"][1, :] = 0
    sg = torch.full((B, 1), 0.5)
    with torch.no_grad():
        e_ref, p_ref = ref_cpu.forward(_sd(2), torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg,
                                       torch.from_numpy(inp["style"]))
    eps, pen = fwd(m, inp, sg)
    assert np.isfinite(eps).all()
    assert np.abs(eps - e_ref.numpy()).max() < 5e-5 and np.abs(pen - p_ref.numpy()).max() < 5e-5


@pytest.mark.parametrize("mode", ["new", "standard"])
def test_short_sampling_matches_oracle_T_generalised(mode):
    """T != 60 exercises the T-generalised schedule (0.02 + explin(1e-5, 0.4, T))."""
    m = get_model(2, "fp32")
    B, L, Lt, T = 2, 40, 5, 9
    inp = spec.synthetic_inputs(B, L, Lt, seed=5, T=T)
    noise = torch.from_numpy(inp["noise"])
    ref, _ = ref_cpu.sample(_sd(2), torch.from_numpy(inp["text"]), torch.from_numpy(inp["style"]), L, noise, T=T, mode=mode)
    out = dhg_amd.sample(m, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=L, T=T,
                         diffusion_mode=mode, noise=noise.cuda()).cpu()
    assert (out - ref).abs().max().item() < 1e-4


def test_graph_replay_equals_eager_launches():
    m = get_model(2, "bf16")
    B, L, Lt = 4, 96, 9
    inp = spec.synthetic_inputs(B, L, Lt, seed=8)
    tx, sv = torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda()
    a = dhg_amd.sample(m, tx, sv, L=L, seed=42).cpu()
    a2 = dhg_amd.sample(m, tx, sv, L=L, seed=42).cpu()          # replay of the cached graph
    _lib.lib().dhw_set_graph(m._handle, 0)
    try:
        b = dhg_amd.sample(m, tx, sv, L=L, seed=42).cpu()
    finally:
        _lib.lib().dhw_set_graph(m._handle, 1)
    assert torch.equal(a, a2) and torch.equal(a, b)
    c = dhg_amd.sample(m, tx, sv, L=L, seed=43).cpu()
    assert not torch.equal(a, c) and torch.isfinite(c).all()


def test_full_size_batch_properties():
    """BASELINE configs[1] size (B=64, L=488, Lt=30): samples are independent (a prompt alone == inside the batch),
    device-side noise is keyed by the global sample index (shard-invariant), runs are deterministic and finite."""
    B, L, Lt = 64, 488, 30
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=Lt).eval()
    m.load_state_dict(_sd(2))
    inp = spec.synthetic_inputs(B, L, Lt, seed=1)
    tx, sv = torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda()
    full = dhg_amd.sample(m, tx, sv, L=L, seed=7).cpu()
    assert full.shape == (B, L, 3) and torch.isfinite(full).all()
    assert ((full[..., 2] > 0) & (full[..., 2] < 1)).all()
    again = dhg_amd.sample(m, tx, sv, L=L, seed=7).cpu()
    assert torch.equal(full, again)
    # shard [40, 48) on its own handle-call, as a second GPU would run it
    shard = dhg_amd.sample(m, tx[40:48].contiguous(), sv[40:48].contiguous(), L=L, seed=7, first_sample=40).cpu()
    assert torch.equal(shard, full[40:48])
    # (the device generator itself: tests/test_gpu_round2.py::test_device_noise_generator_moments_and_independence)
    # forward at full batch: batch independence of the denoiser
    sg = torch.full((B, 1), 0.7)
    e_full, p_full = fwd(m, inp, sg)
    sub = {k: v[10:12] for k, v in inp.items() if k != "noise"}
    e_sub, p_sub = fwd(m, sub, sg[10:12])
    assert np.array_equal(e_full[10:12], e_sub) and np.array_equal(p_full[10:12], p_sub)


def test_error_behaviour_mirrors_the_reference():
    m = get_model(2, "bf16")
    ok = spec.synthetic_inputs(1, 16, 3, seed=1)
    with pytest.raises(ValueError):      # T % 8 != 0 mis-sizes the skip additions in the reference (model.py:169-175)
        m(torch.zeros(1, 12, 2).cuda(), torch.from_numpy(ok["text"]).cuda(), torch.ones(1, 1).cuda(),
          torch.from_numpy(ok["style"]).cuda())
    with pytest.raises(ValueError):
        dhg_amd.sample(m, torch.from_numpy(ok["text"]).cuda(), torch.from_numpy(ok["style"]).cuda(), L=16,
                       diffusion_mode="bogus")
    # strict, by-name weight hand-over at the C-ABI: unknown key and wrong shape are rejected with the key name
    l = _lib.lib()
    buf = np.zeros(4, np.float32)
    shp = (C.c_int64 * 1)(4)
    rc = l.dhw_load(m._handle, b"not.a.key", buf.ctypes.data_as(C.c_void_p), 0, shp, 1)
    assert rc == -2 and b"not.a.key" in l.dhw_last_error(m._handle)
    rc = l.dhw_load(m._handle, b"input_dense.bias", buf.ctypes.data_as(C.c_void_p), 0, shp, 1)
    assert rc == -2 and b"input_dense.bias" in l.dhw_last_error(m._handle)
    # a fresh handle refuses to run before every key has been loaded
    dims = _lib.DhwDims(2, 128, 192, 256, 1, 8, 1, 14, 0)
    h = C.c_void_p()
    assert l.dhw_create(C.byref(h), C.byref(dims), 0) == 0
    try:
        z = torch.zeros(64, device="cuda")
        rc = l.dhw_forward(h, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 8, 1, z.data_ptr(), z.data_ptr(), None)
        assert rc == -2 and b"missing key" in l.dhw_last_error(h)
        rc = l.dhw_forward(h, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 8, 1, z.data_ptr(), z.data_ptr(), None)
        assert rc == -1
    finally:
        l.dhw_destroy(h)


def test_internal_errors_come_back_as_a_status_and_the_handle_survives():
    """include/dhw.h "nothing throws across the ABI", on a live handle: an unknown activation name is an argument error with
    the name in the message (round 4: a std::map::at on such a name aborted the process); an exception raised inside an entry
    point's body is DHW_ERR_INTERNAL with the message on the handle; the handle computes the same forward afterwards."""
    m = get_model(2, "fp32")
    inp = spec.synthetic_inputs(2, 16, 3, seed=4)
    args = [torch.from_numpy(inp[k]).cuda() for k in ("strokes", "text")] + [torch.full((2, 1), 0.6).cuda(), torch.from_numpy(inp["style"]).cuda()]
    e0, p0, _ = m(*args)
    l = _lib.lib()
    buf = np.zeros(16, np.float32)
    shape = (C.c_int64 * 3)()
    # ("enc3.k1" was the internal buffer name of that round; it is a tap now: an internal name that still is none stands in)
    for name in (b"enc3.tl", b"no.such.tap", b""):
        rc = l.dhw_debug_read(m._handle, name, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, shape)
        assert rc == -1 and b"no activation named" in l.dhw_last_error(m._handle), (name, rc)
    with pytest.raises(_lib.DhwError):
        m.debug_read("att_layers.7")
    for kind, needle in ((1, b"map::at"), (2, b"bad_alloc"), (3, b"unknown C++ exception")):
        assert l.dhw_debug_raise(m._handle, kind) == -5
        assert needle in l.dhw_last_error(m._handle)
    e1, p1, _ = m(*args)
    assert torch.equal(e0, e1) and torch.equal(p0, p1)
    assert m.debug_read("enc3").shape == (2, 8, 192)


def test_cpu_inputs_are_moved_and_results_come_back_on_cpu():
    """Drop-in use as in the reference's own smoke test (tests/test_model.py:14-21): CPU tensors in, tensors out."""
    torch.manual_seed(0)
    m = dhg_amd.DiffusionModel(2, 128, 192, 256)   # reference-style constructor, random init
    strokes = torch.rand(8, 400, 2)
    text = (torch.rand(8, 40) < 0.25).int()
    sigma = torch.rand(8, 1)
    style_vector = torch.rand(8, 1, 1280)
    eps, pen, none = m(strokes, text, sigma, style_vector)
    assert eps.shape == (8, 400, 2) and pen.shape == (8, 400) and none is None
    assert eps.device.type == "cpu" and torch.isfinite(eps).all() and ((pen > 0) & (pen < 1)).all()


def _fresh_model(prec, env, **kw):
    """A model whose handle is created under the given library switches (they are read at dhw_create)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = dhg_amd.DiffusionModel(2, precision=prec, max_B=kw.get("B", 4), max_L=kw.get("L", 488), max_Lt=kw.get("Lt", 40)).eval()
        m.load_state_dict(_sd(2), strict=True)
        # force handle creation now, while the switches are set
        inp = spec.synthetic_inputs(1, 8, 2, seed=1)
        fwd(m, inp, torch.full((1, 1), 0.5))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return m


def test_one_launch_per_gemm_path_matches_reference_golden(golden_dir):
    """bf16 with the fused block kernels switched off (DHW_FUSE=0): the generic GEMM + stand-alone attention path."""
    g = np.load(os.path.join(golden_dir, "fwd_pad.npz"))
    B, L, Lt = int(g["B"]), int(g["L"]), int(g["Lt"])
    m = _fresh_model("bf16", {"DHW_FUSE": "0"})
    inp = spec.synthetic_inputs(B, L, Lt, seed=int(g["seed"]), pad=int(g["pad"]))
    alpha = dhg_amd.get_alpha_set()
    eps, pen = fwd(m, inp, torch.sqrt(alpha[30]) * torch.ones((B, 1, 1)))
    assert np.abs(eps - g["eps_i30"]).max() < TOL["bf16"]["eps"]
    assert np.abs(pen - g["pen_i30"]).max() < TOL["bf16"]["pen"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sampler_switches_do_not_change_the_samples(prec):
    """The all-steps text plane, the heads fused into dec1, Upsample + skip_conv fused into the decoder blocks and the
    enc1-fused input Linear only reorder the evaluation:
    every switch combination must give the same samples (same arithmetic per element)."""
    B, L, Lt, T = 3, 80, 9, 7
    inp = spec.synthetic_inputs(B, L, Lt, seed=12, pad=1, T=T)
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    outs = {}
    for name, env in (("default", {}), ("persist", {"DHW_PERSIST": "1"}), ("no_plane", {"DHW_PLANE": "0"}), ("no_fused_heads", {"DHW_FUSE_HEADS": "0"}),
                      ("no_fused_up", {"DHW_FUSE_UP": "0"}), ("no_chain", {"DHW_CHAIN": "0"}),
                      ("enc_bm64", {"DHW_ENC_BM": "64"}), ("enc_bm32", {"DHW_ENC_BM": "32"}), ("conv_bm64", {"DHW_CONV_BM": "64"}),
                      ("f32_enc_per_gemm", {"DHW_FUSE_F32": "0"}), ("unfused", {"DHW_FUSE": "0", "DHW_PLANE": "0"}),
                      ("unfused_text_plane", {"DHW_FUSE_TEXT": "0"}), ("unfused_plane", {"DHW_FUSE": "0"})):
        m = _fresh_model(prec, env, B=B, L=L, Lt=Lt)
        outs[name] = dhg_amd.sample(m, tx, sv, L=L, T=T, noise=nz).cpu()
        # DHW_PERSIST=1 (bf16): every denoiser call is ONE persistent launch (csrc/persist.h); every other configuration launches kernel by kernel
        assert m.persistent_plans() == (1 if (prec == "bf16" and name == "persist") else 0), name
    assert torch.equal(outs["default"], outs["no_plane"])
    # the persistent launch runs the same block bodies (with its own canonical row tiles) behind per-sample counters: same bits
    assert torch.equal(outs["default"], outs["persist"]), "persistent launch"
    # fused vs unfused block kernels round intermediates to bf16 at different points; |x| reaches ~9 after these 7 steps.
    # Measured (r2): <= 0.03 for every pair
    tol = 1e-4 if prec == "fp32" else 0.06
    assert (outs["default"] - outs["no_fused_heads"]).abs().max().item() < tol
    assert (outs["default"] - outs["no_fused_up"]).abs().max().item() < tol   # (bf16 only: fp32 keeps the separate GEMM)
    assert (outs["default"] - outs["no_chain"]).abs().max().item() < tol      # (bf16 only)
    # (DHW_CHAIN_CONV is frozen by the first launch of the process: its conv_chain / no_conv_chain comparisons run in fresh child
    # processes, tests/test_gpu_blocks.py::test_conv_chain_switch_does_not_change_the_samples, same assertion and tolerance)
    # row-tile sizes the launcher would pick for other batch sizes: per-row arithmetic does not depend on the tile
    # fp32: the fused EncoderLayer kernels against one launch per GEMM + stand-alone attention (bf16: switch has no effect)
    assert (outs["default"] - outs["f32_enc_per_gemm"]).abs().max().item() < tol
    for k in ("enc_bm64", "enc_bm32", "conv_bm64"):
        assert (outs["default"] - outs[k]).abs().max().item() < tol, k
    assert (outs["default"] - outs["unfused"]).abs().max().item() < tol
    # the all-steps text plane through the generic GEMM / attention launches (its own ".T" workspace buffers), with the fused stroke kernels and without
    assert (outs["default"] - outs["unfused_text_plane"]).abs().max().item() < tol
    assert (outs["default"] - outs["unfused_plane"]).abs().max().item() < tol


def test_convblock_row_halves_one_phase_apart_give_the_same_bits():
    """DHW_CONV_PP (csrc/convblock_core.h, PP): the tall 126-row ConvBlock tiles (enc1, dec1 once the batch needs them: B x ceil(L / 62)
    > 256 workgroups) with their two row halves running one phase apart.  Only the barrier schedule changes — every MFMA and every
    epilogue operation is the same instruction on the same operands — so the samples must be identical bit for bit, for each of
    the two kinds of block on its own and for both."""
    B, L, Lt, T = 66, 256, 9, 3
    inp = spec.synthetic_inputs(B, L, Lt, seed=14, pad=1, T=T)
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    outs = {}
    for pp in ("0", "1", "2", "3"):
        m = _fresh_model("bf16", {"DHW_CONV_PP": pp}, B=B, L=L, Lt=Lt)
        os.environ["DHW_CONV_PP"] = pp          # (read at launch = graph capture time)
        try:
            outs[pp] = dhg_amd.sample(m, tx, sv, L=L, T=T, noise=nz).cpu()
        finally:
            os.environ.pop("DHW_CONV_PP", None)
        del m
    assert torch.isfinite(outs["0"]).all()
    for pp in ("1", "2", "3"):
        assert torch.equal(outs["0"], outs[pp]), f"DHW_CONV_PP={pp}"


def test_two_text_pairs_per_workgroup_give_the_same_bits():
    """text_layer_kernel holds two (step, prompt) pairs of the all-steps text plane per workgroup when they share a FiLM row (even
    batch): one weight stream for both.  Same MFMA sequence per row => identical samples; forced on here (the launcher's own choice
    needs >= 1024 pairs) against one pair per workgroup, at an even batch whose pairs fill whole and half tiles (Lt = 9 of 32 rows)."""
    B, L, Lt, T = 4, 80, 9, 5
    inp = spec.synthetic_inputs(B, L, Lt, seed=17, pad=2, T=T)
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    outs = [dhg_amd.sample(_fresh_model("bf16", {"DHW_TEXT_PAIRS": v}, B=B, L=L, Lt=Lt), tx, sv, L=L, T=T, noise=nz).cpu() for v in ("1", "2")]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("L", [488, 168, 48, 264])
def test_three_head_layer_on_both_row_tiles_matches_oracle(L, monkeypatch):
    """enc3 (d = 192, three heads: 12 (row group, head) units on 8 waves) on 64-row and on 32-row tiles.  The bench batch picks 64 rows by itself
    (B * ceil(L/2 / 64) >= 256); here the tile is forced at B = 2 so that the oracle finishes in seconds.  Key counts: 244 (four blocks, the last
    one partial), 84 (20 keys in the last block), 24 (a single partial block), 132 (the last block holds 4 keys).  The enc3 tap isolates the layer;
    eps / pen bound what reaches the output."""
    B, Lt = 2, 9
    inp = spec.synthetic_inputs(B, L, Lt, seed=900 + L, pad=1)
    sg = torch.tensor([[0.3], [0.8]])
    taps = {}
    with torch.no_grad():
        e_ref, p_ref = ref_cpu.forward(_sd(2), torch.from_numpy(inp["strokes"]), torch.from_numpy(inp["text"]), sg,
                                       torch.from_numpy(inp["style"]), taps=taps)
    seen = {}
    for prec, bm in (("bf16", "64"), ("bf16", "32"), ("fp32", "64")):
        monkeypatch.setenv("DHW_ENC_BM192", bm)   # (read at every launch)
        m = get_model(2, prec)
        eps, pen = fwd(m, inp, sg)
        ref = taps["enc3"].numpy()
        got = m.debug_read("enc3").numpy().reshape(ref.shape)
        tol = TOL[prec]["tap"] if prec == "fp32" else TOL[prec]["tap_rel"] * np.abs(ref).max()
        assert np.abs(got - ref).max() < tol, (prec, bm, np.abs(got - ref).max(), tol)
        assert np.abs(eps - e_ref.numpy()).max() < TOL[prec]["eps"] and np.abs(pen - p_ref.numpy()).max() < TOL[prec]["pen"]
        seen[prec, bm] = (got.copy(), eps.copy())
    # a row's arithmetic does not depend on the tile the launcher picks (what makes a shard equal to the same samples inside a batch)
    assert np.array_equal(seen["bf16", "64"][0], seen["bf16", "32"][0]) and np.array_equal(seen["bf16", "64"][1], seen["bf16", "32"][1])


def test_long_sequence_config_matches_oracle():
    """BASELINE configs[3] shape class (L=1000, 62 tokens) with a short schedule: exercises multi-block attention
    (L/2 = 500 keys), several row tiles per sample at every level and the T-generalised schedule."""
    B, L, Lt, T = 1, 1000, 62, 3
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=B, max_L=L, max_Lt=Lt).eval()
    m.load_state_dict(_sd(2))
    inp = spec.synthetic_inputs(B, L, Lt, seed=44, T=T)
    noise = torch.from_numpy(inp["noise"])
    ref, _ = ref_cpu.sample(_sd(2), torch.from_numpy(inp["text"]), torch.from_numpy(inp["style"]), L, noise, T=T)
    out = dhg_amd.sample(m, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=L, T=T,
                         noise=noise.cuda()).cpu()
    assert (out - ref).abs().max().item() < 1e-4
    mb = dhg_amd.DiffusionModel(2, precision="bf16", max_B=B, max_L=L, max_Lt=Lt).eval()
    mb.load_state_dict(_sd(2))
    outb = dhg_amd.sample(mb, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=L, T=T,
                          noise=noise.cuda()).cpu()
    assert torch.isfinite(outb).all() and (outb - ref).abs().max().item() < 0.1


def test_infer_file_end_to_end(tmp_path, monkeypatch):
    """The reference's command-line path (inference.py:19-96) around the HIP sampler: experiment directory -> config +
    newest checkpoint -> model -> one prompt -> strokes (+ PNG when matplotlib is there)."""
    (tmp_path / "config.yml").write_text("training_args:\n  att_layers_num: 2\n  channels: 128\n  dropout: 0.0\n")
    torch.save({"state_dict": {"module." + k: v for k, v in _sd(2).items()}}, tmp_path / "checkpoint_2000.pth")
    torch.save({"state_dict": _sd(4)}, tmp_path / "checkpoint_100.pth")          # older, different shape: must not be picked
    style = spec.synthetic_inputs(1, 8, 1, seed=9)["style"][0]
    np.save(tmp_path / "style.npy", style)
    monkeypatch.chdir(tmp_path)
    try:
        import matplotlib  # noqa: F401
        render = True
    except ImportError:
        render = False
    prompt = "Follow the White Rabbit"
    strokes = dhg_amd.infer_file(prompt, str(tmp_path / "style.npy"), experiment_path=str(tmp_path), output="res", seed=3, render=render)
    assert strokes.shape == (392, 3) and np.isfinite(strokes).all()           # 24 tokens -> 16 per token, next multiple of 8
    assert not render or (tmp_path / "res.png").stat().st_size > 0
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=1, max_L=392, max_Lt=24).eval()
    m.load_state_dict(_sd(2))
    ids = torch.tensor([dhg_amd.Tokenizer().encode(prompt)])
    ref = dhg_amd.sample(m, ids.cuda(), torch.from_numpy(style)[None].cuda(), L=392, seed=3).cpu().numpy()[0]
    assert np.array_equal(strokes, ref)


@pytest.mark.parametrize("B,L,Lt,T", [(1, 8, 1, 2), (5, 136, 7, 2), (130, 64, 3, 2), (96, 488, 30, 1), (40, 1000, 62, 1)])
def test_shape_sweep_bf16_tracks_the_fp32_path(B, L, Lt, T):
    """Batch / length combinations that make the launchers pick every row-tile variant (16/32/64-row EncoderLayer tiles,
    46/62/126-row ConvBlock tiles, chained and unchained enc_bc, one or several workgroup rounds): the fused bf16 path
    must track this library's own fp32 path (itself pinned to the reference by the goldens) on the same inputs."""
    inp = spec.synthetic_inputs(B, L, Lt, seed=100 + B, T=T)
    tx, sv, nz = (torch.from_numpy(inp[k]).cuda() for k in ("text", "style", "noise"))
    outs = {}
    for prec in ("fp32", "bf16"):
        m = dhg_amd.DiffusionModel(2, precision=prec, max_B=B, max_L=L, max_Lt=Lt).eval()
        m.load_state_dict(_sd(2))
        outs[prec] = dhg_amd.sample(m, tx, sv, L=L, T=T, noise=nz).cpu()
        del m
    ref, got = outs["fp32"], outs["bf16"]
    assert torch.isfinite(got).all()
    scale = ref[..., :2].abs().max().item()
    assert (got[..., :2] - ref[..., :2]).abs().max().item() < 0.03 * scale      # bf16 weights / activations, T <= 2 steps
    assert (got[..., 2] - ref[..., 2]).abs().max().item() < 0.05
    # ... and both against the CPU oracle on the first and last prompt of the batch, so the variants these shapes select are
    # pinned by the oracle directly, not only through the library's own fp32 path
    for b in sorted({0, B - 1}):
        want, _ = ref_cpu.sample(_sd(2), tx[b:b + 1].cpu(), sv[b:b + 1].cpu(), L, nz[:, b:b + 1].cpu(), T=T)
        wscale = want[..., :2].abs().max().item()
        assert (ref[b:b + 1] - want).abs().max().item() < 1e-3 * max(1.0, wscale), b
        assert (got[b:b + 1, :, :2] - want[..., :2]).abs().max().item() < 0.03 * wscale, b
        assert (got[b:b + 1, :, 2] - want[..., 2]).abs().max().item() < 0.05, b


def test_full_size_batch_matches_the_oracle_on_sampled_prompts():
    """BASELINE configs[1] batch (B=64, L=488, Lt=30) with an 8-step schedule: the launch configuration of the bench
    (126-row ConvBlock tiles, 16-row attention-level tiles, chained enc_bc -> enc_a, all-steps text plane) checked
    directly against the oracle on three prompts of the batch."""
    B, L, Lt, T = 64, 488, 30, 8
    inp = spec.synthetic_inputs(B, L, Lt, seed=21, T=T)
    tx, sv, nz = (torch.from_numpy(inp[k]) for k in ("text", "style", "noise"))
    outs = {}
    for prec in ("fp32", "bf16"):
        m = dhg_amd.DiffusionModel(2, precision=prec, max_B=B, max_L=L, max_Lt=Lt).eval()
        m.load_state_dict(_sd(2))
        outs[prec] = dhg_amd.sample(m, tx.cuda(), sv.cuda(), L=L, T=T, noise=nz.cuda()).cpu()
        del m
    for b in (0, 37, 63):
        ref, _ = ref_cpu.sample(_sd(2), tx[b:b + 1], sv[b:b + 1], L, nz[:, b:b + 1], T=T)
        scale = ref[..., :2].abs().max().item()
        assert (outs["fp32"][b:b + 1] - ref).abs().max().item() < 1e-3, b
        assert (outs["bf16"][b:b + 1, :, :2] - ref[..., :2]).abs().max().item() < 0.03 * scale, b
        assert (outs["bf16"][b:b + 1, :, 2] - ref[..., 2]).abs().max().item() < 0.05, b
