"""Deterministic sampling and inversion on the host side (no GPU needed): ``ddim_levels``; every argument of ``sample_ddim``,
``invert``, ``transfer`` and ``slerp`` is checked with ValueError before any device is touched; the C-ABI declares, exports and
binds the three dhw_ddim_* symbols and their argument checks answer without a device; ``infer.py --steps`` dispatches; the
CPU helper the GPU tests use as their yardstick (tests/ddim_ref.py) inverts what it samples; and the host arithmetic
(csrc/ddim/ddim_host.h) alone under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ddim_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, T = 2, 64, 9


# ---------------------------------------------------------------- ddim_levels
def test_ddim_levels():
    assert dhg_amd.ddim_levels(60, 4) == [59, 39, 19, 0]
    assert dhg_amd.ddim_levels(60, 1) == [59] and dhg_amd.ddim_levels(1) == [0] and dhg_amd.ddim_levels(1, 1) == [0]
    assert dhg_amd.ddim_levels(60, 60) == list(range(59, -1, -1)) == dhg_amd.ddim_levels(60) == dhg_amd.ddim_levels()
    assert dhg_amd.ddim_levels(9, 4) == [8, 5, 2, 0] and dhg_amd.ddim_levels(9, 2) == [8, 0]
    for T_ in range(1, 70):
        for s in range(1, T_ + 1):
            lv = dhg_amd.ddim_levels(T_, s)
            assert len(lv) == s and lv[0] == T_ - 1 and (s == 1 or lv[-1] == 0)
            assert all(a > b for a, b in zip(lv, lv[1:])), (T_, s, lv)                       # strictly decreasing for every steps <= T
            assert s == 1 or lv == [((s - 1 - j) * (T_ - 1)) // (s - 1) for j in range(s)]
    for bad in (dict(steps=0), dict(steps=61), dict(steps=-1), dict(steps=2.0), dict(steps=True), dict(T=0), dict(T=1.5), dict(T=2 ** 29 + 1)):
        with pytest.raises(ValueError):
            dhg_amd.ddim_levels(**{**dict(T=60), **bad})


# ---------------------------------------------------------------- validation before any device is touched
def _model():
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=2, max_L=64, max_Lt=4).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    return m


def _no_device(monkeypatch, m):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(m, "_device", boom)
    monkeypatch.setattr(m, "_ensure_handle", boom)


TEXT, STYLE = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))
STROKES = torch.zeros((B, L, 3))

BAD_LEVELS = [
    (dict(steps=0), "steps = 0"),
    (dict(steps=T + 1), r"steps = 10 must lie in \[1, T = 9\]"),
    (dict(steps=2.5), "not an integer"),
    (dict(steps=True), "not an integer"),
    (dict(steps=3, levels=[8, 4, 0]), "steps or levels, not both"),
    (dict(levels=[]), "levels is empty"),
    (dict(levels=[T]), r"levels\[0\] = 9 must lie in \[0, T = 9\)"),
    (dict(levels=[3, -1]), r"levels\[1\] = -1"),
    (dict(levels=[4, 4]), r"levels\[1\] = 4 is not below levels\[0\] = 4"),
    (dict(levels=[0, 8]), "strictly decreasing"),
    (dict(levels=[0.5]), "not an integer"),
    (dict(levels=[True]), "not an integer"),
    (dict(levels=list(range(T, -1, -1))), "more than T"),
    (dict(levels=3), "sequence"),
    (dict(T=0), "T = 0"),
    (dict(lengths=[64]), "lengths has 1 entries"),
    (dict(lengths=[64, 12]), r"lengths\[1\] = 12"),
    (dict(lengths=[72, 64]), r"lengths\[0\] = 72"),
    (dict(lengths=[64.0, 64]), "not an integer"),
]
BAD_SAMPLE = BAD_LEVELS + [
    (dict(latent=torch.zeros((B, L, 3))), r"latent must be \[B,L,2\]"),
    (dict(latent=torch.zeros((B + 1, L, 2))), r"latent must be \[B,L,2\]"),
    (dict(latent=torch.zeros((B, L + 8, 2))), r"latent must be \[B,L,2\]"),
    (dict(latent=torch.zeros((B, L, 2), dtype=torch.int32)), "floating-point"),
    (dict(latent=np.zeros((B, L, 2), np.float32)), "floating-point tensor"),
    (dict(L=60), "multiple of 8"),
    (dict(L=0), "L = 0"),
    (dict(seed=-1), "seed = -1"),
    (dict(seed=1.0), "not an integer"),
    (dict(first_sample=0.5), "not an integer"),
    (dict(text=torch.ones((B + 1, 4), dtype=torch.int64)), "style_vector must be a tensor"),
    (dict(text=torch.ones((B, 4))), "integer tensor"),
    (dict(style=torch.zeros((B, 14, 1279))), "style_vector"),
]
BAD_INVERT = BAD_LEVELS + [
    (dict(strokes=torch.zeros((B, L, 2))), r"strokes must be \[B,L,3\]"),
    (dict(strokes=torch.zeros((B, L, 3), dtype=torch.int64)), "floating-point"),
    (dict(strokes=STROKES.numpy()), "floating-point tensor"),
    (dict(strokes=torch.zeros((B, L + 4, 3))), "multiple of 8"),
    (dict(strokes=torch.zeros((B + 1, L, 3))), r"text must be an integer tensor \[B = 3"),
    (dict(iters=0), r"iters = 0 must lie in \[1, 8\]"),
    (dict(iters=9), r"iters = 9 must lie in \[1, 8\]"),
    (dict(iters=1.0), "not an integer"),
    (dict(iters=True), "not an integer"),
    (dict(style=torch.zeros((B, 14))), "style_vector"),
]


@pytest.mark.parametrize("kw,msg", BAD_SAMPLE)
def test_sample_ddim_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    kw = dict(kw)
    text, style = kw.pop("text", TEXT), kw.pop("style", STYLE)
    kw.setdefault("T", T)
    kw.setdefault("L", L)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.sample_ddim(m, text, style, **kw)


@pytest.mark.parametrize("kw,msg", BAD_INVERT)
def test_invert_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    kw = dict(kw)
    strokes, style = kw.pop("strokes", STROKES), kw.pop("style", STYLE)
    kw.setdefault("T", T)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.invert(m, strokes, TEXT, style, **kw)
    # transfer hands the same arguments to invert first
    with pytest.raises(ValueError, match=msg):
        dhg_amd.transfer(strokes, TEXT, style, torch.zeros((strokes.shape[0], 14, 1280)), m, **kw)


def test_transfer_and_slerp_reject_bad_arguments(monkeypatch):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(ValueError, match="unknown keyword"):
        dhg_amd.transfer(STROKES, TEXT, STYLE, STYLE, m, T=T, seed=3)
    with pytest.raises(ValueError, match="style_to"):
        dhg_amd.transfer(STROKES, TEXT, STYLE, torch.zeros((B + 1, 14, 1280)), m, T=T)
    with pytest.raises(ValueError, match="text_to"):
        dhg_amd.transfer(STROKES, TEXT, STYLE, STYLE, m, T=T, text_to=torch.ones((B + 1, 4), dtype=torch.int64))
    a = torch.zeros((B, L, 2))
    for args, msg in (((a, torch.zeros((B, L, 3)), 0.5), "latent_b"), ((a, torch.zeros((B, L + 8, 2)), 0.5), "differ in shape"),
                      ((a.long(), a, 0.5), "latent_a"), ((a, a, [0.1, 0.2, 0.3]), "w must be"), ((a, a, float("nan")), "w must be")):
        with pytest.raises(ValueError, match=msg):
            dhg_amd.slerp(*args)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 12"):
        dhg_amd.slerp(a, a, 0.5, lengths=[64, 12])


@pytest.mark.parametrize("kw", [dict(), dict(steps=4), dict(steps=1), dict(levels=[8, 3, 0]), dict(levels=torch.tensor([7, 2])), dict(lengths=[8, 64]),
                                dict(latent=torch.zeros((B, L, 2), dtype=torch.float64), seed=2 ** 64 - 1, return_latent=True)])
def test_valid_arguments_get_as_far_as_the_device(monkeypatch, kw):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.sample_ddim(m, TEXT, STYLE, **{**dict(T=T, L=L), **kw})
    inv = {k: v for k, v in kw.items() if k in ("steps", "levels", "lengths")}
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.invert(m, STROKES, TEXT, STYLE, T=T, iters=8, **inv)
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.transfer(STROKES, TEXT, STYLE, STYLE, m, T=T, iters=2, **inv)


def test_slerp_is_spherical_and_per_sample():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((2, 16, 2), generator=g), torch.randn((2, 16, 2), generator=g)
    lens = [8, 16]
    assert torch.allclose(dhg_amd.slerp(a, b, 0.0), a, atol=1e-6) and torch.allclose(dhg_amd.slerp(a, b, 1.0), b, atol=1e-6)
    mid = dhg_amd.slerp(a, b, [0.5, 0.25], lengths=lens)
    assert torch.equal(mid[0, 8:], torch.zeros((8, 2)))
    for i, (n, w) in enumerate(zip(lens, (0.5, 0.25))):
        x, y = a[i, :n].double().flatten(), b[i, :n].double().flatten()
        t = torch.acos(torch.dot(x, y) / (x.norm() * y.norm()))
        want = (torch.sin((1 - w) * t) * x + torch.sin(w * t) * y) / torch.sin(t)
        assert torch.allclose(mid[i, :n].double().flatten(), want, atol=1e-5)
        assert torch.allclose(mid[i:i + 1, :n], dhg_amd.slerp(a[i:i + 1, :n], b[i:i + 1, :n], w), atol=0)   # a row depends on its own sample alone
    same = dhg_amd.slerp(a, a, 0.3)                                                    # parallel latents: the linear branch
    assert torch.allclose(same, a, atol=1e-6)
    unit = torch.nn.functional.normalize(torch.randn((1, 8, 2), generator=g).flatten(), dim=0).reshape(1, 8, 2)
    other = torch.nn.functional.normalize(torch.randn((1, 8, 2), generator=g).flatten(), dim=0).reshape(1, 8, 2)
    assert abs(dhg_amd.slerp(unit, other, 0.37).norm().item() - 1.0) < 1e-5            # stays on the sphere


# ---------------------------------------------------------------- the C-ABI
def test_ddim_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    for name, nargs in (("dhw_ddim_sample", 16), ("dhw_ddim_invert", 14), ("dhw_ddim_update", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    l = _lib.lib()
    lv = (C.c_int32 * 1)(0)
    # a null handle is refused by the argument checks, which run before any HIP call: these answer without a GPU
    assert l.dhw_ddim_sample(None, None, None, 1, 8, 1, None, 1, lv, 1, None, 0, 0, None, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    assert l.dhw_ddim_invert(None, None, None, None, 1, 8, 1, None, 1, lv, 1, 1, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    for name in ("ddim_levels", "sample_ddim", "invert", "transfer", "slerp"):
        assert callable(getattr(dhg_amd, name)), name


def test_ddim_update_checks_answer_without_a_device():
    """dhw_ddim_update takes no handle: its refusals are read through dhw_last_error(NULL), each naming its argument."""
    l = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    for args, what in (((p, p, None, 0, 8, p), "B=0"), ((p, p, None, 1, 0, p), "L=0"), ((p, p, None, 2 ** 16, 2 ** 15, p), "below 2^31"),
                       ((None, p, None, 1, 8, p), "(base)"), ((p, None, None, 1, 8, p), "(eps)"), ((p, p, None, 1, 8, None), "(out)"),
                       ((p + 4, p, None, 1, 8, p), "base must be 8-byte aligned"), ((p, p + 4, None, 1, 8, p), "eps must be 8-byte aligned"),
                       ((p, p, None, 1, 8, p + 4), "out must be 8-byte aligned"), ((p, p, p + 2, 1, 8, p), "lens must be 4-byte aligned")):
        base, eps, lens, B_, L_, out = args
        rc = l.dhw_ddim_update(base, eps, lens, B_, L_, 1.0, 0.0, 1.0, 0.0, out, None)
        msg = l.dhw_last_error(None).decode()
        assert rc == -1 and what in msg and "dhw_ddim_update" in msg, (what, rc, msg)


# ---------------------------------------------------------------- the command line
def test_infer_cli_steps_dispatch(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake_batch(prompts, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(batch=prompts, **kw)
        return [np.zeros((8, 3), np.float32) for _ in prompts]

    def fake_one(prompt, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(one=prompt, **kw)
        return np.zeros((8, 3), np.float32)

    monkeypatch.setattr(dhg_amd, "infer_file_batch", fake_batch)
    monkeypatch.setattr(dhg_amd, "infer_file", fake_one)
    f = tmp_path / "lines.txt"
    f.write_text("first line\nsecond\n")
    for renderer in ("matplotlib", "gpu"):
        seen.clear()
        infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--steps", "12", "--renderer", renderer])
        assert seen["steps"] == 12 and seen["batch"] == ["first line", "second"] and seen["renderer"] == renderer and "candidates" not in seen
        seen.clear()
        infer.main(["a prompt", "style.npy", "--experiment-path", "exp", "--steps", "7", "--renderer", renderer])
        assert seen["steps"] == 7 and seen["one"] == "a prompt" and seen["renderer"] == renderer
    seen.clear()
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--steps", "5", "--candidates", "3"])
    assert seen["steps"] == 5 and seen["candidates"] == 3
    for argv in (["--prompts-file", str(f), "style.npy", "--experiment-path", "exp"], ["a prompt", "style.npy", "--experiment-path", "exp"]):
        seen.clear()
        infer.main(argv)
        assert "steps" not in seen   # without the flag: the call of before, argument for argument
    for bad in (["--steps", "0"], ["--steps", "-3"], ["--steps", "4", "--score", "old.npy"], ["--steps", "4", "--restyle", "old.npy"],
                ["--steps", "4", "--align", "old.npy"], ["--steps", "x"]):
        with pytest.raises(SystemExit):
            infer.main(["--prompts-file", str(f), "style.npy", *bad])


def test_steps_reach_the_deterministic_sampler(monkeypatch):
    """infer / infer_batch with ``steps`` call sample_ddim with ddim_levels(T, steps); without it they call sample as before."""
    from dhg_amd import inference
    calls = []

    def fake_ddim(model, text, sv, **kw):
        calls.append(("ddim", kw))
        return torch.zeros((text.shape[0], kw["L"], 3))

    def fake_sample(model, text, sv, **kw):
        calls.append(("sample", kw))
        return torch.zeros((text.shape[0], kw["L"], 3))

    monkeypatch.setattr(inference, "sample_ddim", fake_ddim)
    monkeypatch.setattr(inference, "sample", fake_sample)
    sv = torch.zeros((1, 14, 1280))
    inference.infer("Hi", sv, None, T=60, seed=4, steps=4)
    assert calls[-1][0] == "ddim" and calls[-1][1]["levels"] == [59, 39, 19, 0] and calls[-1][1]["seed"] == 4 and calls[-1][1]["T"] == 60
    out = inference.infer_batch(["Hi", "Rabbit"], sv, None, T=9, seed=1, first_sample=3, steps=2)
    kind, kw = calls[-1]
    assert kind == "ddim" and kw["levels"] == [8, 0] and kw["first_sample"] == 3 and kw["lengths"] == [len(o) for o in out]
    inference.infer("Hi", sv, None, seed=4)
    inference.infer_batch(["Hi"], sv, None)
    assert [c[0] for c in calls[-2:]] == ["sample", "sample"] and all("levels" not in c[1] for c in calls[-2:])
    with pytest.raises(ValueError, match="steps = 61"):
        inference.infer("Hi", sv, None, steps=61)


# ---------------------------------------------------------------- the helper, proven before it is used as a yardstick
def test_ddim_ref_sampling_inverts_inversion_for_a_fixed_eps():
    """With a denoiser whose answer does not depend on x, step j of ddim_ref.invert solves step j of ddim_ref.sample exactly in
    real arithmetic (one fixed-point iteration is the fixed point), so sample(invert(x)) = x up to rounding.  The bound is
    derived, not measured: a round trip over S levels is 2 S updates of 5 float32 operations, each rounding its own result by
    at most half an ulp: 5 * 2 S * 0.5 = 20 ulp at S = 4.  The ulp is taken at the largest magnitude an intermediate can have,
    (max|x| + max|e|) / min_j A_j: every intermediate is a level's A x0 + B e with A, B <= 1, or the x0 estimate, which divides
    by A_j."""
    To, S = 9, 4
    levels = dhg_amd.ddim_levels(To, S)
    assert levels == [8, 5, 2, 0]
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 40, 3), generator=g)
    e_fixed = torch.randn((1, 40, 2), generator=g)   # (the same for every sample, so that a sample run alone gets its own)
    q_fixed = torch.rand((1, 40), generator=g)

    def const(sd, xin, text, sigma, style):
        n = xin.shape[1]
        return e_fixed[:, :n].expand(xin.shape[0], n, 2), q_fixed[:, :n].expand(xin.shape[0], n)

    lat = ddim_ref.invert(const, None, x, None, None, levels, To)
    back = ddim_ref.sample(const, None, None, None, levels, To, lat)
    a_min = min(float(c[0]) for c in ddim_ref.coefs(levels, To))
    scale = (x[..., :2].abs().max().item() + e_fixed.abs().max().item()) / a_min
    ulp = float(np.spacing(np.float32(scale)))
    err = (back[..., :2] - x[..., :2]).abs().max().item()
    print(f"round trip with a fixed eps: max error {err:.3e} = {err / ulp:.2f} ulp at {scale:.3f} (bound 20 ulp = {20 * ulp:.3e})")
    assert err <= 20 * ulp
    assert torch.equal(back[..., 2], q_fixed.expand(2, 40)) and not torch.equal(lat, x[..., :2])
    for k in (2, 3):   # further iterations start from the fixed point: they change nothing
        assert torch.equal(ddim_ref.invert(const, None, x, None, None, levels, To, iters=k), lat)
    # a ragged call of the helper is each sample alone
    rag = ddim_ref.sample(const, None, [None, None], [None, None], levels, To, lat, lengths=[40, 24])
    assert torch.equal(rag[0], back[0]) and torch.equal(rag[1, :24], back[1, :24]) and torch.equal(rag[1, 24:], torch.zeros((16, 3)))
    # the coefficients are the header's: sqrt(a_j), sqrt(1 - a_j), then (1, 0); the schedule is the library's to the last bit or ulp
    abar = ddim_ref.schedule(To)
    assert np.array_equal(abar, _lib.schedule(To)[1]) or np.allclose(abar, _lib.schedule(To)[1], rtol=2e-7, atol=0)
    c = ddim_ref.coefs(levels, To)
    assert len(c) == S + 1 and c[-1] == (np.float32(1), np.float32(0)) and c[0][0] == np.sqrt(abar[8]) and c[0][0].dtype == np.float32


# ---------------------------------------------------------------- the host arithmetic of the ddim entries, alone, under ASan + UBSan
def test_ddim_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/ddim_host_check.cpp (csrc/ddim/ddim_host.h only) built with the host compiler under AddressSanitizer + UBSan
    where the toolchain links them (as tests/test_score_cpu.py builds its program), run on the CPU: the coefficient table
    against numpy bit for bit, every refusal, and (inside the program) a message buffer shorter than the message."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "ddim_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "ddim_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("ddim_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    Tq = 9
    abar = _lib.schedule(Tq)[1]
    abar.tofile(tmp_path / "abar.f32")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def run(T_, iters, *levels):
        r = subprocess.run([exe, str(tmp_path / "abar.f32"), str(T_), str(iters), *map(str, levels)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip().splitlines()

    one = np.float32(1.0)
    for levels in ([8, 5, 2, 0], [8], [0], list(range(8, -1, -1))):
        rows = run(Tq, 1, *levels)
        assert len(rows) == len(levels) + 1
        want = [(np.sqrt(abar[i]), np.sqrt(one - abar[i])) for i in levels] + [(one, np.float32(0))]   # fp32 throughout, one rounding per operation
        for ln, (A, Bc) in zip(rows, want):
            tag, a_, b_ = ln.split()
            got = np.array([float.fromhex(a_), float.fromhex(b_)], np.float32)
            assert tag == "co" and np.array_equal(got, np.array([A, Bc], np.float32)), (levels, ln)
    for T_, it, lv, what in ((Tq, 1, [], "S = 0"), (Tq, 1, [Tq], "levels[0] = 9"), (Tq, 1, [3, -1], "levels[1] = -1"), (Tq, 1, [4, 4], "strictly decreasing"),
                             (Tq, 1, [0, 8], "levels[1] = 8 is not below levels[0] = 0"), (Tq, 1, list(range(9, -1, -1)), "S = 10"),
                             (0, 1, [0], "T = 0"), (-3, 1, [0], "T = -3"), (2 ** 29 + 1, 1, [0], "2^29"), (Tq, 0, [8, 0], "iters = 0"), (Tq, 9, [8, 0], "iters = 9"),
                             (Tq, -1, [8], "iters = -1")):
        (ln,) = run(T_, it, *lv)
        assert ln.startswith("err ") and what in ln, ln
    assert run(Tq, 8, 8, 0)[0].startswith("co ")
