"""Scoring on the host side (no GPU needed): the C-ABI declares, exports and binds dhw_score; every argument of ``score`` and
``candidates`` of ``infer_batch`` is checked with ValueError before any device is touched; and the CPU helper the GPU tests
use as their yardstick (tests/score_ref.py) is itself the reference's training loss: with uniform lengths the batch mean
of its two terms equals ``ref_cpu.loss_fn`` on the same denoiser outputs to 1e-6 on values of order 1 (measured: at most
2.4e-7 over the three levels — the two differ in torch's log1p(-q) against log(1 - q) and in the order of the means)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec
from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, T = 2, 64, 9


def test_score_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+dhw_score\s*\(", header)
    assert hasattr(_lib.lib(), "dhw_score") and "dhw_score" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["dhw_score"]
    assert len(args) == 16
    # a null handle is refused by the argument checks, which run before any HIP call: this answers without a GPU
    lv = (_lib.C.c_int32 * 1)(0)
    assert _lib.lib().dhw_score(None, None, None, None, 1, 8, 1, None, 1, lv, 1, None, 0, 0, None, None) == -1
    assert "null handle" in _lib.lib().dhw_last_error(None).decode()
    assert callable(dhg_amd.score) and callable(dhg_amd.score_file)


def test_default_levels():
    assert dhg_amd.default_levels(60) == [7, 22, 37, 52]
    assert dhg_amd.default_levels(60) == [(2 * j + 1) * 60 // 8 for j in range(4)]
    assert dhg_amd.default_levels(4) == [0, 1, 2, 3]
    assert dhg_amd.default_levels(3) == [0, 1, 2] and dhg_amd.default_levels(1) == [0]   # never more levels than T
    for T_ in range(1, 70):
        lv = dhg_amd.default_levels(T_)
        assert 1 <= len(lv) <= min(4, T_) and all(0 <= v < T_ for v in lv) and (T_ < 4 or len(lv) == 4)


def _model():
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=2, max_L=64, max_Lt=4).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    return m


def _no_device(monkeypatch, m):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the scoring arguments were checked")
    monkeypatch.setattr(m, "_device", boom)
    monkeypatch.setattr(m, "_ensure_handle", boom)


STROKES = torch.zeros((B, L, 3))

BAD = [
    (dict(strokes=torch.zeros((B, L, 2))), r"strokes must be \[B,L,3\]"),
    (dict(strokes=torch.zeros((B, L))), r"strokes must be \[B,L,3\]"),
    (dict(strokes=torch.zeros((B, L, 3), dtype=torch.int64)), "floating-point"),
    (dict(strokes=STROKES.numpy()), "floating-point tensor"),
    (dict(strokes=torch.zeros((B, L + 4, 3))), "multiple of 8"),
    (dict(strokes=torch.zeros((B + 1, L, 3))), r"text must be \[B = 3"),
    (dict(levels=[]), "levels is empty"),
    (dict(levels=[T]), r"levels\[0\] = 9 must lie in \[0, T = 9\)"),
    (dict(levels=[0, -1]), r"levels\[1\] = -1"),
    (dict(levels=[0.5]), "not an integer"),
    (dict(levels=[True]), "not an integer"),
    (dict(levels=[0] * (T + 1)), "more than T"),
    (dict(levels=3), "sequence"),
    (dict(T=0), "T = 0"),
    (dict(levels=[0, 4], noise=torch.zeros((3, B, L, 2))), r"noise must be \[K,B,L,2\]"),
    (dict(levels=[0, 4], noise=torch.zeros((2, B, L, 3))), r"noise must be \[K,B,L,2\]"),
    (dict(noise=torch.zeros((1, B, L, 2))), r"noise must be \[K,B,L,2\]"),   # (default levels: K = 4)
    (dict(levels=[0], noise=torch.zeros((1, B, L, 2), dtype=torch.int32)), "floating-point"),
    (dict(lengths=[64]), "lengths has 1 entries"),
    (dict(lengths=[64, 12]), r"lengths\[1\] = 12"),
    (dict(lengths=[72, 64]), r"lengths\[0\] = 72"),
    (dict(lengths=[64.0, 64]), "not an integer"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_score_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    kw = dict(kw)
    strokes = kw.pop("strokes", STROKES)
    kw.setdefault("T", T)
    text, style = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))
    with pytest.raises(ValueError, match=msg):
        dhg_amd.score(m, strokes, text, style, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(levels=[8, 0, 0]), dict(levels=torch.tensor([1, 2])), dict(lengths=[8, 64], pen_round=True),
                                dict(levels=[3], noise=torch.zeros((1, B, L, 2), dtype=torch.float64))])
def test_valid_score_arguments_get_as_far_as_the_device(monkeypatch, kw):
    m = _model()
    _no_device(monkeypatch, m)
    text, style = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.score(m, STROKES, text, style, T=T, **kw)


@pytest.mark.parametrize("bad", [0, -2, 1.5, True, None])
def test_infer_batch_rejects_bad_candidates(monkeypatch, bad):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(ValueError, match="candidates"):
        dhg_amd.infer_batch(["ab", "c"], torch.zeros((1, 14, 1280)), m, candidates=bad)
    with pytest.raises(ValueError, match="candidates"):
        dhg_amd.infer_file_batch(["ab"], np.zeros((14, 1280), np.float32), "c.yml", "c.pth", candidates=bad)


def test_infer_cli_candidates_and_score_dispatch(monkeypatch, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake_batch(prompts, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(prompts=prompts, **kw)
        return [np.zeros((8, 3), np.float32) for _ in prompts]

    def fake_score(prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, **kw):
        seen.update(score_prompts=prompts, strokes=strokes_path, source=source)
        return [(8 * (i + 1), 1.5, 0.25, 1.75) for i, _ in enumerate(prompts)]

    monkeypatch.setattr(dhg_amd, "infer_file_batch", fake_batch)
    monkeypatch.setattr(dhg_amd, "score_file", fake_score)
    f = tmp_path / "lines.txt"
    f.write_text("first line\nsecond\n")
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--candidates", "5"])
    assert seen["candidates"] == 5 and seen["prompts"] == ["first line", "second"]
    seen.clear()
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp"])
    assert "candidates" not in seen   # candidates = 1: the call of before, argument for argument
    capsys.readouterr()
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--score", "old.npy"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert seen["strokes"] == "old.npy" and seen["source"] == "style.npy" and len(lines) == 2
    assert lines[1] == "line 1: length 16 score 1.5 pen 0.25 total 1.75"
    infer.main(["one prompt", "style.npy", "--experiment-path", "exp", "--score", "old.npy"])
    assert seen["score_prompts"] == ["one prompt"] and len(capsys.readouterr().out.strip().splitlines()) == 1
    for bad in (["--candidates", "0"], ["--score", "old.npy", "--candidates", "2"], ["--score", "old.npy", "--restyle", "x.npy"]):
        with pytest.raises(SystemExit):
            infer.main(["--prompts-file", str(f), "style.npy", *bad])


# ---------------------------------------------------------------- the helper, proven before it is used as a yardstick
def test_score_ref_batch_mean_is_the_reference_loss():
    Bo, Lo, Lt, To = 2, 40, 5, 9
    levels = [0, 4, 8]
    inp = spec.synthetic_inputs(Bo, Lo, Lt, seed=5, T=To)
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}
    text, style = torch.from_numpy(inp["text"]), torch.from_numpy(inp["style"])
    g = torch.Generator().manual_seed(31)
    strokes = torch.randn((Bo, Lo, 3), generator=g)
    strokes[..., 2] = (strokes[..., 2] > 0.5).float()
    noise = torch.randn((len(levels), Bo, Lo, 2), generator=g)
    details = []
    out = score_ref.score(ref_cpu.forward, sd, strokes, text, style, levels, To, noise, details=details)
    assert tuple(out.shape) == (Bo, 3, 2) and torch.isfinite(out).all()
    abar = score_ref.schedule(To)
    assert np.array_equal(abar, _lib.schedule(To)[1]) or np.allclose(abar, _lib.schedule(To)[1], rtol=2e-7, atol=0)
    for k, i in enumerate(levels):
        d = details[k]
        total, s_loss, p_loss = ref_cpu.loss_fn(d["z"], d["eps"], d["pen"], d["q"], torch.full((Bo, 1), float(abar[i])))
        got = out[:, k].sum(dim=1).mean().item()
        diff = abs(got - total.item())
        print(f"level {i}: score_ref batch mean {got:.7f}, loss_fn {total.item():.7f}, difference {diff:.2e} "
              f"(score {abs(out[:, k, 0].mean().item() - s_loss.item()):.2e}, pen {abs(out[:, k, 1].mean().item() - p_loss.item()):.2e})")
        assert 0.1 < total.item() < 10   # ("of order 1")
        assert diff <= 1e-6
    # a ragged call of the helper is each sample alone
    rag = score_ref.score(ref_cpu.forward, sd, strokes, text, style, levels, To, noise, lengths=[Lo, Lo])
    assert torch.allclose(rag, out, rtol=0, atol=1e-6)


# ---------------------------------------------------------------- the host arithmetic of dhw_score, alone, under ASan + UBSan
def test_score_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/score_host_check.cpp (csrc/score/score_host.h only) built with the host compiler under AddressSanitizer + UBSan
    where the toolchain links them (as tests/test_hostpack_cpu.py builds its program), run on the CPU."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "score_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "score_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("score_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    Tq = 9
    abar = _lib.schedule(Tq)[1]
    abar.tofile(tmp_path / "abar.f32")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def run(T_, *levels):
        r = subprocess.run([exe, str(tmp_path / "abar.f32"), str(T_), *map(str, levels)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip().splitlines()

    levels = [8, 0, 4, 4]
    rows = run(Tq, *levels)
    assert len(rows) == 4
    one = np.float32(1.0)
    for ln, i in zip(rows, levels):
        tag, ka, kb, a, it = ln.split()
        got = np.array([float.fromhex(ka), float.fromhex(kb), float.fromhex(a)], np.float32)
        want = np.array([np.sqrt(abar[i]), np.sqrt(one - abar[i]), abar[i]], np.float32)   # fp32 throughout, one rounding per operation
        assert tag == "lv" and np.array_equal(got, want) and int(it) == 2 ** 29 + i
    for T_, lv, what in ((Tq, [], "K = 0"), (Tq, [0, Tq], "levels[1] = 9"), (Tq, [-1], "levels[0] = -1"), (Tq, [0] * (Tq + 1), "K = 10"),
                         (0, [0], "T = 0"), (-3, [0], "T = -3")):
        (ln,) = run(T_, *lv)
        assert ln.startswith("err ") and what in ln, ln
