"""Conditioned sampling on the host side (no GPU needed): the C-ABI declares, exports and binds dhw_sample_cond, every
conditioning argument of ``sample`` / ``restyle`` is checked with ValueError before any device is touched, and the CPU
helper the GPU tests use as their yardstick (tests/cond_ref.py) is itself proven against the oracle's unconditioned loop."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, inference, spec
from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, T = 2, 64, 4


def test_cond_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+dhw_sample_cond\s*\(", header)
    assert hasattr(_lib.lib(), "dhw_sample_cond") and "dhw_sample_cond" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["dhw_sample_cond"]
    assert len(args) == len(_lib.SIGNATURES["dhw_sample_ragged"][1]) + 4
    # a null handle is refused by the argument checks, which run before any HIP call: this answers without a GPU
    assert _lib.lib().dhw_sample_cond(None, None, None, 1, 8, 1, None, 1, 0, None, 0, 0, None, None, 1, None, None, None) == -1
    assert "null handle" in _lib.lib().dhw_last_error(None).decode()


def _model():
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=2, max_L=64, max_Lt=4).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    return m


def _no_device(monkeypatch, m):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the conditioning arguments were checked")
    monkeypatch.setattr(m, "_device", boom)
    monkeypatch.setattr(m, "_ensure_handle", boom)


KNOWN = torch.zeros((B, L, 3))
KEEP = torch.zeros((B, L), dtype=torch.bool)
NOISE = torch.zeros((T + 1, B, L, 2))
CNOISE = torch.zeros((T, B, L, 2))

BAD = [
    (dict(known=KNOWN, t_start=0), r"t_start = 0"),
    (dict(known=KNOWN, t_start=T + 1), r"t_start = 5"),
    (dict(known=KNOWN, t_start=2.0), "not an integer"),
    (dict(known=KNOWN, t_start=True), "not an integer"),
    (dict(t_start=2), "needs known"),
    (dict(keep=KEEP), "keep needs known"),
    (dict(known=torch.zeros((B, L, 2))), r"known must be \[B,L,3\]"),
    (dict(known=torch.zeros((B, L + 8, 3))), r"known must be \[B,L,3\]"),
    (dict(known=torch.zeros((B, L, 3), dtype=torch.int32)), "floating-point"),
    (dict(known=KNOWN.numpy()), "floating-point tensor"),
    (dict(known=KNOWN, keep=torch.zeros((B, L + 8), dtype=torch.bool)), r"keep must be \[B,L\]"),
    (dict(known=KNOWN, keep=torch.zeros((B, L, 1), dtype=torch.bool)), r"keep must be \[B,L\]"),
    (dict(known=KNOWN, keep=torch.zeros((B, L))), "bool or uint8"),
    (dict(known=KNOWN, keep=torch.zeros((B, L), dtype=torch.int64)), "bool or uint8"),
    (dict(known=KNOWN, keep=KEEP, noise=NOISE), "cond_noise is required"),
    (dict(known=KNOWN, keep=KEEP, cond_noise=CNOISE), "noise is missing"),
    (dict(known=KNOWN, noise=NOISE, cond_noise=CNOISE), "keep is missing"),
    (dict(known=KNOWN, keep=KEEP, noise=NOISE, cond_noise=torch.zeros((T + 1, B, L, 2))), r"cond_noise must be \[T,B,L,2\]"),
    (dict(known=KNOWN, keep=KEEP, noise=NOISE, cond_noise=CNOISE.double().long()), "floating-point"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_sample_rejects_bad_conditioning_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    text, style = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))
    with pytest.raises(ValueError, match=msg):
        dhg_amd.sample(m, text, style, L=L, T=T, **kw)


@pytest.mark.parametrize("kw", [dict(known=KNOWN), dict(known=KNOWN, keep=KEEP), dict(known=KNOWN, keep=KEEP.to(torch.uint8), t_start=1),
                                dict(known=KNOWN, t_start=2, noise=NOISE), dict(known=KNOWN, keep=KEEP, noise=NOISE, cond_noise=CNOISE),
                                dict(t_start=T), dict(known=KNOWN.double(), lengths=[8, 64])])
def test_valid_conditioning_gets_as_far_as_the_device(monkeypatch, kw):
    m = _model()
    _no_device(monkeypatch, m)
    text, style = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.sample(m, text, style, L=L, T=T, **kw)


def test_restyle_maps_strength_to_t_start_and_checks_it(monkeypatch):
    calls = []

    def fake_sample(model, text, style, **kw):
        calls.append(kw)
        return torch.zeros((text.shape[0], kw["L"], 3))

    monkeypatch.setattr(inference, "sample", fake_sample)
    text, style = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))
    for strength, T_, want in ((0.5, 60, 30), (0.0, 60, 1), (1.0, 60, 60), (0.26, 9, 2), (0.01, 9, 1), (0.99, 9, 9)):
        out = dhg_amd.restyle(KNOWN, text, style, None, lengths=[8, 64], strength=strength, keep=KEEP, T=T_, seed=3)
        kw = calls.pop()
        assert kw["t_start"] == want and kw["T"] == T_ and kw["L"] == L and kw["lengths"] == [8, 64] and kw["seed"] == 3
        assert kw["known"] is KNOWN and kw["keep"] is KEEP and tuple(out.shape) == (B, L, 3)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            dhg_amd.restyle(KNOWN, text, style, None, strength=bad)
    with pytest.raises(ValueError, match=r"strokes must be \[B,L,3\]"):
        dhg_amd.restyle(KNOWN[..., :2], text, style, None)


def test_infer_cli_restyle_and_save_strokes_dispatch(monkeypatch, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake_restyle(prompts, strokes_path, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(prompts=prompts, strokes=strokes_path, source=source, output=output, **kw)
        return [np.full((dhg_amd.stroke_length(len(p)), 3), 1.0 + i, np.float32) for i, p in enumerate(prompts)]

    monkeypatch.setattr(dhg_amd, "restyle_file", fake_restyle)
    f = tmp_path / "lines.txt"
    f.write_text("first line\nsecond\n")
    saved = tmp_path / "new.npy"
    infer.main(["--prompts-file", str(f), "other.npy", "--experiment-path", "exp", "--restyle", "old.npy", "--strength", "0.25",
                "--save-strokes", str(saved), "--renderer", "gpu"])
    assert seen["prompts"] == ["first line", "second"] and seen["strokes"] == "old.npy" and seen["source"] == "other.npy"
    assert seen["strength"] == 0.25 and seen["renderer"] == "gpu"
    arr = np.load(saved)
    n0, n1 = dhg_amd.stroke_length(len("first line")), dhg_amd.stroke_length(len("second"))
    assert arr.shape == (2, max(n0, n1), 3) and n1 < n0
    assert (arr[0] == 1.0).sum() > 0 and not arr[1, arr.shape[1] - 1].any()   # the shorter line is padded with 0
    with pytest.raises(SystemExit):
        infer.main(["--prompts-file", str(f), "other.npy", "--restyle", "old.npy", "--strength", "1.5"])


# ---------------------------------------------------------------- the helper, proven before it is used as a yardstick
def _oracle_inputs():
    Bo, Lo, Lt, To = 2, 40, 5, 9
    inp = spec.synthetic_inputs(Bo, Lo, Lt, seed=5, T=To)
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}
    return sd, torch.from_numpy(inp["text"]), torch.from_numpy(inp["style"]), torch.from_numpy(inp["noise"]), Lo, To


@pytest.mark.parametrize("mode", ["new", "standard"])
def test_cond_ref_without_conditioning_reproduces_the_oracle_loop(mode):
    sd, text, style, noise, Lo, To = _oracle_inputs()
    ref, _ = ref_cpu.sample(sd, text, style, Lo, noise, T=To, mode=mode)
    known = torch.full((2, Lo, 3), float("nan"))
    got = cond_ref.cond_sample(ref_cpu.forward, sd, text, style, Lo, noise, T=To, mode=mode, known=known,
                               keep=torch.zeros((2, Lo), dtype=torch.bool), t_start=To, cond_noise=torch.zeros((To, 2, Lo, 2)))
    err = (got - ref).abs().max().item()
    print(f"cond_ref vs ref_cpu.sample [{mode}]: max abs difference {err:.3e}")
    assert torch.isfinite(got).all() and err <= 1e-6
    plain = cond_ref.cond_sample(ref_cpu.forward, sd, text, style, Lo, noise, T=To, mode=mode)
    assert torch.equal(plain, got)


@pytest.mark.parametrize("t_start", [9, 4, 1])
def test_cond_ref_with_everything_kept_returns_known(t_start):
    sd, text, style, noise, Lo, To = _oracle_inputs()
    g = torch.Generator().manual_seed(3)
    known = torch.randn((2, Lo, 3), generator=g)
    known[..., 2] = (known[..., 2] > 0).float()
    calls = []

    def fwd(*a):
        calls.append(1)
        return ref_cpu.forward(*a)

    got = cond_ref.cond_sample(fwd, sd, text, style, Lo, noise, T=To, known=known, keep=torch.ones((2, Lo), dtype=torch.bool),
                               t_start=t_start, cond_noise=torch.randn((To, 2, Lo, 2), generator=g))
    assert torch.equal(got, known) and len(calls) == t_start
