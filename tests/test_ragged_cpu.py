"""Ragged batches on the host side (no GPU needed): the C-ABI declares and exports the ragged entry points, bad ``lengths``
are rejected with ValueError before any device is touched, ``infer_batch`` sets every prompt's own stroke length and pads the
text with 0, and ``infer.py --prompts-file`` parses and dispatches."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, inference, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_entry_points_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in ("dhw_forward_ragged", "dhw_sample_ragged"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def _model():
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=2, max_L=64, max_Lt=4).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    return m


def _no_device(monkeypatch, m):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the lengths were checked")
    monkeypatch.setattr(m, "_device", boom)
    monkeypatch.setattr(m, "_ensure_handle", boom)


BAD = [([8, 12], "multiple of 8"), ([0, 8], r"lengths\[0\] = 0"), ([8, 72], r"lengths\[1\] = 72"), ([8], "2"),
       ([8, 16, 24], "3 entries"), ([8.0, 16], "not an integer"), ([-8, 16], r"lengths\[0\] = -8"),
       (torch.tensor([8.0, 16.0]), "integers"), (np.array([8.5, 16.0]), "not an integer"), (7, "sequence")]


@pytest.mark.parametrize("lengths,msg", BAD)
def test_sample_rejects_bad_lengths_before_any_device_access(monkeypatch, lengths, msg):
    m = _model()
    _no_device(monkeypatch, m)
    text = torch.ones((2, 4), dtype=torch.int64)
    style = torch.zeros((2, 14, 1280))
    with pytest.raises(ValueError, match=msg):
        dhg_amd.sample(m, text, style, L=64, T=2, lengths=lengths)


@pytest.mark.parametrize("lengths,msg", BAD)
def test_forward_rejects_bad_lengths_before_any_device_access(monkeypatch, lengths, msg):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(ValueError, match=msg):
        m(torch.zeros((2, 64, 2)), torch.ones((2, 4), dtype=torch.int64), torch.full((2, 1), 0.5), torch.zeros((2, 14, 1280)),
          lengths=lengths)


def test_lengths_default_L_is_their_maximum_and_bound_it(monkeypatch):
    m = _model()
    _no_device(monkeypatch, m)
    text, style = torch.ones((2, 4), dtype=torch.int64), torch.zeros((2, 14, 1280))
    with pytest.raises(AssertionError, match="device was touched"):   # valid: gets as far as the device
        dhg_amd.sample(m, text, style, T=2, lengths=[8, 40])
    with pytest.raises(ValueError, match=r"L = 32"):
        dhg_amd.sample(m, text, style, L=32, T=2, lengths=[8, 40])


def test_forward_with_lengths_is_inference_only(monkeypatch):
    m = _model()
    _no_device(monkeypatch, m)
    args = (torch.zeros((2, 64, 2)), torch.ones((2, 4), dtype=torch.int64), torch.full((2, 1), 0.5), torch.zeros((2, 14, 1280)))
    m.train()
    with pytest.raises(ValueError, match="inference-only"):
        m(*args, lengths=[8, 64])
    m.eval()
    m.requires_grad_(True)
    with pytest.raises(ValueError, match="inference-only"):
        m(*args, lengths=[8, 64])


def test_infer_batch_sets_each_prompts_length_and_pads_the_text(monkeypatch):
    calls = []

    def fake_sample(model, text, style, L=None, T=60, diffusion_mode="new", noise=None, seed=0, first_sample=0, lengths=None):
        calls.append(dict(text=text.clone(), style=style, L=L, T=T, mode=diffusion_mode, seed=seed, first=first_sample, lengths=list(lengths)))
        return torch.arange(text.shape[0] * L * 3, dtype=torch.float32).reshape(text.shape[0], L, 3)

    monkeypatch.setattr(inference, "sample", fake_sample)
    prompts = ["Hi", "Follow the White Rabbit", "abc"]
    tok = dhg_amd.Tokenizer()
    ids = [tok.encode(p) for p in prompts]
    out = dhg_amd.infer_batch(prompts, torch.zeros((1, 14, 1280)), model=None, diffusion_mode="standard", T=7, seed=5, first_sample=2)
    (c,) = calls
    lens = [dhg_amd.stroke_length(len(i)) for i in ids]
    assert c["lengths"] == lens and c["L"] == max(lens) and c["T"] == 7 and c["mode"] == "standard" and c["seed"] == 5 and c["first"] == 2
    assert c["text"].shape == (3, max(len(i) for i in ids))
    for b, i in enumerate(ids):
        assert c["text"][b, :len(i)].tolist() == i and not c["text"][b, len(i):].any()
    assert tuple(c["style"].shape) == (3, 14, 1280)
    assert [o.shape for o in out] == [(n, 3) for n in lens]
    full = torch.arange(3 * max(lens) * 3, dtype=torch.float32).reshape(3, max(lens), 3).numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(out[b], full[b, :n])
    with pytest.raises(ValueError, match="style_vector"):
        dhg_amd.infer_batch(prompts, torch.zeros((2, 14, 1280)), model=None)


def test_infer_cli_prompts_file_dispatches(monkeypatch, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake_batch(prompts, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(prompts=prompts, source=source, exp=experiment_path, output=output, mode=mode, **kw)
        return [np.zeros((dhg_amd.stroke_length(len(p)), 3), np.float32) for p in prompts]

    monkeypatch.setattr(dhg_amd, "infer_file_batch", fake_batch)
    f = tmp_path / "lines.txt"
    f.write_text("first line\n\nsecond\n")
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--output", "page", "--seed", "4"])
    assert seen["prompts"] == ["first line", "second"] and seen["source"] == "style.npy" and seen["exp"] == "exp"
    assert seen["output"] == "page" and seen["seed"] == 4 and seen["mode"] == "new"
    assert "page_1.png" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        infer.main(["--prompts-file", str(f)])   # no source
