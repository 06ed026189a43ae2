"""Classifier-free guidance on the host side (no GPU needed): the four new entries are declared, exported and bound and their
handle-less checks answer without a device; every argument rule of ``sample(..., guidance=)`` / ``sample_ddim(..., guidance=)``
and of ``GraphedTrainStep(cond_drop=)`` raises ValueError before any device is touched; the front ends and the two command
lines pass the flags on and refuse the combinations they do not serve; ``null_condition`` is the empty prompt; the CPU helper
the GPU tests use as their yardstick (tests/guide_ref.py) satisfies the identities of the statement; the dropout draw behaves
as a Bernoulli(p) stream on a counter of its own; and the host arithmetic (csrc/guide/guide_host.h) alone under
AddressSanitizer + UBSan."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec
from dhg_amd import train_model as tm
from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402
import cond_ref  # noqa: E402
import ddim_ref  # noqa: E402
import guide_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, Lt, T = 2, 64, 4, 9
TEXT, STYLE = torch.ones((B, Lt), dtype=torch.int64), torch.zeros((B, 14, 1280))


# ---------------------------------------------------------------- the C-ABI
def test_guide_entry_points_are_declared_exported_and_bound():
    for header, names in (("dhw.h", (("dhw_guided_ddim_sample", 17), ("dhw_guided_sample", 15), ("dhw_guide_update", 16))),
                          ("dhw_train.h", (("dhw_train_cond_drop", 10),))):
        with open(os.path.join(ROOT, "include", header)) as f:
            src = f.read()
        for name, nargs in names:
            assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
            assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES
            assert len(_lib.SIGNATURES[name][1]) == nargs
    l = _lib.lib()
    lv, sc = (C.c_int32 * 1)(0), (C.c_float * 1)(1.0)
    # a null handle is refused by the argument checks, which run before any HIP call: these answer without a GPU
    assert l.dhw_guided_ddim_sample(None, None, None, 1, 8, 1, None, 1, lv, 1, sc, None, 0, 0, None, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    assert l.dhw_guided_sample(None, None, None, 1, 8, 1, None, 1, 0, sc, None, 0, 0, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    assert callable(dhg_amd.null_condition) and "cond_drop" in tm.GraphedTrainStep.__init__.__code__.co_varnames


def test_guide_update_checks_answer_without_a_device():
    """dhw_guide_update takes no handle: its refusals are read through dhw_last_error(NULL), each naming its argument."""
    l = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    good = dict(kind=0, base=p, eps2=p, pen=None, lens=None, scale=p, z=None, B=1, L=8, out=p, out3=None)
    cases = [(dict(kind=3), "kind = 3"), (dict(kind=-1), "kind = -1"), (dict(B=0), "B=0"), (dict(L=0), "L=0"), (dict(B=2 ** 15, L=2 ** 15), "below 2^31"),
             (dict(base=None), "(base)"), (dict(eps2=None), "(eps2)"), (dict(scale=None), "(scale)"), (dict(out=None), "out and out3"),
             (dict(out3=p), "(pen"), (dict(z=p), "kind = 0"), (dict(base=p + 4), "base must be 8-byte aligned"), (dict(eps2=p + 4), "eps2 must be 8-byte aligned"),
             (dict(kind=1, z=p + 4), "z must be 8-byte aligned"), (dict(out=p + 4), "out must be 8-byte aligned"), (dict(lens=p + 2), "4-byte aligned"),
             (dict(scale=p + 2), "4-byte aligned")]
    for change, what in cases:
        a = {**good, **change}
        rc = l.dhw_guide_update(a["kind"], a["base"], a["eps2"], a["pen"], a["lens"], a["scale"], a["z"], a["B"], a["L"], 1.0, 0.0, 1.0, 0.0, a["out"], a["out3"], None)
        msg = l.dhw_last_error(None).decode()
        assert rc == -1 and what in msg and "dhw_guide_update" in msg, (what, rc, msg)


def test_cond_drop_checks_answer_without_a_device():
    l = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    good = dict(rng=p, B=1, Lt=4, S=1, p=0.1, ids=p, mask=p, style=p, dropped=p)
    cases = [(dict(B=0), "B = 0"), (dict(Lt=0), "Lt = 0"), (dict(S=0), "S = 0"), (dict(p=-0.1), "p = -0.1"), (dict(p=1.5), "p = 1.5"), (dict(p=float("nan")), "p = "),
             (dict(rng=None), "rng is NULL"), (dict(ids=None), "ids is NULL"), (dict(mask=None), "mask is NULL"), (dict(style=None), "style is NULL"),
             (dict(dropped=None), "dropped is NULL"), (dict(ids=p + 4), "ids must be 8-byte aligned"), (dict(style=p + 8), "style must be 16-byte aligned"),
             (dict(mask=p + 2), "mask must be 4-byte aligned"), (dict(B=2 ** 20, S=2 ** 20), "too large")]
    for change, what in cases:
        a = {**good, **change}
        rc = l.dhw_train_cond_drop(a["rng"], a["B"], a["Lt"], a["S"], a["p"], a["ids"], a["mask"], a["style"], a["dropped"], None)
        msg = l.dhw_train_last_error().decode()
        assert rc == -1 and what in msg and "dhw_train_cond_drop" in msg, (what, rc, msg)


# ---------------------------------------------------------------- null_condition
def test_null_condition_is_the_empty_prompt_then_padding():
    ids = dhg_amd.Tokenizer().encode("")
    assert ids == [1]
    text, style = dhg_amd.null_condition(3, 7)
    assert text.dtype == torch.int64 and text.tolist() == [ids + [0] * 6] * 3 and not (text == 0).all(dim=1).any()
    assert style.dtype == torch.float32 and tuple(style.shape) == (3, 14, 1280) and not style.any()
    assert tuple(dhg_amd.null_condition(1, 1, S=4)[1].shape) == (1, 4, 1280) and dhg_amd.null_condition(1, 1)[0].tolist() == [[1]]
    for bad in (dict(B=0, Lt=4), dict(B=1, Lt=0), dict(B=1, Lt=4, S=0), dict(B=1.0, Lt=4)):
        with pytest.raises(ValueError):
            dhg_amd.null_condition(**bad)
    # what the dropout kernel's statement writes is the same condition
    i2, m2, s2 = guide_ref.apply_drop([1, 0], np.full((2, 7), 5), np.zeros((2, 7), np.float32), np.ones((2, 14, 1280), np.float32))
    assert i2[0].tolist() == text[0].tolist() and m2[0].tolist() == (text[0] == 0).float().tolist() and not s2[0].any()
    assert (i2[1] == 5).all() and not m2[1].any() and s2[1].all()


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


BAD_GUIDANCE = [
    (dict(guidance=-0.5), r"guidance\[0\] = -0.5 must be finite and lie in \[0, 64\]"),
    (dict(guidance=64.5), r"guidance\[0\] = 64.5"),
    (dict(guidance=float("nan")), "must be finite"),
    (dict(guidance=float("inf")), "must be finite"),
    (dict(guidance=[1.0]), "guidance has 1 entries, B = 2"),
    (dict(guidance=[1.0, 2.0, 3.0]), "guidance has 3 entries"),
    (dict(guidance=torch.tensor([1.0, 65.0])), r"guidance\[1\] = 65"),
    (dict(guidance=[1.0, "x"]), r"guidance\[1\] = 'x' is not a number"),
    (dict(guidance=True), "must be a number or a sequence"),
    (dict(guidance="2"), "is not a number|entries"),
    (dict(guidance=2.0, uncond_text=torch.ones((B, Lt + 1), dtype=torch.int64)), r"uncond_text must be \[B,Lt\]"),
    (dict(guidance=2.0, uncond_text=torch.ones((B, Lt))), "uncond_text must be an integer tensor"),
    (dict(guidance=2.0, uncond_style=torch.zeros((B, 13, 1280))), r"uncond_style must be \[B,S,1280\]"),
    (dict(guidance=2.0, uncond_style=torch.zeros((B, 14, 1280), dtype=torch.int32)), "uncond_style must be a floating-point tensor"),
    (dict(uncond_text=TEXT), "belong to a guided call"),
    (dict(uncond_style=STYLE), "belong to a guided call"),
    (dict(guidance=2.0, style=torch.zeros((B, 14, 1279))), "style_vector"),
    (dict(guidance=2.0, text=torch.ones((B, Lt))), "integer tensor"),
    (dict(guidance=2.0, L=60), "multiple of 8"),
    (dict(guidance=2.0, seed=-1), "seed = -1"),
    (dict(guidance=2.0, lengths=[64, 12]), r"lengths\[1\] = 12"),
]
BAD_DDIM = BAD_GUIDANCE + [(dict(guidance=2.0, steps=0), "steps = 0"), (dict(guidance=2.0, latent=torch.zeros((B, L, 3))), r"latent must be \[B,L,2\]")]
BAD_SAMPLE = BAD_GUIDANCE + [
    (dict(guidance=2.0, known=torch.zeros((B, L, 3))), r"guidance cannot be combined with conditioned sampling \(known\)"),
    (dict(guidance=2.0, keep=torch.zeros((B, L), dtype=torch.bool)), r"conditioned sampling \(keep\)"),
    (dict(guidance=2.0, t_start=3), r"conditioned sampling \(t_start\)"),
    (dict(guidance=2.0, cond_noise=torch.zeros((T, B, L, 2))), r"conditioned sampling \(cond_noise\)"),
    (dict(guidance=2.0, noise=torch.zeros((T, B, L, 2))), r"noise must be \[T\+1,B,L,2\]"),
    (dict(guidance=2.0, noise=torch.zeros((T + 1, B, L, 2), dtype=torch.int32)), "noise must be a floating-point tensor"),
    (dict(guidance=2.0, T=0), "T = 0"),
    (dict(guidance=2.0, diffusion_mode="fast"), "diffusion_mode"),
]


@pytest.mark.parametrize("kw,msg", BAD_DDIM)
def test_guided_sample_ddim_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    kw = dict(kw)
    text, style = kw.pop("text", TEXT), kw.pop("style", STYLE)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.sample_ddim(m, text, style, **{**dict(T=T, L=L), **kw})


@pytest.mark.parametrize("kw,msg", BAD_SAMPLE)
def test_guided_sample_rejects_bad_arguments_before_any_device_access(monkeypatch, kw, msg):
    m = _model()
    _no_device(monkeypatch, m)
    kw = dict(kw)
    text, style = kw.pop("text", TEXT), kw.pop("style", STYLE)
    with pytest.raises(ValueError, match=msg):
        dhg_amd.sample(m, text, style, **{**dict(T=T, L=L), **kw})


@pytest.mark.parametrize("kw", [dict(guidance=2.5), dict(guidance=0), dict(guidance=[0.0, 64.0]), dict(guidance=torch.tensor([1.0, 2.0])),
                                dict(guidance=np.float32(3.0), uncond_style=STYLE), dict(guidance=1.5, uncond_text=TEXT, lengths=[8, 64])])
def test_valid_guided_arguments_get_as_far_as_the_device(monkeypatch, kw):
    """... and ask for a handle of 2B rows: the capacity grows as it does for any larger batch."""
    m = _model()
    seen = []

    def boom(dev, B_, *a):
        seen.append(B_)
        raise AssertionError("a device was touched")
    monkeypatch.setattr(m, "_device", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(m, "_ensure_handle", boom)
    for call, extra in ((dhg_amd.sample_ddim, dict(steps=4, return_latent=True)), (dhg_amd.sample, dict(noise=torch.zeros((T + 1, B, L, 2))))):
        with pytest.raises(AssertionError, match="device was touched"):
            call(m, TEXT, STYLE, T=T, L=L, **extra, **kw)
    assert seen == [2 * B, 2 * B]


def test_guided_pair_stacks_the_real_and_the_guidance_condition():
    from dhg_amd import inference
    text = torch.tensor([[5, 6, 0, 0], [7, 1, 0, 0]])
    style = torch.rand((2, 3, 1280))
    t2, s2 = inference._guided_pair(text, style, None, None)
    nt, ns = dhg_amd.null_condition(2, 4, 3)
    assert t2.dtype == torch.int64 and torch.equal(t2, torch.cat((text, nt))) and torch.equal(s2, torch.cat((style, ns)))
    t2, s2 = inference._guided_pair(text, style, None, style)                       # text-only guidance
    assert torch.equal(t2[2:], nt) and torch.equal(s2[2:], style)
    t2, s2 = inference._guided_pair(text, style, torch.flip(text, (0,)), None)
    assert torch.equal(t2[2:], torch.flip(text, (0,))) and not s2[2:].any()


# ---------------------------------------------------------------- the front ends and the command lines
def test_guidance_reaches_the_samplers_through_the_front_ends(monkeypatch):
    from dhg_amd import inference
    calls = []

    def fake(kind):
        def f(model, text, sv, **kw):
            calls.append((kind, text.shape[0], kw))
            return torch.zeros((text.shape[0], kw["L"], 3))
        return f
    monkeypatch.setattr(inference, "sample_ddim", fake("ddim"))
    monkeypatch.setattr(inference, "sample", fake("sample"))
    sv = torch.zeros((1, 14, 1280))
    inference.infer("Hi", sv, None, guidance=2.5)
    inference.infer("Hi", sv, None, steps=4, guidance=0)
    inference.infer_batch(["Hi", "Rabbit"], sv, None, guidance=[1.0, 3.0])
    inference.infer_batch(["Hi"], sv, None, steps=3, guidance=1.5)
    assert [(c[0], c[2]["guidance"]) for c in calls] == [("sample", 2.5), ("ddim", 0), ("sample", [1.0, 3.0]), ("ddim", 1.5)]
    calls.clear()
    inference.infer("Hi", sv, None)
    inference.infer_batch(["Hi"], sv, None, steps=3)
    assert all("guidance" not in c[2] for c in calls)   # without the argument: the call of before, argument for argument
    for bad, msg in ((dict(guidance=2.0, candidates=2), "candidates > 1"), (dict(guidance=-1.0), "must be finite"), (dict(guidance=[1.0, 2.0]), "guidance has 2")):
        with pytest.raises(ValueError, match=msg):
            inference.infer_batch(["Hi"], sv, None, **bad) if "candidates" in bad else inference.infer("Hi", sv, None, **bad)
    with pytest.raises(ValueError, match="candidates > 1"):
        inference.write_page("a b", sv, None, guidance=2.0, candidates=2)

    # write_page: a guided round is half as long, and line i keeps generator index first_sample + i
    class M:
        _cap = dict(max_B=4)
    calls.clear()
    monkeypatch.setattr(dhg_amd.vis, "render_page", lambda *a, **k: (torch.zeros((1, 1, 8, 8)), None, None))
    inference.write_page("aa bb cc dd ee", sv, M(), max_chars=2, guidance=2.0, first_sample=10, height=200, width=200, lines_per_page=5, pitch=20.0,
                         margin_left=10.0, margin_top=10.0)
    assert [(c[1], c[2]["first_sample"], c[2]["guidance"]) for c in calls] == [(2, 10, 2.0), (2, 12, 2.0), (1, 14, 2.0)]
    calls.clear()
    inference.write_page("aa bb cc dd ee", sv, M(), max_chars=2, first_sample=10, height=200, width=200, lines_per_page=5, pitch=20.0, margin_left=10.0,
                         margin_top=10.0)
    assert [(c[1], c[2]["first_sample"]) for c in calls] == [(4, 10), (1, 14)] and all("guidance" not in c[2] for c in calls)


def test_file_front_ends_size_the_model_for_both_halves(monkeypatch):
    from dhg_amd import checkpoint, inference
    seen = {}

    def fake_load(config_path, checkpoint_path, **kw):
        seen.update(kw)
        return None
    monkeypatch.setattr(checkpoint, "load_model", fake_load)
    monkeypatch.setattr(inference, "load_style", lambda *a: torch.zeros((1, 14, 1280)))
    monkeypatch.setattr(inference, "infer", lambda *a, **k: seen.update(one=k) or np.zeros((8, 3), np.float32))
    monkeypatch.setattr(inference, "infer_batch", lambda p, *a, **k: seen.update(batch=k) or [np.zeros((8, 3), np.float32) for _ in p])
    inference.infer_file("Hi", "s.npy", "c.yml", "m.pth", render=False, guidance=2.0)
    assert seen["max_B"] == 2 and seen["one"]["guidance"] == 2.0
    inference.infer_file_batch(["a", "b", "c"], "s.npy", "c.yml", "m.pth", render=False, guidance=2.0, steps=5)
    assert seen["max_B"] == 6 and seen["batch"]["guidance"] == 2.0 and seen["batch"]["steps"] == 5
    inference.infer_file("Hi", "s.npy", "c.yml", "m.pth", render=False)
    inference.infer_file_batch(["a", "b", "c"], "s.npy", "c.yml", "m.pth", render=False)
    assert seen["max_B"] == 3 and "guidance" not in seen["one"] and "guidance" not in seen["batch"]
    for call, args in ((inference.infer_file, ("Hi",)), (inference.infer_file_batch, (["a"],)), (inference.write_page_file, ("a b",))):
        with pytest.raises(ValueError, match="candidates > 1"):
            call(*args, "s.npy", "c.yml", "m.pth", guidance=2.0, candidates=2)
        with pytest.raises(ValueError, match="must be finite"):
            call(*args, "s.npy", "c.yml", "m.pth", guidance=65.0)


def test_infer_cli_guidance_dispatch(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}
    fake = lambda key, ret: lambda first, *a, **kw: seen.update({key: first}, **kw) or ret(first)   # noqa: E731
    monkeypatch.setattr(dhg_amd, "infer_file_batch", fake("batch", lambda p: [np.zeros((8, 3), np.float32) for _ in p]))
    monkeypatch.setattr(dhg_amd, "infer_file", fake("one", lambda p: np.zeros((8, 3), np.float32)))
    monkeypatch.setattr(dhg_amd, "write_page_file", fake("page", lambda p: [np.zeros((8, 3), np.float32)]))
    f = tmp_path / "lines.txt"
    f.write_text("first line\nsecond\n")
    infer.main(["a prompt", "style.npy", "--experiment-path", "exp", "--guidance", "2.5"])
    assert seen["guidance"] == 2.5 and seen["one"] == "a prompt" and "steps" not in seen
    seen.clear()
    infer.main(["a prompt", "style.npy", "--experiment-path", "exp", "--guidance", "0", "--steps", "7"])
    assert seen["guidance"] == 0.0 and seen["steps"] == 7
    seen.clear()
    infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--guidance", "3"])
    assert seen["guidance"] == 3.0 and seen["batch"] == ["first line", "second"]
    seen.clear()
    infer.main(["--page-file", str(f), "style.npy", "--experiment-path", "exp", "--guidance", "1.5", "--steps", "4"])
    assert seen["guidance"] == 1.5 and seen["steps"] == 4 and "first line" in seen["page"]
    for argv in (["--prompts-file", str(f), "style.npy"], ["a prompt", "style.npy"], ["--page-file", str(f), "style.npy"]):
        seen.clear()
        infer.main(argv + ["--experiment-path", "exp"])
        assert "guidance" not in seen   # without the flag: the call of before, argument for argument
    for bad in (["--guidance", "-1"], ["--guidance", "65"], ["--guidance", "nan"], ["--guidance", "x"], ["--guidance", "2", "--score", "old.npy"],
                ["--guidance", "2", "--align", "old.npy"], ["--guidance", "2", "--restyle", "old.npy"], ["--guidance", "2", "--candidates", "3"]):
        with pytest.raises(SystemExit):
            infer.main(["--prompts-file", str(f), "style.npy", *bad])


def test_train_py_cond_drop_reaches_fit(monkeypatch):
    spec_ = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(cli)
    calls = []
    monkeypatch.setattr(tm, "fit", lambda *a, **k: calls.append((a, k)))
    cli.main(["--config", "c.yml", "--cond-drop", "0.1"])
    cli.main(["--config", "c.yml"])
    assert calls[0][1]["cond_drop"] == 0.1 and calls[1][1]["cond_drop"] == 0.0
    for bad in ("-0.1", "1.5", "x"):
        with pytest.raises(SystemExit):
            cli.main(["--config", "c.yml", "--cond-drop", bad])
    monkeypatch.undo()
    import inspect
    assert inspect.signature(tm.fit).parameters["cond_drop"].default == 0.0 and list(inspect.signature(tm.read_train_config).parameters) == ["config_path"]


def test_graphed_step_checks_cond_drop_before_any_device_access(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    for name in ("is_available", "current_device", "mem_get_info"):
        monkeypatch.setattr(torch.cuda, name, boom)
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(ValueError, match="needs device_rng=True"):
        tm.GraphedTrainStep(None, None, 2, 8, 4, device_rng=False, cond_drop=0.1)
    for bad in (-0.1, 1.5, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="cond_drop = "):
            tm.GraphedTrainStep(None, None, 2, 8, 4, cond_drop=bad)


# ---------------------------------------------------------------- the helper, proven before it is used as a yardstick
def _small():
    sd = {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}
    inp = spec.synthetic_inputs(2, 16, 5, seed=11, pad=1, T=1)
    g = torch.Generator().manual_seed(12)
    text, style = torch.from_numpy(inp["text"]), torch.from_numpy(inp["style"])
    utext, ustyle = dhg_amd.null_condition(2, 5, style.shape[1])
    return sd, text, style, utext, ustyle, torch.randn((2, 16, 2), generator=g), torch.randn((4, 2, 16, 2), generator=g)


def test_guide_ref_at_scale_one_and_zero_is_the_unguided_reference():
    """The statement's identities, exactly: scale 1 is the conditional run (as values: a -0 may become +0), scale 0 is the run
    under the guidance condition, and a row does not depend on the other rows' scales."""
    sd, text, style, utext, ustyle, latent, noise = _small()
    lv, T_ = [2, 0], 3
    plain_c = ddim_ref.sample(ref_cpu.forward, sd, text, style, lv, T_, latent)
    plain_u = ddim_ref.sample(ref_cpu.forward, sd, utext, ustyle, lv, T_, latent)
    g1 = guide_ref.sample_ddim(ref_cpu.forward, sd, text, style, utext, ustyle, 1.0, lv, T_, latent)
    g0 = guide_ref.sample_ddim(ref_cpu.forward, sd, text, style, utext, ustyle, 0.0, lv, T_, latent)
    mix = guide_ref.sample_ddim(ref_cpu.forward, sd, text, style, utext, ustyle, [1.0, 0.0], lv, T_, latent)
    assert np.array_equal(g1.numpy(), plain_c.numpy()) and np.array_equal(g0[..., :2].numpy(), plain_u[..., :2].numpy())
    assert np.array_equal(mix[0].numpy(), plain_c[0].numpy()) and np.array_equal(mix[1, :, :2].numpy(), plain_u[1, :, :2].numpy())
    assert not np.array_equal(plain_c.numpy(), plain_u.numpy())
    for mode in ("new", "standard"):
        a_c = cond_ref.cond_sample(ref_cpu.forward, sd, text, style, 16, noise, T=T_, mode=mode)
        a_u = cond_ref.cond_sample(ref_cpu.forward, sd, utext, ustyle, 16, noise, T=T_, mode=mode)
        s1 = guide_ref.sample(ref_cpu.forward, sd, text, style, utext, ustyle, 1.0, 16, noise, T_, mode)
        s0 = guide_ref.sample(ref_cpu.forward, sd, text, style, utext, ustyle, 0.0, 16, noise, T_, mode)
        assert np.array_equal(s1.numpy(), a_c.numpy()) and np.array_equal(s0[..., :2].numpy(), a_u[..., :2].numpy()), mode
    # lengths: each sample alone
    rag = guide_ref.sample_ddim(ref_cpu.forward, sd, text, style, utext, ustyle, 2.5, lv, T_, latent, lengths=[8, 16])
    alone = guide_ref.sample_ddim(ref_cpu.forward, sd, text[:1], style[:1], utext[:1], ustyle[:1], 2.5, lv, T_, latent[:1, :8])
    assert torch.equal(rag[0, :8], alone[0]) and not rag[0, 8:].any()


def test_guide_ref_pen_is_the_conditional_rows_and_the_combine_is_the_closed_form():
    """A denoiser that answers fixed (e_c, e_u) whatever x: x(S) = x(0) / A_0 - (B_0 / A_0) e in exact arithmetic (the steps
    telescope: x(j+1)/A_{j+1} = x(j)/A_j + (B_{j+1}/A_{j+1} - B_j/A_j) e, A_S = 1, B_S = 0), e = e_c + (w - 1)(e_c - e_u).  The
    bound is derived: S updates of 5 float32 operations and a combine of 3, each rounding a value no larger than
    M = (|x(0)| + |e|) / A_0 by at most 2^-24 relative, amplified by at most 1 / A_0 on the way down -> 8 S 2^-24 M / A_0, doubled."""
    g = torch.Generator().manual_seed(5)
    e_c, e_u, q_c, q_u = torch.randn((2, 16, 2), generator=g), torch.randn((2, 16, 2), generator=g), torch.rand((2, 16), generator=g), torch.rand((2, 16), generator=g)
    x0 = torch.randn((2, 16, 2), generator=g)
    utext, ustyle = dhg_amd.null_condition(2, 5)
    text, style = torch.full((2, 5), 7), torch.ones((2, 14, 1280))

    def fixed(sd, x, t, sigma, s):
        return (e_u, q_u) if not s.any() else (e_c, q_c)
    T_, lv = 9, [8, 5, 2, 0]
    co = ddim_ref.coefs(lv, T_)
    A0, B0 = float(co[0][0]), float(co[0][1])
    for w in ([2.5, 2.5], [0.0, 7.0], [1.0, 64.0]):
        got = guide_ref.sample_ddim(fixed, None, text, style, utext, ustyle, w, lv, T_, x0)
        wv = torch.tensor(w, dtype=torch.float64).reshape(2, 1, 1)
        e = e_c.double() + (wv - 1) * (e_c.double() - e_u.double())
        want = x0.double() / A0 - (B0 / A0) * e
        M = float((x0.abs().double() + e.abs()).max()) / A0
        bound = 2 * 8 * len(lv) * 2.0 ** -24 * M / A0
        err = float((got[..., :2].double() - want).abs().max())
        assert err <= bound, (w, err, bound)
        assert torch.equal(got[..., 2], q_c)
    # the combine itself, against numpy float32, with the select at w = 0
    w = torch.tensor([0.0, 1.0, 2.5, 64.0]).reshape(4, 1, 1)
    a, b = torch.randn((4, 3, 2), generator=g), torch.randn((4, 3, 2), generator=g) * 1e-3
    got = guide_ref.combine(a, b, w).numpy()
    an, bn, wn = a.numpy(), b.numpy(), w.numpy()
    want = an + (wn - np.float32(1)) * (an - bn)
    assert want.dtype == np.float32 and np.array_equal(got[1:], want[1:]) and np.array_equal(got[0], bn[0]) and np.array_equal(got[1], an[1])
    assert not np.array_equal(want[0], bn[0])   # why w = 0 is a select: e_c - fl(e_c - e_u) is not e_u


# ---------------------------------------------------------------- the dropout statement
def test_cond_drop_draw_is_a_bernoulli_stream_on_its_own_counter():
    """4096 streams at p = 0.1, seed fixed (so the check is deterministic): the count lies inside the 4-sigma binomial interval
    409.6 +- 4 sqrt(4096 * 0.1 * 0.9) = [332.8, 486.4]; p = 0 drops none, p = 1 all; the words are not the batch draw's."""
    N, seed, index = 4096, 20240, 3
    d = guide_ref.cond_drop(seed, index, N, 0.1)
    sigma = (N * 0.1 * 0.9) ** 0.5
    assert abs(int(d.sum()) - N * 0.1) <= 4 * sigma, int(d.sum())
    assert not guide_ref.cond_drop(seed, index, N, 0.0).any() and guide_ref.cond_drop(seed, index, N, 1.0).all()
    assert np.array_equal(d, guide_ref.cond_drop(seed, index, N, 0.1))
    assert not np.array_equal(d, guide_ref.cond_drop(seed + 1, index, N, 0.1)) and not np.array_equal(d, guide_ref.cond_drop(seed, index + 1, N, 0.1))
    # monotone in p: the same u decides
    assert (guide_ref.cond_drop(seed, index, N, 0.5) >= d).all()
    # sample b of draw d is stream d * B + b
    assert np.array_equal(guide_ref.cond_drop(seed, 1, 8, 0.3), guide_ref.cond_drop(seed, 0, 16, 0.3)[8:])
    # independent of the batch draw's words for the same stream: another counter, so no word is shared, and the drop decision is
    # uncorrelated with the batch draw's first word (|corr| within 4 / sqrt(N) of 0)
    drop_w = guide_ref.drop_words(seed, index, N)
    batch_w = []
    for b in range(N):
        stream = index * N + b
        batch_w.append(batch_ref.philox4x32_10((stream & batch_ref.M32, stream >> 32, 0, 0), (seed & batch_ref.M32, seed >> 32)))
    assert not set(w for ws in drop_w for w in ws) & set(w for ws in batch_w for w in ws)
    u_batch = np.array([w[0] for w in batch_w], np.float64) / 2.0 ** 32
    corr = np.corrcoef(d.astype(np.float64), u_batch)[0, 1]
    assert abs(corr) <= 4 / N ** 0.5, corr
    idx = batch_ref.draw(seed, index, 1000, 64, np.linspace(0.9, 0.1, 10, dtype=np.float32))[0]
    assert len(idx) == 64   # (the batch draw is what it was: its reference is unchanged)


# ---------------------------------------------------------------- the host arithmetic of the guided entries, alone, under ASan + UBSan
def test_guide_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/guide_host_check.cpp (csrc/guide/guide_host.h only) built with the host compiler under AddressSanitizer + UBSan
    where the toolchain links them (as tests/test_ddim_cpu.py builds its program), run on the CPU: the coefficients of every
    ancestral step against numpy bit for bit, every refusal, and (inside the program) a message buffer shorter than the message."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "guide_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "guide_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("guide_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    Tq = 9
    beta, abar = _lib.schedule(Tq)
    beta.tofile(tmp_path / "beta.f32")
    abar.tofile(tmp_path / "abar.f32")

    def run(mode=0, kind=0, B_=2, L_=16, max_B=4, scales=("1", "2.5")):
        r = subprocess.run([exe, str(tmp_path / "beta.f32"), str(tmp_path / "abar.f32"), str(Tq), str(mode), str(kind), str(B_), str(L_), str(max_B), *scales],
                           capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return r.stdout.strip().splitlines()

    one = np.float32(1.0)
    for mode in (0, 1):
        lines = run(mode=mode)
        assert len(lines) == Tq
        for ln, i in zip(lines, range(Tq - 1, -1, -1)):
            f = ln.split()
            got = [np.float32(float.fromhex(v)) for v in f[1:5]] + [int(f[5])] + [np.float32(float.fromhex(v)) for v in f[6:8]]
            a, b = abar[i], beta[i]
            a_next = abar[i - 1] if i > 1 else one
            if mode == 0:
                want = [np.sqrt(one - a), np.sqrt(one - b), np.sqrt(one - a_next), np.float32(0), 1]
            else:
                want = [np.sqrt(one - a), one / np.sqrt(one - b), np.sqrt(b), b, int(i != 0)]
            want += [np.sqrt(a), np.sqrt(abar[i - 1]) if i > 0 else np.float32(0)]
            assert f[0] == "st" and got == want, (mode, i, got, want)
    for kw, what in ((dict(kind=3), "kind = 3"), (dict(kind=-1), "kind = -1"), (dict(scales=("1", "-0.5")), "scale[1] = -0.5"), (dict(scales=("64.5", "1")), "scale[0] = 64.5"),
                     (dict(scales=("1", "nan")), "scale[1] = nan"), (dict(scales=("inf", "1")), "scale[0] = inf"), (dict(scales=()), "null pointer (scale)"),
                     (dict(B_=3, max_B=5), "2B = 6 rows through the denoiser, the handle holds max_B = 5"), (dict(B_=0, scales=()), "null pointer"),
                     (dict(B_=1, max_B=1, scales=("1",)), "2B = 2"), (dict(B_=2 ** 15, L_=2 ** 15, max_B=2 ** 16), "2 * B * L below 2^31")):
        out = run(**kw)
        assert len(out) == 1 and out[0].startswith("err ") and what in out[0], (kw, out)
    assert len(run(B_=2, max_B=4, scales=("0", "64"))) == Tq
