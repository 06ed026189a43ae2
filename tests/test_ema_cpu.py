"""EMA weights in the optimizer pass, the full training state and the held-out loss (include/dhw_train.h dhw_train_adam_ema_dev;
train.Adam(ema_decay=), train_model.save_train_state / load_train_state / EvalStep, fit(ema=, save_state=, resume=, val_path=,
eval_freq=), train.py --ema / --save-state / --resume / --val / --eval-freq), what needs no GPU: the symbol, the entry's handle-less
argument rules, the warm-up rule, every refusal of a bad decay, the command line, the state file's round trip on CPU stand-ins with
each mismatch it must name, and the ValueErrors that are raised before a device is touched."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import dhg_amd  # noqa: F401
from dhg_amd import _lib, train, train_model as tm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


# ---------------------------------------------------------------- the C entry
def test_symbol_is_declared_exported_and_bound_with_11_arguments():
    hdr = open(os.path.join(ROOT, "include", "dhw_train.h")).read()
    assert re.search(r"\bint dhw_train_adam_ema_dev\(", hdr)
    assert "dhw_train_adam_ema_dev" in _lib.SIGNATURES and hasattr(_lib.lib(), "dhw_train_adam_ema_dev")
    assert len(_lib.SIGNATURES["dhw_train_adam_ema_dev"][1]) == 11
    assert len(_lib.SIGNATURES["dhw_train_adam_dev"][1]) == 9                      # the plain entry keeps its signature
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "train.hip")).read()
    assert src.count("adam_element(h, ") >= 3                                       # one statement of the element update, both kernels call it


def _entry(**kw):
    one = lambda: (C.c_void_p * 1)(FAKE)   # noqa: E731
    a = dict(nbuf=1, p=one(), g=one(), m=one(), v=one(), ema=one(), n=(C.c_int64 * 1)(8), hyper=FAKE, ema_hyper=FAKE, sqnorm=FAKE)
    a.update(kw)
    l = _lib.lib()
    rc = l.dhw_train_adam_ema_dev(*a.values(), None)
    return rc, l.dhw_train_last_error().decode()


@pytest.mark.parametrize("bad,msg", [(dict(ema=None), "ema is NULL"), (dict(ema_hyper=None), "ema_hyper is NULL"), (dict(nbuf=0), "nbuf = 0"),
                                     (dict(nbuf=-3), "nbuf = -3"), (dict(p=None), "bad argument"), (dict(sqnorm=None), "bad argument"),
                                     (dict(ema=(C.c_void_p * 1)(None)), "buffer 0")])
def test_the_entrys_null_and_nbuf_rules_answer_without_a_device(bad, msg):
    rc, err = _entry(**bad)
    assert rc == -1 and err.startswith("dhw_train_adam_ema_dev:") and msg in err, (bad, rc, err)


# ---------------------------------------------------------------- the host rules
def test_ema_decay_at_warms_up_and_caps():
    for t, want in ((1, 2 / 11), (2, 0.25), (10, 0.55), (10 ** 5, 0.9999)):
        assert train.ema_decay_at(t, 0.9999) == want == ema_ref.ema_decay_at(t, 0.9999), t
    assert train.ema_decay_at(1, 0.1) == 0.1                                        # a decay under the warm-up value is the cap at once


def test_ema_hyper_rounds_decay_and_its_complement_separately():
    ad = train.Adam([torch.zeros(3)], ema_decay=0.9999)
    assert ad.ema is not None and ad.ema[0].data_ptr() != ad.params[0].data_ptr() and len(ad.hyper(1e-3)) == 9
    assert ad.ema_hyper() == [float(np.float32(2 / 11)), float(np.float32(9 / 11))]
    ad.step_count = 10 ** 6
    d, omd = ad.ema_hyper()
    assert d == float(np.float32(0.9999)) and omd == float(np.float32(1.0 - 0.9999)) and omd != float(np.float32(1) - np.float32(0.9999))
    plain = train.Adam([torch.zeros(3)])
    assert plain.ema is None and plain.ema_decay is None
    with pytest.raises(ValueError, match="keeps no EMA"):
        plain.ema_hyper()
    with pytest.raises(ValueError, match="ema_hyper_dev goes with"):
        plain.step_dev([torch.zeros(3)], torch.zeros(9), torch.zeros(1), torch.zeros(2))
    with pytest.raises(ValueError, match="ema_hyper_dev goes with"):
        ad.step_dev([torch.zeros(3)], torch.zeros(9), torch.zeros(1))


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    for name in ("is_available", "current_device", "mem_get_info"):
        monkeypatch.setattr(torch.cuda, name, boom)
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("bad", [True, False, "0.999", float("nan"), 0, 0.0, -0.5, 1, 1.0, 1.5, float("inf"), [0.9]])
def test_every_bad_ema_decay_raises_before_a_device_is_touched(monkeypatch, bad):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="ema_decay = .* must be None or a number in \\(0, 1\\)"):
        train.Adam([torch.zeros(3)], ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        tm.fit("missing.yml", None, ema=bad)


def test_adam_step_with_host_scalars_refuses_an_ema_optimizer(monkeypatch):
    _no_device(monkeypatch)
    ad = train.Adam([torch.zeros(3)], ema_decay=0.5)
    with pytest.raises(ValueError, match="step_dev"):
        ad.step([torch.zeros(3)], 1e-3)
    assert ad.step_count == 0


# ---------------------------------------------------------------- the command line
def test_train_py_flags_reach_fit(monkeypatch):
    spec_ = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(cli)
    calls = []
    monkeypatch.setattr(tm, "fit", lambda *a, **k: calls.append((a, k)))
    cli.main(["--config", "c.yml"])
    cli.main(["--config", "c.yml", "--ema", "0.9999", "--save-state", "--val", "v.pt", "--eval-freq", "500"])
    cli.main(["--config", "c.yml", "--resume", "run/train_state.pth"])
    off, on, res = (c[1] for c in calls)
    assert (off["ema"], off["save_state"], off["resume"], off["val_path"], off["eval_freq"]) == (None, False, None, None, None)
    assert (on["ema"], on["save_state"], on["resume"], on["val_path"], on["eval_freq"]) == (0.9999, True, None, "v.pt", 500)
    assert res["resume"] == "run/train_state.pth" and res["save_state"] is True               # --resume implies --save-state
    for bad in (["--ema", "1"], ["--ema", "0"], ["--ema", "x"], ["--eval-freq", "5"], ["--val", "v.pt", "--eval-freq", "0"]):
        with pytest.raises(SystemExit):
            cli.main(["--config", "c.yml", *bad])
    monkeypatch.undo()
    par = inspect.signature(tm.fit).parameters
    assert [par[k].default for k in ("ema", "save_state", "resume", "val_path", "eval_freq")] == [None, False, None, None, None]


# ---------------------------------------------------------------- the state file
def _stand_ins(ema_decay=0.999, seed=0, precision="fp32"):
    g = torch.Generator().manual_seed(seed)
    layout, sizes = ["b.weight", "a.bias", "c.weight"], {"b.weight": 12, "a.bias": 4, "c.weight": 5}
    model = types.SimpleNamespace(flat=torch.randn(21, generator=g), layout=layout, sizes=sizes, precision=precision)
    opt = train.Adam([model.flat], ema_decay=ema_decay)
    opt.m[0].copy_(torch.randn(21, generator=g))
    opt.v[0].copy_(torch.randn(21, generator=g).abs())
    if opt.ema is not None:
        opt.ema[0].copy_(torch.randn(21, generator=g))
    opt.step_count = 7 + seed
    return model, opt


def _bits(t):
    return t.view(torch.int32)


def test_state_round_trips_bit_for_bit_in_place_and_leaves_no_tmp(tmp_path):
    model, opt = _stand_ins()
    path = tmp_path / "train_state.pth"
    gen = torch.Generator().manual_seed(5)
    tm.save_train_state(path, model, opt, 7, {"gen": gen.get_state(), "torch": torch.get_rng_state()})
    assert os.listdir(tmp_path) == ["train_state.pth"]                                      # the .tmp file was moved into place
    raw = torch.load(path, weights_only=True)                                               # tensors and plain containers only
    assert set(raw) == {"format", "count", "step_count", "flat", "m", "v", "ema", "ema_decay", "layout", "optim", "precision", "host_rng"}
    assert raw["format"] == 1 and raw["count"] == 7 and raw["step_count"] == 7 and raw["ema_decay"] == 0.999 and raw["precision"] == "fp32"
    assert [tuple(x) for x in raw["layout"]] == [("b.weight", 12), ("a.bias", 4), ("c.weight", 5)]
    assert raw["optim"] == {"betas": [0.9, 0.98], "eps": 1e-8, "weight_decay": 1e-5, "max_norm": 100.0}
    assert torch.equal(raw["host_rng"]["gen"], gen.get_state())
    fresh, fopt = _stand_ins(seed=1)
    addr = [t.data_ptr() for t in (fresh.flat, fopt.m[0], fopt.v[0], fopt.ema[0])]
    assert not torch.equal(fresh.flat, model.flat) and fopt.step_count == 8
    assert tm.load_train_state(path, fresh, fopt) == 7
    assert [t.data_ptr() for t in (fresh.flat, fopt.m[0], fopt.v[0], fopt.ema[0])] == addr  # copied INTO the buffers a graph may hold
    for a, b in ((fresh.flat, model.flat), (fopt.m[0], opt.m[0]), (fopt.v[0], opt.v[0]), (fopt.ema[0], opt.ema[0])):
        assert torch.equal(_bits(a), _bits(b))
    assert fopt.step_count == 7
    # without an EMA on both sides: ema None in the file
    m2, o2 = _stand_ins(ema_decay=None)
    tm.save_train_state(path, m2, o2, 0)
    assert torch.load(path, weights_only=True)["ema"] is None and tm.load_train_state(path, *_stand_ins(ema_decay=None, seed=2)) == 0
    with pytest.raises(ValueError, match="count = "):
        tm.save_train_state(path, m2, o2, -1)


def _saved(tmp_path, **change):
    model, opt = _stand_ins()
    path = tmp_path / "s.pth"
    tm.save_train_state(path, model, opt, 3)
    state = torch.load(path, weights_only=True)
    state.update(change)
    torch.save(state, path)
    return path


MISMATCH = [
    (dict(format=2), {}, "`format`"),
    (dict(layout=[("b.weight", 12), ("a.bias", 4), ("c.weight", 6)]), {}, "`layout`"),
    (dict(layout=[("a.bias", 4), ("b.weight", 12), ("c.weight", 5)]), {}, "`layout`"),
    (dict(optim={"betas": [0.9, 0.999], "eps": 1e-8, "weight_decay": 1e-5, "max_norm": 100.0}), {}, "`optim`"),
    (dict(optim={"betas": [0.9, 0.98], "eps": 1e-8, "weight_decay": 1e-5, "max_norm": 0.0}), {}, "`optim`"),
    (dict(precision="bf16"), {}, "`precision`"),
    (dict(ema=None), {}, "`ema`"),
    ({}, dict(ema_decay=None), "`ema`"),
    (dict(ema_decay=0.9999), {}, "`ema_decay`"),
    (dict(count=-1), {}, "`count`"),
    (dict(count=2.0), {}, "`count`"),
    (dict(step_count=True), {}, "`step_count`"),
    (dict(step_count=None), {}, "`step_count`"),
    (dict(m=torch.zeros(20)), {}, "`m`"),
]


@pytest.mark.parametrize("k", range(len(MISMATCH)))
def test_each_mismatch_raises_naming_its_key_and_writes_nothing(tmp_path, k):
    change, here, key = MISMATCH[k]
    path = _saved(tmp_path, **change)
    model, opt = _stand_ins(seed=1, **here)
    before = [t.clone() for t in (model.flat, opt.m[0], opt.v[0])]
    with pytest.raises(ValueError, match=key):
        tm.load_train_state(path, model, opt)
    assert all(torch.equal(a, b) for a, b in zip(before, (model.flat, opt.m[0], opt.v[0]))) and opt.step_count == 8


# ---------------------------------------------------------------- refusals before any device access
def test_fit_resume_on_a_missing_file_raises_before_any_device_access(monkeypatch, tmp_path):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="no training state at"):
        tm.fit("missing.yml", None, tmp_path / "run", resume=tmp_path / "nowhere.pth")
    with pytest.raises(ValueError, match="needs val_path"):
        tm.fit("missing.yml", None, eval_freq=5)
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="eval_freq"):
            tm.fit("missing.yml", None, val_path="v.pt", eval_freq=bad)
    assert not (tmp_path / "run").exists()


def test_eval_step_checks_its_arguments_before_any_device_access(monkeypatch):
    _no_device(monkeypatch)
    rd = types.SimpleNamespace(N=5, L=64, Lt=10, S=14, max_token=1)
    with pytest.raises(ValueError, match="holds 5 rows, fewer than one batch of B = 6"):
        tm.EvalStep(None, rd, 6)
    for levels, msg in (((7, 60), r"levels\[1\] = 60 must lie in \[0, T = 60\)"), ((), "levels is empty"), ((1.5,), "is not an integer"), (3, "must be a sequence")):
        with pytest.raises(ValueError, match=msg):
            tm.EvalStep(None, rd, 2, levels=levels)
    with pytest.raises(ValueError, match="B = 0"):
        tm.EvalStep(None, rd, 0)
    with pytest.raises(ValueError, match="T = 0"):
        tm.EvalStep(None, rd, 2, T=0)
    from dhg_amd.inference import default_levels
    assert default_levels(60) == [7, 22, 37, 52]
