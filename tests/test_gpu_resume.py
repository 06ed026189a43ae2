"""The full training state on the GPU: save_train_state / load_train_state around a resident GraphedTrainStep with an EMA optimizer — a
resumed run lands where the uninterrupted one does, and a resume that forgets Adam's moments does not — and fit() with ema, save_state,
a validation set and resume."""
import os

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import spec, train, train_model as tm

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L, LT, S, N = 2, 64, 10, 14, 9


def _dataset(n, l, lt, seed):
    g = torch.Generator().manual_seed(seed)
    strokes = torch.cat([torch.randn(n, l, 2, generator=g), (torch.rand(n, l, 1, generator=g) < 0.2).float()], dim=-1)
    text = torch.randint(1, spec.VOCAB, (n, lt), generator=g)
    text[:, lt - 2:] = 0
    return {"strokes": strokes, "text": text, "style": torch.randn(n, S, 1280, generator=g).abs()}


def _build(sd, rd, abar):
    model = tm.TrainModel(sd, num_layers=2, device=DEV, drop_rate=0.1)
    opt = train.Adam(model.parameters(), ema_decay=0.999)
    return model, opt, tm.GraphedTrainStep(model, opt, B, L, LT, warmup=100, seed=7, data=rd, alpha_set=abar)


def _snap(model, opt):
    return {"flat": model.flat.cpu(), "m": opt.m[0].cpu(), "v": opt.v[0].cpu(), "ema": opt.ema[0].cpu()}


def _bits(t):
    return t.view(torch.int32)


def test_a_resumed_run_lands_where_the_uninterrupted_one_does_and_forgotten_moments_show(tmp_path):
    """Run A: updates 1-4.  Run B: updates 1-2, save; a FRESH model, optimizer and step from the initial weights, load, updates 3-4.
    (The first two updates of A and B are the same execution: the state is saved from A's objects after update 2, and A goes on.)
    Right after the load every buffer holds the saved bits.  Updates 3-4 then agree as two runs of the same update do: losses to 2e-6,
    parameters and EMA to (L2 difference) < 1e-3 x (L2 displacement from the initial weights).  Control: the same resume with m and v
    zeroed after the load must VIOLATE that bound, which shows the criterion sees a forgotten moment; and updates 3-4 repeated from
    the saved state on A's own objects give the run-to-run ratio the criterion has to leave room for (printed)."""
    d = _dataset(N, L, LT, seed=5)
    d["writer"] = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2])
    sd, abar = spec.synthetic_state_dict(2, 128, 192, 256, seed=0), dhg_amd.get_alpha_set(60).float()
    rd = tm.ResidentData(d, DEV)
    path = tmp_path / "train_state.pth"

    model_a, opt_a, step_a = _build(sd, rd, abar)
    p0 = model_a.flat.cpu().double()
    for n in (1, 2):
        step_a(step=n)
    tm.save_train_state(path, model_a, opt_a, 2)
    saved = _snap(model_a, opt_a)
    assert opt_a.step_count == 2 and os.listdir(tmp_path) == ["train_state.pth"]
    loss_a = [step_a(step=n).cpu().numpy() for n in (3, 4)]
    end_a = _snap(model_a, opt_a)

    def resume_on(model, opt, step, forget=False):
        assert tm.load_train_state(path, model, opt) == 2 and opt.step_count == 2
        now = _snap(model, opt)
        assert all(torch.equal(_bits(now[k]), _bits(saved[k])) for k in saved), "the loaded buffers are not the saved bits"
        if forget:
            opt.m[0].zero_()
            opt.v[0].zero_()
        losses = [step(step=n).cpu().numpy() for n in (3, 4)]
        return losses, _snap(model, opt)

    model_b, opt_b, step_b = _build(sd, rd, abar)
    assert opt_b.step_count == 0 and torch.equal(model_b.flat.cpu().double(), p0)
    loss_b, end_b = resume_on(model_b, opt_b, step_b)
    _, end_forgot = resume_on(model_b, opt_b, step_b, forget=True)        # (in place again: the captured graph holds the addresses)
    _, end_again = resume_on(model_a, opt_a, step_a)                      # A's own objects, updates 3-4 once more

    def ratio(x, y, k):
        return float(np.linalg.norm((x[k].double() - y[k].double()).numpy())) / float(np.linalg.norm((y[k].double() - p0).numpy()))

    r = {name: {k: ratio(e, end_a, k) for k in ("flat", "ema")} for name, e in (("resumed", end_b), ("repeat", end_again), ("forgot m, v", end_forgot))}
    print("L2 difference / displacement against run A:", r)
    assert np.allclose(np.array(loss_b), np.array(loss_a), rtol=2e-6, atol=0), (loss_a, loss_b)
    for k in ("flat", "ema"):
        assert r["resumed"][k] < 1e-3 and r["repeat"][k] < 1e-3, (k, r)
    assert r["forgot m, v"]["flat"] >= 1e-3, ("the criterion does not see a forgotten moment", r)


def test_fit_with_ema_state_validation_and_resume(tmp_path):
    cfg = tmp_path / "cfg.yml"
    cfg.write_text("""
experiment: {seed: 1}
dataset_args: {max_seq_len: 64, max_text_len: 8}
training_args: {steps: 4, batch_size: 2, warmup_steps: 100, clip_grad: 100.0, dropout: 0.1, att_layers_num: 2, channels: 128, log_freq: 2, save_freq: 2}
optimizer: {type: torch.optim.Adam, params: {lr: 0.0003, weight_decay: 0.00001, betas: [0.9, 0.98]}}
""")
    d = _dataset(12, 64, 8, seed=8)
    d["writer"] = torch.arange(12) // 3
    torch.save(d, tmp_path / "batches.pt")
    torch.save(_dataset(4, 64, 8, seed=9), tmp_path / "val.pt")
    run = tmp_path / "run"
    lines = []
    tm.fit(cfg, tmp_path / "batches.pt", run, log=lines.append, resident=True, ema=0.999, save_state=True, val_path=tmp_path / "val.pt")
    print("\n".join(lines))
    assert [ln.split(" | ")[0] for ln in lines] == ["Step 2", "Eval 2", "Eval 2 (ema)", "Step 4", "Eval 4", "Eval 4 (ema)"]
    for ln in lines:
        assert " | Loss: " in ln and " | Score: " in ln and " | Pen: " in ln and (" | Time: " in ln) == ln.startswith("Step")
        assert all(0.0 < float(x.split(" ")[1]) < 100.0 for x in ln.split(" | ")[1:4]), ln       # losses: positive, of order one
    assert sorted(os.listdir(run)) == ["checkpoint_2.pth", "checkpoint_4.pth", "ema_2.pth", "ema_4.pth", "ema_final.pth", "model_final.pth", "train_state.pth"]
    ck = torch.load(run / "ema_2.pth", weights_only=True)
    assert set(ck) == {"meta", "state_dict"} and len(ck["state_dict"]) == 323
    ema, raw = torch.load(run / "ema_final.pth", weights_only=True), torch.load(run / "model_final.pth", weights_only=True)
    init = spec.synthetic_state_dict(2, seed=0)
    assert list(ema) == list(raw) == list(init) and all(v.shape == raw[k].shape for k, v in ema.items())
    k = "enc1.conv1.weight"                                              # a Conv1d weight: stored permuted, named view permuted back
    assert float((ema[k] - torch.from_numpy(init[k])).abs().max()) > 0 and float((ema[k] - raw[k]).abs().max()) > 0    # moved, and not the raw weights
    assert dhg_amd.find_checkpoint(run).name == "model_final.pth"
    model = dhg_amd.load_model(cfg, run / "ema_final.pth")
    inp = spec.synthetic_inputs(2, 64, 8, seed=2)
    out = dhg_amd.sample(model, torch.from_numpy(inp["text"]).cuda(), torch.from_numpy(inp["style"]).cuda(), L=64, T=2, seed=3)
    assert out.shape == (2, 64, 3) and bool(torch.isfinite(out).all())
    state = torch.load(run / "train_state.pth", weights_only=True)
    assert state["count"] == 4 and state["step_count"] == 4 and state["ema_decay"] == 0.999 and state["host_rng"] is not None
    more = []
    tm.fit(cfg, tmp_path / "batches.pt", tmp_path / "run2", steps=6, log=more.append, resident=True, ema=0.999, resume=run / "train_state.pth",
           val_path=tmp_path / "val.pt")
    assert [ln.split(" | ")[0] for ln in more] == ["Step 6", "Eval 6", "Eval 6 (ema)"], more
    assert all(0.0 < float(x.split(" ")[1]) < 100.0 for ln in more for x in ln.split(" | ")[1:4]), more
    assert sorted(os.listdir(tmp_path / "run2")) == ["checkpoint_6.pth", "ema_6.pth", "ema_final.pth", "model_final.pth", "train_state.pth"]
    assert torch.load(tmp_path / "run2" / "train_state.pth", weights_only=True)["count"] == 6
