"""Training from a dataset resident on the GPU, on the GPU: the draw kernel against its numpy statement (tests/batch_ref.py) bit
for bit, the gather kernel against torch indexing bit for bit, a resident step against a host-fed step given the same rows, the
draws under graph replay, and fit(resident=True)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec, train, train_model as tm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _writers():
    w = np.array([5] * 1 + [9] * 2 + [2] * 3 + [7] * 31, np.int64)
    return w[np.random.default_rng(0).permutation(len(w))]


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize("N,B,grouped", [(37, 5, True), (37, 5, False), (1, 3, False)])
def test_draw_equals_the_numpy_statement_bit_for_bit(N, B, grouped):
    T, seed = 60, 0x1234567_89ABCDEF
    abar = dhg_amd.get_alpha_set(T).numpy().astype(np.float32)
    host_tables = tm.group_tables(_writers()) if grouped else None
    tables = [t.to(DEV) for t in host_tables] if grouped else [None] * 4
    abar_d = torch.from_numpy(abar).to(DEV)
    rng = torch.zeros(2, dtype=torch.int64, device=DEV)
    idx, src = torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
    alphas, sigma = torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)

    def draw(index):
        rng.copy_(torch.tensor([seed, index], dtype=torch.int64))
        rc = _lib.lib().dhw_train_batch_draw(rng.data_ptr(), N, B, abar_d.data_ptr(), T, *(_ptr(t) for t in tables), idx.data_ptr(), src.data_ptr(),
                                             alphas.data_ptr(), sigma.data_ptr(), _st())
        assert rc == 0, _lib.lib().dhw_train_last_error()
        return idx.cpu().numpy().copy(), src.cpu().numpy().copy(), alphas.cpu().numpy().copy(), sigma.cpu().numpy().copy()

    got = {}
    for index in (0, 1, 7, 2 ** 33):
        got[index] = g = draw(index)
        want = batch_ref.draw(seed, index, N, B, abar, tuple(t.numpy() for t in host_tables) if grouped else None)
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), (index, g[:2], want[:2])
        assert np.array_equal(g[2].view(np.uint32), want[2].view(np.uint32)), (index, g[2], want[2])
        assert np.array_equal(g[3].view(np.uint32), want[3].view(np.uint32)), (index, g[3], want[3])
    again = draw(1)
    assert all(np.array_equal(a, b) for a, b in zip(again, got[1]))                 # the same index reproduces
    assert not np.array_equal(got[0][2], got[1][2]) and not np.array_equal(got[7][2], got[2 ** 33][2])   # another index differs
    if N > 1:
        assert not np.array_equal(got[0][0], got[1][0])


# ---------------------------------------------------------------- 2. the gather
def _dataset(N, L, Lt, S, seed=3, zero_rows=(1,)):
    g = torch.Generator().manual_seed(seed)
    strokes = torch.cat([torch.randn(N, L, 2, generator=g), (torch.rand(N, L, 1, generator=g) < 0.2).float()], dim=-1)
    text = torch.randint(1, spec.VOCAB, (N, Lt), generator=g)
    text[:, Lt - 2:] = 0                       # padding at the end of every row
    for r in zero_rows:
        text[r] = 0                            # and whole rows of padding
    return {"strokes": strokes, "text": text, "style": torch.randn(N, S, 1280, generator=g).abs()}


def _gather(d, idx, src, N, B, L, Lt, S):
    """-> the five outputs (trimmed to their shapes) and the guard tails behind them."""
    dd = {k: v.to(DEV) for k, v in d.items()}
    GUARD = 64
    outs = {"x": (B * L * 2, torch.float32, -7.0), "pen": (B * L, torch.float32, -7.0), "ids": (B * Lt, torch.int64, -7), "mask": (B * Lt, torch.float32, -7.0),
            "style": (B * S * 1280, torch.float32, -7.0)}
    buf = {k: torch.full((n + GUARD,), fill, dtype=dt, device=DEV) for k, (n, dt, fill) in outs.items()}
    i_d, s_d = torch.tensor(idx, dtype=torch.int32, device=DEV), torch.tensor(src, dtype=torch.int32, device=DEV)
    rc = _lib.lib().dhw_train_batch_gather(dd["strokes"].data_ptr(), dd["text"].data_ptr(), dd["style"].data_ptr(), i_d.data_ptr(), s_d.data_ptr(), N, B, L, Lt, S,
                                           buf["x"].data_ptr(), buf["pen"].data_ptr(), buf["ids"].data_ptr(), buf["mask"].data_ptr(), buf["style"].data_ptr(), _st())
    assert rc == 0, _lib.lib().dhw_train_last_error()
    torch.cuda.synchronize()
    for k, (n, dt, fill) in outs.items():
        assert bool((buf[k][n:] == fill).all()), f"{k}: written past its end"     # from the first byte past the output on
    return {k: buf[k][:n].cpu() for k, (n, _, _) in outs.items()}


@pytest.mark.parametrize("S", [14, 1])
def test_gather_equals_torch_indexing_bit_for_bit(S):
    N, L, Lt, B = 7, 24, 5, 3
    d = _dataset(N, L, Lt, S, zero_rows=(2,))
    idx, src = [2, 5, 2], [4, 6, 0]            # a repeated index (an all-padding text row), style_src != idx
    got = _gather(d, idx, src, N, B, L, Lt, S)
    i, s = torch.tensor(idx), torch.tensor(src)
    assert torch.equal(got["x"].view(B, L, 2), d["strokes"][i][:, :, :2].contiguous())
    assert torch.equal(got["pen"].view(B, L), d["strokes"][i][:, :, 2].contiguous())
    assert torch.equal(got["ids"].view(B, Lt), d["text"][i])
    assert torch.equal(got["mask"].view(B, Lt), (d["text"][i] == 0).float()) and bool(got["mask"].view(B, Lt)[0].all())
    assert torch.equal(got["style"].view(B, S, 1280), d["style"][s])


def test_gather_writes_zeros_and_a_full_mask_for_an_index_outside_the_dataset():
    N, L, Lt, S, B = 7, 24, 5, 2, 4
    d = _dataset(N, L, Lt, S)
    got = _gather(d, [3, -1, 7, 4], [3, 2, 1, 2 ** 31 - 1], N, B, L, Lt, S)     # samples 1, 2 (idx) and 3 (style_src) are out of range
    for k, per in (("x", L * 2), ("pen", L), ("ids", Lt), ("style", S * 1280)):
        v = got[k].view(B, per)
        assert bool((v[1:] == 0).all()) and bool(v[0].abs().sum() > 0), k
    m = got["mask"].view(B, Lt)
    assert bool((m[1:] == 1).all()) and torch.equal(m[0], (d["text"][3] == 0).float())


# ---------------------------------------------------------------- 3. / 4. the step
SHAPE = dict(B=2, L=64, Lt=10, N=9, S=14)


def _resident_setup():
    d = _dataset(SHAPE["N"], SHAPE["L"], SHAPE["Lt"], SHAPE["S"], seed=5, zero_rows=())
    d["writer"] = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2])
    return d, spec.synthetic_state_dict(2, 128, 192, 256, seed=0), dhg_amd.get_alpha_set(60).float()


def _step(sd, data=None, alpha_set=None, **kw):
    model = tm.TrainModel(sd, num_layers=2, device=DEV, drop_rate=0.1)
    return tm.GraphedTrainStep(model, train.Adam(model.parameters()), SHAPE["B"], SHAPE["L"], SHAPE["Lt"], seed=7, data=data, alpha_set=alpha_set, **kw)


BUFFERS = ("x", "pen", "alphas", "sigma", "ids", "mask", "style")


@pytest.mark.parametrize("graph", [True, False])
def test_resident_step_equals_the_host_fed_step_on_the_rows_it_drew(graph):
    d, sd, abar = _resident_setup()
    rd = tm.ResidentData(d, DEV)
    assert rd.tables is not None and (rd.N, rd.L, rd.Lt, rd.S) == (9, 64, 10, 14)
    k = 3
    res = _step(sd, rd, abar)
    loss_r = res(step=k, graph=graph).cpu()
    idx, src, alphas = (t.cpu() for t in res.last_draw())
    w = d["writer"]
    assert bool(((0 <= idx) & (idx < 9)).all()) and torch.equal(w[src.long()], w[idx.long()]) and bool((src != idx).all())
    want = batch_ref.draw(7, k, 9, 2, abar.numpy(), tuple(t.numpy() for t in tm.group_tables(w)))
    assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(src.numpy(), want[1]) and np.array_equal(alphas.numpy(), want[2])
    fed = _step(sd)
    batch = {"strokes": d["strokes"][idx.long()], "text": d["text"][idx.long()], "style": d["style"][src.long()]}
    loss_h = fed(batch, None, k, alphas=alphas.reshape(-1, 1), graph=graph).cpu()
    for name in BUFFERS:
        a, b = getattr(res, name).cpu(), getattr(fed, name).cpu()
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), name
    print("losses resident / host-fed:", loss_r.tolist(), loss_h.tolist())
    # (the loss sums are fp32 atomics over blocks: the same inputs give the same loss up to summation order — the 2e-6 of
    # test_device_drawn_encoder_dropout_trains)
    assert bool(torch.isfinite(loss_r).all()) and bool(((loss_r - loss_h).abs() <= 2e-6 * loss_h.abs()).all()), (loss_r, loss_h)
    with pytest.raises(ValueError, match="without batch"):
        res(batch, step=k + 1)
    with pytest.raises(ValueError, match="without alphas"):
        res(step=k + 1, alphas=alphas)
    assert res.data is rd


def test_replays_draw_by_the_update_number():
    d, sd, abar = _resident_setup()
    model = tm.TrainModel(sd, num_layers=2, device=DEV, drop_rate=0.1)
    step = tm.GraphedTrainStep(model, train.Adam(model.parameters()), 2, 64, 10, warmup=10 ** 9, seed=7, data=tm.ResidentData(d, DEV), alpha_set=abar)
    draws, losses = [], []
    for n in (1, 2, 1):
        losses.append(float(step(step=n)[0]))
        draws.append([t.cpu().clone() for t in step.last_draw()])
    assert step.graph is not None
    assert all(torch.equal(a, b) for a, b in zip(draws[0], draws[2]))
    assert not torch.equal(draws[0][2], draws[1][2]) and not (torch.equal(draws[0][0], draws[1][0]) and torch.equal(draws[0][1], draws[1][1]))
    assert abs(losses[0] - losses[2]) < 1e-4 * abs(losses[0]) and abs(losses[0] - losses[1]) > 1e-4 * abs(losses[0]), losses   # (lr ~ 0: the weights stay put)


# ---------------------------------------------------------------- 5. fit(resident=True)
def test_fit_resident_trains_from_a_file_with_writers(tmp_path):
    cfg = tmp_path / "cfg.yml"
    cfg.write_text("""
experiment: {seed: 1}
dataset_args: {max_seq_len: 64, max_text_len: 8}
training_args: {steps: 4, batch_size: 2, warmup_steps: 100, clip_grad: 100.0, dropout: 0.1, att_layers_num: 2, channels: 128, log_freq: 2, save_freq: 3}
optimizer: {type: torch.optim.Adam, params: {lr: 0.0003, weight_decay: 0.00001, betas: [0.9, 0.98]}}
""")
    d = _dataset(12, 64, 8, 14, seed=8, zero_rows=())
    d["writer"] = torch.arange(12) // 3
    d["kept"] = list(range(12))
    torch.save(d, tmp_path / "batches.pt")
    with pytest.raises(ValueError, match="needs data_path"):
        tm.fit(cfg, None, tmp_path / "none", resident=True)
    lines = []
    tm.fit(cfg, tmp_path / "batches.pt", tmp_path / "run", log=lines.append, resident=True)
    assert len(lines) == 2 and lines[0].startswith("Step 2 | Loss: ") and " | Score: " in lines[1] and " | Pen: " in lines[1] and " | Time: " in lines[1]
    ck = torch.load(tmp_path / "run" / "checkpoint_3.pth", weights_only=True)
    assert set(ck) == {"meta", "state_dict"} and len(ck["state_dict"]) == 323
    sd = torch.load(tmp_path / "run" / "model_final.pth", weights_only=True)
    ref = spec.synthetic_state_dict(2, seed=0)
    assert list(sd) == list(ref) and all(bool(torch.isfinite(v).all()) for v in sd.values())
    assert max(float((sd[k] - torch.from_numpy(ref[k])).abs().max()) for k in ref) > 0
    assert dhg_amd.load_model(cfg, tmp_path / "run" / "model_final.pth") is not None
