"""train_model.EvalStep on the GPU: the held-out loss of its forward-only passes against the separately pinned training step fed the same
rows, noise levels and noise; its repeatability; and that it leaves the model and a training graph captured before it as they were."""
import ctypes as C

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec, train, train_model as tm

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, L, LT, S = 2, 64, 10, 14
N_VAL, LEVELS, SEED = 5, (7, 52), 3            # two whole batches; row 4 is left out


def _dataset(n, seed):
    g = torch.Generator().manual_seed(seed)
    strokes = torch.cat([torch.randn(n, L, 2, generator=g), (torch.rand(n, L, 1, generator=g) < 0.2).float()], dim=-1)
    text = torch.randint(1, spec.VOCAB, (n, LT), generator=g)
    text[:, LT - 2:] = 0
    return {"strokes": strokes, "text": text, "style": torch.randn(n, S, 1280, generator=g).abs()}


def _drawn_eps(index):
    """eps of dhw_train_draw for rng = (SEED, index), on the host."""
    rng = torch.tensor([SEED, index], dtype=torch.int64, device=DEV)
    eps, keep = torch.zeros(B, L, 2, device=DEV), torch.zeros(B, S, 1280, device=DEV)
    rc = _lib.lib().dhw_train_draw(rng.data_ptr(), B, L, eps.data_ptr(), keep.numel(), keep.numel() // B, 0.0, keep.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().dhw_train_last_error()
    return eps.cpu()


def test_eval_step_equals_the_training_step_path_and_disturbs_nothing():
    sd, abar = spec.synthetic_state_dict(2, 128, 192, 256, seed=0), dhg_amd.get_alpha_set(60).float()
    val = _dataset(N_VAL, seed=11)
    K = len(LEVELS)

    # a training run as it would be: encoder dropout on, a resident feed; lr ~ 0 (warmup 1e9), so the weights stay the initial ones
    model = tm.TrainModel(sd, num_layers=2, device=DEV, drop_rate=0.1)
    train_step = tm.GraphedTrainStep(model, train.Adam(model.parameters()), B, L, LT, warmup=10 ** 9, seed=7,
                                     data=tm.ResidentData(_dataset(9, seed=5), DEV), alpha_set=abar)
    before = [train_step(step=n).cpu().numpy() for n in (1, 2)]                   # captured here, before any EvalStep exists
    assert train_step.graph is not None
    flat0 = model.flat.clone()

    ev = tm.EvalStep(model, tm.ResidentData(val, DEV), B, levels=LEVELS, seed=SEED)
    assert ev.batches == 2 and ev.levels == [7, 52]
    got = ev().cpu().numpy()
    again = ev().cpu().numpy()
    assert got.shape == (K, 3) and np.isfinite(got).all()
    assert np.allclose(again, got, rtol=2e-6, atol=0), (got, again)
    assert np.allclose(got[:, 0], got[:, 1] + got[:, 2], rtol=1e-6) and abs(got[0, 0] - got[1, 0]) > 1e-4 * abs(got[0, 0])   # the levels differ
    assert (model.drop_rate, model.style_drop) == (0.1, tm.TrainModel.STYLE_DROP) and torch.equal(model.flat, flat0)
    after = train_step(step=2).cpu().numpy()
    assert np.allclose(after, before[1], rtol=2e-6, atol=0) and not np.allclose(after, before[0], rtol=1e-4), (before, after)

    # the yardstick: the host-fed training step in eval mode on the same rows, noise levels and noise
    plain = tm.TrainModel(sd, num_layers=2, device=DEV, drop_rate=0.0)
    plain.style_drop = 0.0
    fed = tm.GraphedTrainStep(plain, train.Adam(plain.parameters()), B, L, LT, device_rng=False, warmup=10 ** 9)
    ones = torch.ones(B, S, 1280)
    want = np.zeros((K, 3))
    n = 0
    for i in range(N_VAL // B):
        rows = slice(i * B, i * B + B)
        batch = {k: val[k][rows] for k in ("strokes", "text", "style")}
        for k, level in enumerate(LEVELS):
            n += 1
            loss = fed(batch, None, n, alphas=torch.full((B, 1), float(abar[level])), eps=_drawn_eps(i * K + k), style_keep=ones)
            want[k] += loss.cpu().numpy().astype(np.float64) / (N_VAL // B)
    print("EvalStep:", got.tolist(), "training-step path:", want.tolist())
    assert np.allclose(got, want, rtol=2e-6, atol=0), (got, want)


def test_eval_step_refuses_what_it_cannot_evaluate():
    sd = spec.synthetic_state_dict(2, 128, 192, 256, seed=0)
    model = tm.TrainModel(sd, num_layers=2, device=DEV)
    rd = tm.ResidentData(_dataset(3, seed=1), DEV)
    with pytest.raises(ValueError, match="fewer than one batch"):
        tm.EvalStep(model, rd, 4)
    with pytest.raises(ValueError, match=r"levels\[0\] = 60"):
        tm.EvalStep(model, rd, 2, levels=[60])
