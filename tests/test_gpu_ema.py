"""dhw_train_adam_ema_dev on the GPU (include/dhw_train.h): the fused Adam + EMA pass against dhw_train_adam_dev bit for bit, against the
float64 statements of tests/ema_ref.py, and inside GraphedTrainStep.

Every buffer of a direct call sits inside 64 floats of canary on each side, at a 16-byte boundary (offset 0: the 16-byte form when all
five are there) or one float past it (the scalar form).  Sizes: 1, 3, 1029 (a tail of 1 after 257 vectors, two workgroups), 4099 one
float off, and GRID x 256 x 4 + 712 x 4 + 1 with GRID read from the launcher's source — 2 100 001 for its 2048 workgroups: every lane
takes one vector, 712 lanes a second one, and one element is left for the scalar tail."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd  # noqa: F401
from dhg_amd import spec, train, train_model as tm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("p", "g", "m", "v", "ema")


def _grid_cap():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "train.hip")).read()
    return int(re.search(r"constexpr unsigned ADAM_EMA_GRID = (\d+);", src).group(1))


N_TWO_PASSES = _grid_cap() * 256 * 4 + 712 * 4 + 1
ALL_OFF = {k: 1 for k in NAMES}
CASES = [(1, {}), (3, {}), (1029, {}), (4099, ALL_OFF), (4099, {"ema": 1}), (N_TWO_PASSES, {})]


class Buf:
    """One device buffer of n floats inside its canary margins, ``off`` floats past a 16-byte boundary."""

    def __init__(self, val, off, gen):
        self.n, self.lo = val.numel(), CANARY + off
        self.hi = self.lo + self.n
        self.host = torch.randn(self.hi + CANARY, generator=gen)
        self.host[self.lo:self.hi] = val
        self.whole = self.host.to(DEV)
        assert self.whole.data_ptr() % 16 == 0
        self.view = self.whole[self.lo:self.hi]
        assert (self.view.data_ptr() % 16 != 0) == bool(off)

    def read(self, what):
        back = self.whole.cpu()
        bits = lambda t: t.view(torch.int32)   # noqa: E731
        assert torch.equal(bits(back[:self.lo]), bits(self.host[:self.lo])), f"{what}: wrote in front of the buffer"
        assert torch.equal(bits(back[self.hi:]), bits(self.host[self.hi:])), f"{what}: wrote past the end of the buffer"
        out = back[self.lo:self.hi].clone()
        assert not bool(torch.isnan(out).any()), f"{what}: NaN"
        return out


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(n, seed=0, gscale=1e-2):
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda: torch.randn(n, generator=g)   # noqa: E731
    return {"p": r(), "g": r() * gscale, "m": r() * 1e-2, "v": (r() * 1e-2) ** 2, "ema": r()}


def _fused(inp, offs, max_norm, updates, ema_hypers, lr=3e-4):
    """``updates`` calls of the fused entry on canaried buffers -> per update the read-back {p, m, v, ema, sqnorm}; g checked unchanged."""
    gen = torch.Generator().manual_seed(77)
    bufs = {k: Buf(inp[k], offs.get(k, 0), gen) for k in NAMES}
    ad = train.Adam([bufs["p"].view], max_norm=max_norm, ema_decay=0.5)
    ad.m, ad.v, ad.ema = [bufs["m"].view], [bufs["v"].view], [bufs["ema"].view]
    hyper, eh, sq = torch.zeros(9, device=DEV), torch.zeros(2, device=DEV), torch.full((1,), float("nan"), device=DEV)
    out = []
    for t in range(updates):
        hyper.copy_(torch.tensor(ad.hyper(lr * (t + 1))))
        eh.copy_(torch.tensor(ema_hypers[t], dtype=torch.float32))
        ad.step_dev([bufs["g"].view], hyper, sq, eh)
        torch.cuda.synchronize()
        out.append({k: bufs[k].read((k, t)) for k in NAMES} | {"sqnorm": float(sq)})
        assert _bits_equal(out[-1]["g"], inp["g"]), "g changed"
    return out


def _plain(inp, max_norm, updates, lr=3e-4):
    """The same updates through dhw_train_adam_dev on plain buffers -> the final {p, m, v}."""
    p = inp["p"].to(DEV)
    ad = train.Adam([p], max_norm=max_norm)
    ad.m[0].copy_(inp["m"])
    ad.v[0].copy_(inp["v"])
    g = inp["g"].to(DEV)
    hyper, sq = torch.zeros(9, device=DEV), torch.zeros(1, device=DEV)
    for t in range(updates):
        hyper.copy_(torch.tensor(ad.hyper(lr * (t + 1))))
        ad.step_dev([g], hyper, sq)
    torch.cuda.synchronize()
    return {"p": p.cpu(), "m": ad.m[0].cpu(), "v": ad.v[0].cpu()}


DECAYS = (0.9999, 0.5, 2 / 11)


def _hyper_of(d):
    return [float(np.float32(d)), float(np.float32(1.0 - d))]


@pytest.mark.parametrize("max_norm", [0.0, 100.0])
@pytest.mark.parametrize("n,offs", CASES)
def test_unclipped_bits_of_adam_dev_the_norm_and_the_ema_bound(n, offs, max_norm):
    """Three updates, unclipped (no clipping at all, or a gradient far under the clip so that the factor is exactly 1): p, m, v carry the
    bits dhw_train_adam_dev gives; sqnorm is the float64 norm within the suite's 1e-4; and at each update, with the decays 0.9999, 0.5
    and 2/11 in turn, |ema' - ref64| <= 2^-22 max(|ema|, |p'|) per element, ref64 = decay ema + omd p' in float64 from the GPU's own p'
    and the fp32 scalars.  The bound is derived: omd p' and the FMA round once each (with decay ema exact inside the FMA), an unfused
    evaluation once more — two or three roundings, each at most 2^-24 of a term no larger than max(|ema|, |p'|) since decay + omd <= 1
    + 2^-24."""
    inp = _inputs(n, seed=n % 97)
    assert float(inp["g"].double().norm()) < 50.0
    hypers = [_hyper_of(d) for d in DECAYS]
    got = _fused(inp, offs, max_norm, 3, hypers)
    want = _plain(inp, max_norm, 3)
    for k in ("p", "m", "v"):
        assert _bits_equal(got[-1][k], want[k]), (k, float((got[-1][k] - want[k]).abs().max()))
    sq64 = float((inp["g"].double() ** 2).sum())
    ema_old = inp["ema"]
    for t, step in enumerate(got):
        assert abs(step["sqnorm"] - sq64) <= 1e-4 * sq64, (t, step["sqnorm"], sq64)
        ref = ema_ref.ema_line(ema_old.numpy(), step["p"].numpy(), hypers[t])
        bound = 2.0 ** -22 * np.maximum(np.abs(ema_old.numpy().astype(np.float64)), np.abs(step["p"].numpy().astype(np.float64)))
        err = np.abs(step["ema"].numpy().astype(np.float64) - ref)
        assert bool((err <= bound).all()), (t, DECAYS[t], float((err / np.maximum(bound, 1e-300)).max()))
        ema_old = step["ema"]


@pytest.mark.parametrize("n,offs", [(1029, {}), (4099, ALL_OFF), (N_TWO_PASSES, {})])
def test_ema_hyper_0_1_copies_the_new_weights_and_1_0_keeps_the_average(n, offs):
    inp = _inputs(n, seed=5)
    copied, kept = _fused(inp, offs, 0.0, 1, [[0.0, 1.0]])[0], _fused(inp, offs, 0.0, 1, [[1.0, 0.0]])[0]
    assert _bits_equal(copied["ema"], copied["p"]) and not _bits_equal(copied["p"], inp["p"])
    assert _bits_equal(kept["ema"], inp["ema"]) and _bits_equal(kept["p"], copied["p"])


def test_clipped_updates_track_the_float64_statement():
    """Ten updates on two buffers (5000 + 333 elements: one norm over both) with gradients 1e3 x too large for the clip at 100, Noam
    learning rates and the warm-up decays, against tests/ema_ref.py carried in float64: the criterion of test_clipped_adam_tracks_torch."""
    g = torch.Generator().manual_seed(3)
    p0 = [torch.randn(5000, generator=g), torch.randn(333, generator=g)]
    mine = [p.clone().to(DEV) for p in p0]
    ad = train.Adam(mine, ema_decay=0.9999)
    ref = {k: [p.numpy().astype(np.float64) for p in p0] for k in ("p", "ema")}
    ref["m"], ref["v"] = [np.zeros(5000), np.zeros(333)], [np.zeros(5000), np.zeros(333)]
    hyper, eh, sq = torch.zeros(9, device=DEV), torch.zeros(2, device=DEV), torch.zeros(1, device=DEV)
    for step in range(1, 11):
        grads = [torch.randn(p.shape, generator=g) * 1e3 for p in p0]
        h = ad.hyper(train.noam_lr(step, 256, 4))
        e = ad.ema_hyper()
        assert e == _hyper_of(ema_ref.ema_decay_at(step, 0.9999))
        hyper.copy_(torch.tensor(h))
        eh.copy_(torch.tensor(e))
        ad.step_dev([gr.to(DEV) for gr in grads], hyper, sq, eh)
        cat = lambda xs: np.concatenate([np.asarray(x, np.float64) for x in xs])   # noqa: E731
        p2, m2, v2, sq64 = ema_ref.adam_step(cat(ref["p"]), cat([gr.numpy() for gr in grads]), cat(ref["m"]), cat(ref["v"]), h)
        e2 = ema_ref.ema_line(cat(ref["ema"]), p2, e)
        for k, arr in (("p", p2), ("m", m2), ("v", v2), ("ema", e2)):
            ref[k] = [arr[:5000], arr[5000:]]
        assert sq64 > 100.0 ** 2 and abs(float(sq) - sq64) <= 1e-4 * sq64
    for i in range(2):
        assert np.allclose(mine[i].cpu().numpy(), ref["p"][i], rtol=2e-5, atol=2e-6), i
        assert np.allclose(ad.ema[i].cpu().numpy(), ref["ema"][i], rtol=2e-5, atol=2e-6), i
        assert float(np.abs(ref["ema"][i] - p0[i].numpy()).max()) > 1e-4            # the average has moved


# ---------------------------------------------------------------- in the step
B, L, LT = 2, 64, 10
_RUNS = {}


def _run(ema, graph):
    """Three updates of GraphedTrainStep on one fixed batch -> losses [3, 3], the parameter states after each update, the EMA (or None),
    the initial parameters; each variant is run once and shared by the tests below."""
    key = (ema, graph)
    if key not in _RUNS:
        sd = spec.synthetic_state_dict(2, 128, 192, 256, seed=0)
        model = tm.TrainModel(sd, num_layers=2, device=torch.device(DEV))
        opt = train.Adam(model.parameters(), ema_decay=ema)
        inp = spec.synthetic_inputs(B, L, LT, S=14, seed=21, pad=2)
        g = torch.Generator().manual_seed(21)
        batch = {"strokes": torch.cat([torch.from_numpy(inp["strokes"]), (torch.rand(B, L, 1, generator=g) < 0.1).float()], dim=-1),
                 "text": torch.from_numpy(inp["text"]), "style": torch.from_numpy(inp["style"])}
        alphas = torch.rand(B, 1, generator=g) * 0.9 + 0.05
        step = tm.GraphedTrainStep(model, opt, B, L, LT, 14, warmup=100, seed=4)
        assert ("ema" in step._dv) == (ema is not None)
        p0 = model.flat.cpu().numpy().astype(np.float64)
        losses, states = [], []
        for k in (1, 2, 3):
            losses.append(step(batch, None, k, alphas=alphas, graph=graph).cpu().numpy())
            states.append(model.flat.cpu().numpy().astype(np.float64))
        assert (step.graph is not None) == graph
        _RUNS[key] = dict(losses=np.array(losses), states=states, ema=None if ema is None else opt.ema[0].cpu().numpy().astype(np.float64), p0=p0)
    return _RUNS[key]


def _l2_close(a, b, p0, what):
    """The criterion of tests/test_gpu_train.py (bucketed RCCL vs plain update): difference < 1e-3 x displacement, in L2."""
    diff, moved = np.linalg.norm(a - b), np.linalg.norm(b - p0)
    print(f"{what}: difference (L2) {diff:.3e}, displacement (L2) {moved:.3e}")
    assert moved > 1e-3 and diff < 1e-3 * moved, (what, diff, moved)


def test_graphed_and_eager_steps_with_ema_agree():
    a, b = _run(0.999, True), _run(0.999, False)
    assert np.isfinite(a["losses"]).all() and np.allclose(a["losses"], b["losses"], rtol=2e-6, atol=0)
    _l2_close(a["states"][-1], b["states"][-1], b["p0"], "parameters, graph vs eager")
    _l2_close(a["ema"], b["ema"], b["p0"], "ema, graph vs eager")


@pytest.mark.parametrize("graph", [True, False])
def test_ema_in_the_step_is_the_recurrence_over_the_parameter_states(graph):
    r = _run(0.999, graph)
    ema = r["p0"].copy()
    for t, p in enumerate(r["states"], start=1):
        ema = ema_ref.ema_line(ema, p, _hyper_of(ema_ref.ema_decay_at(t, 0.999)))
    _l2_close(r["ema"], ema, r["p0"], f"ema vs its float64 recurrence (graph={graph})")


def test_ema_on_leaves_the_parameters_of_an_ema_off_run():
    a, b = _run(0.999, True), _run(None, True)
    assert b["ema"] is None and np.allclose(a["losses"], b["losses"], rtol=2e-6, atol=0)
    _l2_close(a["states"][-1], b["states"][-1], b["p0"], "parameters, EMA on vs off")
