"""The eager entries around the denoiser share one handle: its workspace ws[0], its device lengths, and (dhw_score and the
ddim entries) one scratch set.  What one entry leaves behind must not reach the next: runs on the MI355X only (-m gpu).

The reference is the library's own documented guarantee (include/dhw.h): every entry is bit-deterministic and a row depends
on its own sample alone, so a call's result is what the same call gives on a fresh handle, whose buffers nothing has
written.  No tolerance: every comparison is torch.equal.

Shapes: 2 layers, max_B = 4, max_L = 32, max_Lt = 8; B = 2, L = 24, Lt = 3 with one padded token, T = 5; lengths uniform and
[8, 24] (one row and three rows at the L/8 level).  Each call under test directly follows a uniform call of the OTHER family
at B = 3, L = 32: score's filler is an inversion with two iterations (x, w, eps and pen of the scratch all written), the
ddim entries' filler is a score call; attention and forward, which use the workspace and the lengths only, follow either.
The filler leaves finite non-zero rows beyond the call's B * L rows and beyond its lengths."""
import pytest
import torch

import dhg_amd
from dhg_amd import spec

pytestmark = pytest.mark.gpu

B, L, Lt, T = 2, 24, 3, 5
FB, FL = 3, 32                        # the filler calls: more samples and longer rows than the calls under test
LENGTHS = {"uniform": None, "ragged": [8, 24]}
_CACHE = {}


def fresh_model(prec):
    m = dhg_amd.DiffusionModel(2, precision=prec, max_B=4, max_L=32, max_Lt=8).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}, strict=True)
    return m


def _inputs():
    if not _CACHE:
        inp = spec.synthetic_inputs(FB, FL, Lt, seed=71, pad=1, T=1)
        g = torch.Generator().manual_seed(72)
        strokes = torch.randn((FB, FL, 3), generator=g)
        strokes[..., 2] = (strokes[..., 2] > 0.5).float()
        text = torch.from_numpy(inp["text"])
        assert (text == 0).sum() == FB
        _CACHE.update(text=text.cuda(), style=torch.from_numpy(inp["style"]).cuda(), strokes=strokes.cuda(),
                      sigma=torch.tensor([0.9, 0.3, 0.6]).cuda())
    return _CACHE


def _cut(b, l):
    i = _inputs()
    return i["strokes"][:b, :l].contiguous(), i["text"][:b], i["style"][:b], i["sigma"][:b]


def _score(m, lens):
    s, t, sv, _ = _cut(B, L)
    return (dhg_amd.score(m, s, t, sv, lengths=lens, levels=[1, 3], T=T, seed=5),)


def _sample_ddim(m, lens):
    _, t, sv, _ = _cut(B, L)
    return dhg_amd.sample_ddim(m, t, sv, L=L, T=T, steps=2, seed=5, lengths=lens, return_latent=True)


def _invert(m, lens):
    s, t, sv, _ = _cut(B, L)
    return (dhg_amd.invert(m, s, t, sv, lengths=lens, T=T, steps=2, iters=2),)


def _attention(m, lens):
    s, t, sv, sg = _cut(B, L)
    return dhg_amd.attention(m, s[..., :2].contiguous(), t, sg, sv, lengths=lens, layer=-1)


def _forward(m, lens):
    s, t, sv, sg = _cut(B, L)
    return m(s[..., :2].contiguous(), t, sg, sv, lengths=lens if lens is not None else [L] * B)[:2]


def _fill_from_score(m):
    s, t, sv, _ = _cut(FB, FL)
    return dhg_amd.score(m, s, t, sv, levels=[2], T=T, seed=9)


def _fill_from_ddim(m):
    s, t, sv, _ = _cut(FB, FL)
    return dhg_amd.invert(m, s, t, sv, T=T, steps=1, iters=2)


# name -> (the call, the filler of the other family that runs right before it)
CALLS = {
    "score": (_score, _fill_from_ddim),
    "sample_ddim": (_sample_ddim, _fill_from_score),
    "invert": (_invert, _fill_from_score),
    "attention": (_attention, _fill_from_ddim),
    "forward": (_forward, _fill_from_score),
}


def _check_tails(name, outs, lens):
    """Rows at or past lengths[b] are exactly 0 (token: -1) where include/dhw.h says so."""
    for b, n in enumerate(lens):
        if name in ("sample_ddim", "invert", "forward"):
            for o in outs:
                assert o.shape[1] == L and not o[b, n:].any(), (name, b)
        if name == "attention":
            mean, token = outs
            assert not mean[b, n // 8:].any() and (token[b, n // 8:] == -1).all() and (token[b, :n // 8] >= 0).all(), (name, b)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_an_entry_never_sees_what_another_left_in_the_shared_buffers(prec):
    want = {}
    for name, (call, _) in CALLS.items():
        for kind, lens in LENGTHS.items():
            want[name, kind] = [o.cpu() for o in call(fresh_model(prec), lens)]   # the first call of a fresh handle
    m = fresh_model(prec)
    for kind, lens in LENGTHS.items():
        for name, (call, fill) in CALLS.items():
            assert torch.isfinite(fill(m)).all()
            got = [o.cpu() for o in call(m, lens)]
            assert len(got) == len(want[name, kind])
            for g, w in zip(got, want[name, kind]):
                assert torch.isfinite(g).all() and torch.equal(g, w), (name, kind)
            if lens is not None:
                _check_tails(name, got, lens)
    # nothing above is trivially equal: the two length sets give different results, and a score is not 0
    assert not torch.equal(want["sample_ddim", "uniform"][0], want["sample_ddim", "ragged"][0])
    assert want["score", "ragged"][0].abs().min() > 0
