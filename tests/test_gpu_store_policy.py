"""Store policy of the stroke kernels' tile copy-outs (DHW_STORE_POLICY): runs on the MI355X only (-m gpu).

The policy decides HOW the large outputs leave a workgroup — plain stores, write-through stores, or plain stores followed by
one early agent-scope release — never WHAT is stored, so every comparison is torch.equal, no tolerance, and the reference
always comes from a FRESH handle created with DHW_STORE_POLICY=0 (every class plain), never from the handle under test.

DHW_STORE_POLICY holds two bits per output class, read once at dhw_create: bits 0-1 class C (ConvBlock out / pool), bits 2-3
class A (enc_a's x2 and qk2), bits 4-5 class B (enc_bc's out / pool and the chained att_dense output); 0 = plain, 1 = WT,
2 = EARLY.  A handle created without the variable runs the kernels that have the default word compiled in (every class WT);
every other word runs the builds that read it from the parameter blocks — so the all-plain reference and the default handle
are different kernel builds as well.

Shape: bf16 (and fp32 for the denoiser call), 2 layers, synthetic weights and inputs, B = 9, L = 136, Lt = 7, T = 3 — the
smallest that is partial at every level (136 / 68 / 34 / 17 rows: the last tile holds 8 of 128, 4 of 64, 2 of 32, 1 of 16 rows,
the pooled copy-outs an odd tail) and puts two samples on one XCD."""
import os

import pytest
import torch

import dhg_amd
from dhg_amd import spec

pytestmark = pytest.mark.gpu

B, L, LT, T = 9, 136, 7, 3
RAGGED = (136, 72, 8, 136, 40, 136, 136, 16, 104)
PLAIN, WT, EARLY = 0, 1, 2
SHIFT = {"C": 0, "A": 2, "B": 4}
ALL_WT = sum(WT << s for s in SHIFT.values())
ALL_EARLY = sum(EARLY << s for s in SHIFT.values())
SINGLE = [(c, p) for c in "CAB" for p in (PLAIN, WT, EARLY)]   # the nine single-class settings
_INP, _REFS = {}, {}


def _inputs():
    if not _INP:
        inp = spec.synthetic_inputs(B, L, LT, seed=41, pad=1, T=T)
        _INP.update({k: torch.from_numpy(v).cuda() for k, v in inp.items()})
    return _INP


def _model(policy, prec="bf16", extra=None):
    """A model whose handle exists (the switches are read at dhw_create, which the first device call runs)."""
    m = dhg_amd.DiffusionModel(2, precision=prec, max_B=B, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in spec.synthetic_state_dict(2).items()}, strict=True)
    env = {"DHW_STORE_POLICY": None if policy is None else str(policy), **(extra or {})}   # (None: the variable is unset)
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        m._ensure_handle(torch.device("cuda", torch.cuda.current_device()), B, L, LT, 14)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return m


def _samples(m):
    """(device noise, external noise, ragged with device noise, ragged with external noise)"""
    i = _inputs()
    return (dhg_amd.sample(m, i["text"], i["style"], L=L, T=T, seed=7).cpu(),
            dhg_amd.sample(m, i["text"], i["style"], L=L, T=T, noise=i["noise"]).cpu(),
            dhg_amd.sample(m, i["text"], i["style"], L=L, T=T, seed=7, lengths=RAGGED).cpu(),
            dhg_amd.sample(m, i["text"], i["style"], L=L, T=T, noise=i["noise"], lengths=RAGGED).cpu())


def _forward(m):
    i = _inputs()
    sigma = torch.linspace(0.15, 0.95, B).reshape(B, 1).cuda()
    eps, pen, _ = m(i["strokes"], i["text"], sigma, i["style"])
    return eps.cpu(), pen.cpu()


def _ref(what, prec="bf16"):
    """Outputs of a fresh all-plain handle; computed once, shared, never changed."""
    key = (what, prec)
    if key not in _REFS:
        m = _model(0, prec)
        _REFS[key] = _samples(m) if what == "samples" else _forward(m)
        assert all(torch.isfinite(t).all() for t in _REFS[key])
    return _REFS[key]


@pytest.mark.parametrize("cls,pol", SINGLE, ids=[f"{c}-{('plain', 'wt', 'early')[p]}" for c, p in SINGLE])
def test_single_class_policy_gives_the_same_samples(cls, pol):
    ref = _ref("samples")
    got = _samples(_model(pol << SHIFT[cls]))
    for name, r, g in zip(("device noise", "external noise", "ragged, device noise", "ragged, external noise"), ref, got):
        assert torch.equal(r, g), name
    # (ragged rows past each length stay zero under every policy)
    for b, n in enumerate(RAGGED):
        assert not got[2][b, n:].any() and not got[3][b, n:].any()


def test_all_classes_write_through_gives_the_same_samples():
    ref = _ref("samples")
    got = _samples(_model(ALL_WT))
    for name, r, g in zip(("device noise", "external noise", "ragged, device noise", "ragged, external noise"), ref, got):
        assert torch.equal(r, g), name


def test_default_handle_gives_the_same_samples():
    """No DHW_STORE_POLICY: the kernels with the default word compiled in."""
    ref = _ref("samples")
    got = _samples(_model(None))
    for name, r, g in zip(("device noise", "external noise", "ragged, device noise", "ragged, external noise"), ref, got):
        assert torch.equal(r, g), name


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_denoiser_call_is_the_same_under_every_policy(prec):
    eps, pen = _ref("forward", prec)
    for policy in (ALL_WT, ALL_EARLY, None):
        e, p = _forward(_model(policy, prec))
        assert torch.equal(eps, e) and torch.equal(pen, p), policy


def test_persistent_step_with_write_through_gives_the_same_samples():
    """The persistent step runs the same block bodies: write-through only makes its hand-off data visible earlier."""
    i = _inputs()
    ref = _ref("samples")
    m = _model(ALL_WT, extra={"DHW_PERSIST": "1"})
    out = dhg_amd.sample(m, i["text"], i["style"], L=L, T=T, noise=i["noise"]).cpu()
    assert m.persistent_plans() == 1
    assert torch.equal(ref[1], out), "persistent launch"
    d = _model(ALL_WT)
    dhg_amd.sample(d, i["text"], i["style"], L=L, T=T, noise=i["noise"])
    assert d.persistent_plans() == 0
    # the persistent step under another word than the default: the same bodies select at run time
    m = _model(WT << SHIFT["C"], extra={"DHW_PERSIST": "1"})
    out = dhg_amd.sample(m, i["text"], i["style"], L=L, T=T, noise=i["noise"]).cpu()
    assert m.persistent_plans() == 1
    assert torch.equal(ref[1], out), "persistent launch, class C alone"


def test_bad_policy_value_is_refused():
    with pytest.raises(Exception) as e:
        _model(3)
    assert "DHW_STORE_POLICY" in str(e.value)
