"""Scoring (include/dhw.h dhw_score; ``score``, ``infer_batch(..., candidates=)``, ``infer.py --score``): the denoising
objective of given strokes at chosen noise levels.  Runs on the MI355X only (-m gpu).

Contract (include/dhw.h, rules 1-7): the generator stream is iteration 2^29 + i, keyed by the schedule index; rows past a
sample's length are never read; a ragged row equals its alone run, a shard its rows — all bitwise; a score call leaves
the sampler's cached graphs alone.  Against the CPU helper (tests/score_ref.py, proven on the CPU by
tests/test_score_cpu.py) the bound is derived from the denoiser's own tolerance (test_gpu_parity.TOL: |eps - eps_ref| <=
de, |pen - pen_ref| <= dp), with d = z - eps_ref, q = pen_ref, n rows:
    score term   |D| <= 2 de mean_p(|d0| + |d1|) + 2 de^2 + n 2^-24 |ref|      ((d + e)^2 - d^2 = 2 d e + e^2, per component)
    pen term     |D| <= abar dp mean_p(1 / min(q, 1 - q)) + n 2^-24 |ref|      (|d/dq BCE| <= 1 / min(q, 1 - q))
the last summand covering the order of the fp32 sums.
Measured errors: not recorded yet — every oracle test prints error and bound per level and sample before it
asserts.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, spec
from oracle import ref_cpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"fp32": dict(eps=2e-5, pen=2e-5), "bf16": dict(eps=2e-2, pen=5e-3)}   # test_gpu_parity.TOL
B, L, Lt, T = 3, 72, 7, 9
LENS = [72, 40, 8]
LEVELS = [0, 4, 8]
_MODELS = {}
_CACHE = {}


def _sd():
    return {k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}


def fresh_model(prec, **cap):
    m = dhg_amd.DiffusionModel(2, precision=prec, **{**dict(max_B=8, max_L=488, max_Lt=40), **cap}).eval()
    m.load_state_dict(_sd(), strict=True)
    return m


def get_model(prec):
    if prec not in _MODELS:
        _MODELS[prec] = fresh_model(prec)
    return _MODELS[prec]


def _strokes(b, l, seed):
    """[b,l,3]: dx, dy ~ N(0,1), pen in {0,1}."""
    k = torch.randn((b, l, 3), generator=torch.Generator().manual_seed(seed))
    k[..., 2] = (k[..., 2] > 0.5).float()
    return k


def _noise(k, b, l, seed):
    return torch.randn((k, b, l, 2), generator=torch.Generator().manual_seed(seed))


def _inputs(b, l, lt, seed):
    inp = spec.synthetic_inputs(b, l, lt, seed=seed, T=1)
    return torch.from_numpy(inp["text"]), torch.from_numpy(inp["style"])


def _bounds(details, ref_row, tol, n):
    """(score bound, pen bound) of one (level, sample) from the oracle's own values; details: dict(z, eps, q, abar) of [1,n,..]."""
    d = (details["z"] - details["eps"]).abs().double()
    q = details["q"].double()
    de, dp = tol["eps"], tol["pen"]
    slack = n * 2.0 ** -24
    bs = 2 * de * d.sum(dim=-1).mean().item() + 2 * de * de + slack * abs(ref_row[0].item())
    bp = details["abar"] * dp * (1.0 / torch.minimum(q, 1 - q)).mean().item() + slack * abs(ref_row[1].item())
    return bs, bp


def _oracle_case():
    """B=2, L=40, Lt=5, T=9, levels [0,4,8], external noise: inputs and the CPU reference, built once and shared."""
    if "oracle" not in _CACHE:
        tx, sv = _inputs(2, 40, 5, 5)
        st, nz = _strokes(2, 40, 41), _noise(3, 2, 40, 42)
        det = []
        ref = score_ref.score(ref_cpu.forward, _sd(), st, tx, sv, LEVELS, T, nz, lengths=[40, 40], details=det)
        _CACHE["oracle"] = dict(text=tx, style=sv, strokes=st, noise=nz, ref=ref, details=det)
    return _CACHE["oracle"]


def _check_against(got, ref, details, lens, tol, what):
    """got, ref [B,K,2]; details in score_ref's ragged order (k major, b minor).  Prints each figure, then asserts."""
    Bq, K = ref.shape[:2]
    worst = [0.0, 0.0]
    fails = []
    for k in range(K):
        for b in range(Bq):
            bs, bp = _bounds(details[k * Bq + b], ref[b, k], tol, lens[b])
            es, ep = abs(got[b, k, 0].item() - ref[b, k, 0].item()), abs(got[b, k, 1].item() - ref[b, k, 1].item())
            print(f"{what} level#{k} sample {b} (n={lens[b]}): score {ref[b, k, 0].item():.6f} err {es:.3e} bound {bs:.3e} | "
                  f"pen {ref[b, k, 1].item():.6f} err {ep:.3e} bound {bp:.3e}")
            worst = [max(worst[0], es / bs), max(worst[1], ep / bp)]
            if not (es <= bs and ep <= bp):
                fails.append((k, b, es, bs, ep, bp))
    print(f"{what}: worst error / bound: score {worst[0]:.3f}, pen {worst[1]:.3f}")
    assert not fails, fails


# ---------------------------------------------------------------- 1. the oracle, fp32
def test_oracle_fp32():
    """fp32 handle against score_ref, bound derived from TOL["fp32"] (module docstring); every figure is printed first."""
    o = _oracle_case()
    got = dhg_amd.score(get_model("fp32"), o["strokes"].cuda(), o["text"].cuda(), o["style"].cuda(), levels=LEVELS, T=T, noise=o["noise"].cuda()).cpu()
    assert tuple(got.shape) == (2, 3, 2) and torch.isfinite(got).all()
    _CACHE["oracle_fp32"] = got
    _check_against(got, o["ref"], o["details"], [40, 40], TOL["fp32"], "fp32 vs score_ref")


# ---------------------------------------------------------------- 2. bf16 tracks fp32
def test_bf16_tracks_fp32():
    """Same inputs, same formulas with TOL["bf16"], against the fp32 handle's result."""
    o = _oracle_case()
    args = (o["strokes"].cuda(), o["text"].cuda(), o["style"].cuda())
    f32 = _CACHE.get("oracle_fp32")
    if f32 is None:
        f32 = dhg_amd.score(get_model("fp32"), *args, levels=LEVELS, T=T, noise=o["noise"].cuda()).cpu()
    got = dhg_amd.score(get_model("bf16"), *args, levels=LEVELS, T=T, noise=o["noise"].cuda()).cpu()
    assert torch.isfinite(got).all()
    _check_against(got, f32, o["details"], [40, 40], TOL["bf16"], "bf16 vs fp32")


# ---------------------------------------------------------------- 3. reduction sizes: more than one pass, a partial wave, less than a wave
def test_reduction_sizes_ragged_rows_match_oracle_and_their_alone_runs():
    lens, Lq, lv = [264, 72, 8], 264, [4]
    tx, sv = _inputs(3, Lq, 5, 43)
    st, nz = _strokes(3, Lq, 44), _noise(1, 3, Lq, 45)
    m = get_model("fp32")
    got = dhg_amd.score(m, st.cuda(), tx.cuda(), sv.cuda(), lengths=lens, levels=lv, T=T, noise=nz.cuda()).cpu()
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        alone = dhg_amd.score(m, st[b:b + 1, :n].cuda(), tx[b:b + 1].cuda(), sv[b:b + 1].cuda(), levels=lv, T=T, noise=nz[:, b:b + 1, :n].cuda()).cpu()
        assert torch.equal(got[b], alone[0]), (b, got[b], alone[0])
    det = []
    ref = score_ref.score(ref_cpu.forward, _sd(), st, tx, sv, lv, T, nz, lengths=lens, details=det)
    _check_against(got, ref, det, lens, TOL["fp32"], "ragged fp32 vs score_ref")


# ---------------------------------------------------------------- 4. rows past a sample's length are never read
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_rows_past_the_length_are_not_read(prec):
    m = get_model(prec)
    tx, sv = _inputs(B, L, Lt, 46)
    st, nz = _strokes(B, L, 47), _noise(3, B, L, 48)
    clean = dhg_amd.score(m, st.cuda(), tx.cuda(), sv.cuda(), lengths=LENS, levels=LEVELS, T=T, noise=nz.cuda()).cpu()
    for b, n in enumerate(LENS):
        st[b, n:] = float("nan")
        nz[:, b, n:] = float("nan")
    dirty = dhg_amd.score(m, st.cuda(), tx.cuda(), sv.cuda(), lengths=LENS, levels=LEVELS, T=T, noise=nz.cuda()).cpu()
    assert torch.isfinite(clean).all() and torch.equal(clean, dirty)
    gen = [dhg_amd.score(m, s.cuda(), tx.cuda(), sv.cuda(), lengths=LENS, levels=LEVELS, T=T, seed=3).cpu() for s in (torch.nan_to_num(st), st)]
    assert torch.isfinite(gen[0]).all() and torch.equal(gen[0], gen[1])


# ---------------------------------------------------------------- 5. the generator stream is iteration 2^29 + i
def test_generator_stream_is_keyed_by_the_schedule_index():
    m = get_model("fp32")
    tx, sv = (x.cuda() for x in _inputs(B, L, Lt, 49))
    st = _strokes(B, L, 50).cuda()
    seed, first = 11, 4
    drawn = dhg_amd.score(m, st, tx, sv, levels=LEVELS, T=T, seed=seed, first_sample=first).cpu()
    nz = torch.stack([m.debug_randn(seed, first, B, L, 2 ** 29 + i) for i in LEVELS])
    given = dhg_amd.score(m, st, tx, sv, levels=LEVELS, T=T, noise=nz.cuda()).cpu()
    assert torch.isfinite(drawn).all() and torch.equal(drawn, given)
    wrong = torch.stack([m.debug_randn(seed, first, B, L, 2 ** 29 + k) for k in range(3)])   # keyed by k instead of i
    assert not torch.equal(dhg_amd.score(m, st, tx, sv, levels=LEVELS, T=T, noise=wrong.cuda()).cpu()[:, 1:], drawn[:, 1:])
    one = dhg_amd.score(m, st, tx, sv, levels=[4], T=T, seed=seed, first_sample=first).cpu()
    assert torch.equal(one[:, 0], drawn[:, 1])
    dup = dhg_amd.score(m, st, tx, sv, levels=[8, 4, 8, 0], T=T, seed=seed, first_sample=first).cpu()
    assert torch.equal(dup[:, 0], dup[:, 2]) and torch.equal(dup[:, 0], drawn[:, 2]) and torch.equal(dup[:, 1], drawn[:, 1]) and torch.equal(dup[:, 3], drawn[:, 0])


# ---------------------------------------------------------------- 6. sharding
def _shard_case(m):
    Bs = 4
    tx, sv = (x.cuda() for x in _inputs(Bs, L, Lt, 51))
    st = _strokes(Bs, L, 52).cuda()
    lens = [72, 40, 8, 64]
    kw = dict(levels=LEVELS, T=T, seed=6)
    full = dhg_amd.score(m, st, tx, sv, lengths=lens, first_sample=0, **kw).cpu()
    mid = dhg_amd.score(m, st[1:3].contiguous(), tx[1:3].contiguous(), sv[1:3].contiguous(), lengths=lens[1:3], first_sample=1, **kw).cpu()
    halves = [dhg_amd.score(m, st[s:s + 2].contiguous(), tx[s:s + 2].contiguous(), sv[s:s + 2].contiguous(), lengths=lens[s:s + 2],
                            first_sample=s, **kw).cpu() for s in (0, 2)]
    return full, mid, torch.cat(halves)


def test_shards_equal_the_whole_batch():
    full, mid, parts = _shard_case(get_model("bf16"))
    assert torch.isfinite(full).all() and torch.equal(full[1:3], mid) and torch.equal(full, parts)
    _CACHE["shard_full"] = full


def test_shards_equal_the_whole_batch_on_two_streams(monkeypatch):
    monkeypatch.setenv("DHW_STREAMS", "2")   # (read at dhw_create: the handle owns two workspaces and a side stream)
    m = fresh_model("bf16")
    tx1, sv1 = _inputs(1, 8, 1, 1)
    dhg_amd.sample(m, tx1.cuda(), sv1.cuda(), L=8, T=1)   # creates the handle
    monkeypatch.delenv("DHW_STREAMS")
    assert _lib.lib().dhw_set_streams(m._handle, 2) == 2
    full, mid, parts = _shard_case(m)
    assert torch.equal(full[1:3], mid) and torch.equal(full, parts)
    one = _CACHE.get("shard_full")
    if one is None:
        one, _, _ = _shard_case(get_model("bf16"))
    assert torch.equal(full, one)


# ---------------------------------------------------------------- 7. the plain paths are untouched
@pytest.mark.parametrize("lengths", [None, LENS])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_score_call_leaves_the_sampler_alone(prec, lengths):
    m = fresh_model(prec)
    tx, sv = (x.cuda() for x in _inputs(B, L, Lt, 53))
    kw = dict(L=L, T=3, seed=7, first_sample=2, lengths=lengths)
    first = dhg_amd.sample(m, tx, sv, **kw).cpu()                 # captures the graph
    sc = dhg_amd.score(m, first.cuda(), tx, sv, lengths=lengths, T=3, seed=9, pen_round=True).cpu()
    again = dhg_amd.sample(m, tx, sv, **kw).cpu()                 # replays it
    assert torch.isfinite(first).all() and torch.isfinite(sc).all() and torch.equal(first, again)
    assert torch.equal(dhg_amd.score(m, first.cuda(), tx, sv, lengths=lengths, T=3, seed=9, pen_round=True).cpu(), sc)   # bit-deterministic


# ---------------------------------------------------------------- 8. errors at the C-ABI
def _raw_call(m, st, tx, sv, out, lens, T_, levels, Lq=None):
    lv = (C.c_int32 * max(1, len(levels)))(*levels)
    ln = (C.c_int32 * len(lens))(*lens) if lens is not None else None
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().dhw_score(m._handle, st.data_ptr(), tx.data_ptr(), sv.data_ptr(), tx.shape[0], Lq or st.shape[1], tx.shape[1], ln, T_, lv, len(levels),
                              None, 1, 0, out.data_ptr(), s)
    return rc, _lib.lib().dhw_last_error(m._handle).decode()


def test_c_abi_rejects_bad_arguments_and_keeps_the_handle():
    m = get_model("bf16")
    tx, sv = (x.cuda() for x in _inputs(B, L, Lt, 54))
    st = _strokes(B, L, 55).cuda()
    ref = dhg_amd.score(m, st, tx, sv, lengths=LENS, levels=LEVELS, T=T, seed=1).cpu()
    out = torch.full((3, B, 2), float("nan"), device="cuda")
    for args, what in (((LENS, T, []), "K = 0"), ((LENS, T, [0, T]), "levels[1] = 9"), ((LENS, T, [0] * (T + 1)), "K = 10"),
                       (([72, 44, 8], T, LEVELS), "lens[1] = 44"), ((LENS, 0, LEVELS), "T = 0")):
        rc, msg = _raw_call(m, st, tx, sv, out, *args)
        assert rc == -1 and what in msg and "dhw_score" in msg, (what, rc, msg)
    rc, msg = _raw_call(m, st, tx, sv, out, None, T, LEVELS, Lq=68)
    assert rc == -1 and "L=68" in msg, (rc, msg)
    assert torch.isnan(out).all()   # nothing was launched
    rc, msg = _raw_call(m, st, tx, sv, out, LENS, T, LEVELS)
    assert rc == 0, msg
    assert torch.equal(out.cpu().transpose(0, 1), ref)


def test_persistent_step_handle_scores(monkeypatch):
    monkeypatch.setenv("DHW_PERSIST", "1")
    m = fresh_model("bf16")
    tx, sv = (x.cuda() for x in _inputs(B, L, Lt, 54))
    st = _strokes(B, L, 55).cuda()
    got = dhg_amd.score(m, st, tx, sv, lengths=LENS, levels=LEVELS, T=T, seed=1).cpu()   # handle created under the switch
    monkeypatch.delenv("DHW_PERSIST")
    assert torch.equal(got, dhg_amd.score(get_model("bf16"), st, tx, sv, lengths=LENS, levels=LEVELS, T=T, seed=1).cpu())


# ---------------------------------------------------------------- 9. best of N
def test_best_of_n_returns_the_lowest_scoring_candidate():
    prompts, N, Tq, seed, first = ["Hi", "Rabbit"], 3, 3, 5, 2
    m = get_model("bf16")
    sv = _inputs(1, 8, 1, 56)[1].cuda()
    tok = dhg_amd.Tokenizer()
    ids = [tok.encode(p) for p in prompts]
    lens = [dhg_amd.stroke_length(len(i)) for i in ids]
    assert lens[0] != lens[1]
    Bq = len(prompts)
    want, totals = [], []
    for b in range(Bq):
        tx = torch.tensor([ids[b]], dtype=torch.int64).cuda()
        cands, tot = [], []
        for j in range(N):
            idx = first + j * Bq + b
            line = dhg_amd.sample(m, tx, sv, L=lens[b], T=Tq, seed=seed, first_sample=idx)
            sc = dhg_amd.score(m, line, tx, sv, T=Tq, seed=seed, first_sample=idx, pen_round=True).cpu()
            cands.append(line.cpu().numpy()[0])
            tot.append(sc[0].double().sum(dim=1).mean().item())
        print(f"prompt {b}: candidate totals {tot}")
        assert all(np.isfinite(tot))
        want.append(cands[int(np.argmin(tot))])   # (argmin: the first of equal minima)
        totals.append(tot)
    got = dhg_amd.infer_batch(prompts, sv, m, T=Tq, seed=seed, first_sample=first, candidates=N)
    assert [g.shape for g in got] == [(n, 3) for n in lens]
    for b in range(Bq):
        assert np.array_equal(got[b], want[b]), b
    small = fresh_model("bf16", max_B=2)   # one candidate round per call: the split changes nothing
    again = dhg_amd.infer_batch(prompts, sv, small, T=Tq, seed=seed, first_sample=first, candidates=N)
    assert all(np.array_equal(a, g) for a, g in zip(again, got))
    # candidates = 1: the call of before
    one = dhg_amd.infer_batch(prompts, sv, m, T=Tq, seed=seed, first_sample=first, candidates=1)
    tx, ln, svb = dhg_amd.inference._encode_batch("test", prompts, sv)
    plain = dhg_amd.sample(m, tx, svb, L=max(ln), T=Tq, seed=seed, first_sample=first, lengths=ln).cpu().numpy()
    assert all(np.array_equal(one[b], plain[b, :ln[b]]) for b in range(Bq))
    assert all(np.array_equal(one[b], dhg_amd.infer_batch(prompts, sv, m, T=Tq, seed=seed, first_sample=first)[b]) for b in range(Bq))


# ---------------------------------------------------------------- 10. the command line
def test_infer_cli_scores_the_strokes_it_saved(tmp_path, monkeypatch, capsys):
    """The pattern of test_infer_file_end_to_end: infer.py --candidates --save-strokes, then infer.py --score on that file."""
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    (tmp_path / "config.yml").write_text("training_args:\n  att_layers_num: 2\n  channels: 128\n  dropout: 0.0\n")
    torch.save({"state_dict": _sd()}, tmp_path / "checkpoint_2000.pth")
    np.save(tmp_path / "style.npy", spec.synthetic_inputs(1, 8, 1, seed=9)["style"][0])
    (tmp_path / "lines.txt").write_text("Hi there\nRabbit\n")
    monkeypatch.chdir(tmp_path)
    common = ["--prompts-file", "lines.txt", "style.npy", "--experiment-path", str(tmp_path)]
    infer.main(common + ["--save-strokes", "lines.npy", "--renderer", "gpu", "--output", "page", "--candidates", "2"])
    assert (tmp_path / "page_0.png").stat().st_size > 0 and (tmp_path / "page_1.png").stat().st_size > 0
    saved = np.load(tmp_path / "lines.npy")
    pngs = sorted(p.name for p in tmp_path.glob("*.png"))
    capsys.readouterr()
    infer.main(common + ["--score", "lines.npy"])
    lines = capsys.readouterr().out.strip().splitlines()
    print("\n".join(lines))
    assert len(lines) == 2 and sorted(p.name for p in tmp_path.glob("*.png")) == pngs   # no images written
    lens = [dhg_amd.stroke_length(len(dhg_amd.Tokenizer().encode(p))) for p in ("Hi there", "Rabbit")]
    assert saved.shape == (2, max(lens), 3)
    for i, ln in enumerate(lines):
        f = ln.split()
        assert f[:2] == ["line", f"{i}:"] and int(f[f.index("length") + 1]) == lens[i]
        vals = [float(f[f.index(k) + 1]) for k in ("score", "pen", "total")]
        assert all(np.isfinite(vals)) and abs(vals[0] + vals[1] - vals[2]) <= 1e-4 * abs(vals[2])
