"""Second-order multistep sampling on the host side (no GPU needed; include/dhw.h dhw_dpm_*): the four C-ABI
symbols are declared, exported and bound, and their argument checks answer without a device; ``sample_ddim(order=)`` and the
front ends check ``order`` before any device is touched; the command lines parse ``--order``; the coefficient table the library
uses (dhw_dpm_coefs) against the DDIM table bit for bit and against float64 Python within an ulp; the rule itself
(tests/solver_ref.py) on a problem with a known answer: order 2 at S calls is closer than order 1 at 2S, and the float32
statement stays within 16 ulp of the float64 one; and the host arithmetic (csrc/step/solver_host.h) alone under
AddressSanitizer + UBSan."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, quality, spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ddim_ref  # noqa: E402
import solver_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, T = 2, 64, 9
ENTRIES = (("dhw_dpm_coefs", 5), ("dhw_dpm_update", 12), ("dhw_dpm_sample", 17), ("dhw_guided_dpm_sample", 18))


# ---------------------------------------------------------------- the C-ABI
def test_dpm_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dhw.h")) as f:
        header = f.read()
    for name, nargs in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert m.group(1).count(",") + 1 == nargs, name                    # the declaration's own argument count
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    # the two sampling entries are the ddim entries' argument lists plus `order` behind S
    for dpm, ddim in (("dhw_dpm_sample", "dhw_ddim_sample"), ("dhw_guided_dpm_sample", "dhw_guided_ddim_sample")):
        a, d = _lib.SIGNATURES[dpm][1], _lib.SIGNATURES[ddim][1]
        assert a[:10] == d[:10] and a[10] is C.c_int and a[11:] == d[10:]
    l = _lib.lib()
    lv = (C.c_int32 * 1)(0)
    # a null handle is refused by the argument checks, which run before any HIP call: these answer without a GPU
    assert l.dhw_dpm_sample(None, None, None, 1, 8, 1, None, 1, lv, 1, 2, None, 0, 0, None, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    assert l.dhw_guided_dpm_sample(None, None, None, 1, 8, 1, None, 1, lv, 1, 2, None, None, 0, 0, None, None, None) == -1
    assert "null handle" in l.dhw_last_error(None).decode()
    # nothing new is re-exported beyond what _lib binds: the keyword lives on sample_ddim
    assert not any(hasattr(dhg_amd, n) for n in ("sample_dpm", "dpm_coefs"))


def _coefs(T_, levels, order, rc_want=0):
    l = _lib.lib()
    S = len(levels)
    out = (C.c_float * (9 * max(1, S)))()
    rc = l.dhw_dpm_coefs(T_, (C.c_int32 * max(1, S))(*levels), S, order, out)
    assert rc == rc_want, l.dhw_last_error(None).decode()
    return np.array(out, np.float32).reshape(max(1, S), 9)[:S]


def test_dpm_coefs_checks_answer_without_a_device():
    l = _lib.lib()
    out = (C.c_float * 90)()

    def lv(*v):
        return (C.c_int32 * max(1, len(v)))(*v)

    for args, what in (((0, lv(0), 1, 2, out), "T = 0"), ((2 ** 29 + 1, lv(0), 1, 2, out), "2^29"), ((9, lv(8, 0), 0, 2, out), "S = 0"),
                       ((9, lv(*range(9, -1, -1)), 10, 2, out), "S = 10 must lie in [1, T = 9]"), ((9, None, 2, 2, out), "levels is NULL"),
                       ((9, lv(9, 0), 2, 2, out), "levels[0] = 9"), ((9, lv(3, -1), 2, 2, out), "levels[1] = -1"),
                       ((9, lv(4, 4), 2, 2, out), "strictly decreasing"), ((9, lv(0, 8), 2, 2, out), "levels[1] = 8 is not below levels[0] = 0"),
                       ((9, lv(8, 0), 2, 0, out), "order = 0"), ((9, lv(8, 0), 2, 3, out), "order = 3"), ((9, lv(8, 0), 2, -1, out), "order = -1"),
                       ((9, lv(8, 0), 2, 2, None), "(out)")):
        rc = l.dhw_dpm_coefs(*args)
        msg = l.dhw_last_error(None).decode()
        assert rc == -1 and what in msg and "dhw_dpm_coefs" in msg, (what, rc, msg)
    assert l.dhw_dpm_coefs(9, lv(8, 4, 0), 3, 2, out) == 0


def test_dpm_update_checks_answer_without_a_device():
    """dhw_dpm_update takes no handle: its refusals are read through dhw_last_error(NULL), each naming its argument."""
    l = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    row = (C.c_float * 9)(2.0, 0.9, 0.4, 0.95, 0.3, 1.5, 0.5, 0.75, 0.2)
    good = dict(base=p, eps=p, pen=None, lens=None, scale=None, hist=p, B=1, L=8, coef=row, out=p, out3=None)
    for change, what in ((dict(B=0), "B=0"), (dict(L=0), "L=0"), (dict(B=2 ** 16, L=2 ** 15), "below 2^31"), (dict(B=2 ** 15, L=2 ** 15, scale=p), "below 2^31"),
                         (dict(base=None), "(base)"), (dict(eps=None), "(eps)"), (dict(hist=None), "(hist)"), (dict(coef=None), "(coef)"),
                         (dict(out=None), "out and out3"), (dict(out3=p), "(pen"),
                         (dict(coef=(C.c_float * 9)(0.0)), "coef[0] = 0"), (dict(coef=(C.c_float * 9)(3.0)), "coef[0] = 3"),
                         (dict(coef=(C.c_float * 9)(1.5)), "coef[0] = 1.5"), (dict(coef=(C.c_float * 9)(float("nan"))), "coef[0] = nan"),
                         (dict(base=p + 4), "base must be 8-byte aligned"), (dict(eps=p + 4), "eps must be 8-byte aligned"),
                         (dict(hist=p + 4), "hist must be 8-byte aligned"), (dict(out=p + 4), "out must be 8-byte aligned"),
                         (dict(lens=p + 2), "4-byte aligned"), (dict(scale=p + 2), "4-byte aligned"), (dict(out3=p + 2, pen=p), "4-byte aligned"),
                         (dict(out3=p, pen=p + 2), "4-byte aligned")):
        a = {**good, **change}
        rc = l.dhw_dpm_update(a["base"], a["eps"], a["pen"], a["lens"], a["scale"], a["hist"], a["B"], a["L"], a["coef"], a["out"], a["out3"], None)
        msg = l.dhw_last_error(None).decode()
        assert rc == -1 and what in msg and "dhw_dpm_update" in msg, (what, rc, msg)


# ---------------------------------------------------------------- sample_ddim(order=) before any device is touched
def _model():
    m = dhg_amd.DiffusionModel(2, precision="fp32", max_B=4, max_L=64, max_Lt=4).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()})
    return m


def _no_device(monkeypatch, m):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(m, "_device", boom)
    monkeypatch.setattr(m, "_ensure_handle", boom)


TEXT, STYLE = torch.ones((B, 4), dtype=torch.int64), torch.zeros((B, 14, 1280))


@pytest.mark.parametrize("order", [0, 3, -1, 2.0, "2", True, None, [2]])
def test_sample_ddim_rejects_a_bad_order_before_any_device_access(monkeypatch, order):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(ValueError, match="order = .* must be 1 .* or 2"):
        dhg_amd.sample_ddim(m, TEXT, STYLE, T=T, L=L, steps=4, order=order)
    with pytest.raises(ValueError, match="order = "):   # it is the first check: nothing else is looked at
        dhg_amd.sample_ddim(m, None, None, order=order)


@pytest.mark.parametrize("kw", [dict(steps=4), dict(steps=1), dict(levels=[8, 3, 0]), dict(lengths=[8, 64]), dict(guidance=2.5), dict(guidance=[0.0, 1.0], lengths=[8, 64]),
                                dict(latent=torch.zeros((B, L, 2)), return_latent=True)])
@pytest.mark.parametrize("order", [1, 2, np.int64(2)])
def test_a_valid_order_gets_as_far_as_the_device(monkeypatch, kw, order):
    m = _model()
    _no_device(monkeypatch, m)
    with pytest.raises(AssertionError, match="device was touched"):
        dhg_amd.sample_ddim(m, TEXT, STYLE, **{**dict(T=T, L=L), **kw}, order=order)
    # the other rules stay in force with the keyword
    with pytest.raises(ValueError, match="steps or levels, not both"):
        dhg_amd.sample_ddim(m, TEXT, STYLE, T=T, L=L, steps=3, levels=[8, 4, 0], order=order)


def test_invert_and_transfer_take_no_order(monkeypatch):
    m = _model()
    _no_device(monkeypatch, m)
    strokes = torch.zeros((B, L, 3))
    with pytest.raises(TypeError, match="order"):
        dhg_amd.invert(m, strokes, TEXT, STYLE, T=T, steps=4, order=2)
    with pytest.raises(ValueError, match="unknown keyword"):
        dhg_amd.transfer(strokes, TEXT, STYLE, STYLE, m, T=T, steps=4, order=2)
    assert "no one-step inverse" in dhg_amd.invert.__doc__ and "no one-step inverse" in dhg_amd.transfer.__doc__


def test_order_reaches_the_deterministic_sampler(monkeypatch):
    """infer / infer_batch / write_page hand ``order`` to sample_ddim next to ``steps``; without it the call is today's,
    argument for argument; without ``steps`` it is refused."""
    from dhg_amd import inference
    calls = []

    def fake_ddim(model, text, sv, **kw):
        calls.append(("ddim", kw))
        return torch.zeros((text.shape[0], kw["L"], 3))

    def fake_sample(model, text, sv, **kw):
        calls.append(("sample", kw))
        return torch.zeros((text.shape[0], kw["L"], 3))

    monkeypatch.setattr(inference, "sample_ddim", fake_ddim)
    monkeypatch.setattr(inference, "sample", fake_sample)
    sv = torch.zeros((1, 14, 1280))
    inference.infer("Hi", sv, None, T=60, seed=4, steps=4, order=2)
    assert calls[-1][0] == "ddim" and calls[-1][1]["order"] == 2 and calls[-1][1]["levels"] == [59, 39, 19, 0]
    inference.infer_batch(["Hi", "Rabbit"], sv, None, T=9, steps=2, order=1, guidance=2.0)
    assert calls[-1][0] == "ddim" and calls[-1][1]["order"] == 1 and calls[-1][1]["guidance"] == 2.0
    inference.infer("Hi", sv, None, T=60, steps=4)
    inference.infer_batch(["Hi"], sv, None, T=9, steps=2)
    assert all(c[0] == "ddim" and "order" not in c[1] for c in calls[-2:])
    for call in (lambda **k: inference.infer("Hi", sv, None, **k), lambda **k: inference.infer_batch(["Hi"], sv, None, **k),
                 lambda **k: inference.write_page("Hi there", sv, None, **k)):
        with pytest.raises(ValueError, match="order belongs to deterministic sampling"):
            call(order=2)
        with pytest.raises(ValueError, match="order = 3"):
            call(steps=4, order=3)
    for fn in (inference.infer_file, inference.infer_file_batch, inference.write_page_file):
        with pytest.raises(ValueError, match="order belongs to deterministic sampling"):
            fn("Hi" if fn is not inference.infer_file_batch else ["Hi"], "style.npy", experiment_path="exp", order=2)


def test_sampler_of_accepts_order_only_with_steps_or_levels():
    assert quality._sampler_of(dict(steps=10, order=2)) is True and quality._sampler_of(dict(levels=[8, 0], order=1, T=9, guidance=2.0)) is True
    with pytest.raises(TypeError, match="unknown sampler keyword.* order for sample"):
        quality._sampler_of(dict(order=2))
    with pytest.raises(TypeError, match="order"):
        quality._sampler_of(dict(T=9, diffusion_mode="new", order=2), "sample_metrics")


# ---------------------------------------------------------------- the command lines
def test_infer_cli_order(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import infer
    finally:
        sys.path.remove(ROOT)
    seen = {}

    def fake_batch(prompts, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(batch=prompts, **kw)
        return [np.zeros((8, 3), np.float32) for _ in prompts]

    def fake_one(prompt, source, config_path, checkpoint_path, experiment_path, output, mode, **kw):
        seen.update(one=prompt, **kw)
        return np.zeros((8, 3), np.float32)

    monkeypatch.setattr(dhg_amd, "infer_file_batch", fake_batch)
    monkeypatch.setattr(dhg_amd, "infer_file", fake_one)
    f = tmp_path / "lines.txt"
    f.write_text("first line\nsecond\n")
    for order in (1, 2):
        seen.clear()
        infer.main(["--prompts-file", str(f), "style.npy", "--experiment-path", "exp", "--steps", "12", "--order", str(order)])
        assert seen["steps"] == 12 and seen["order"] == order and seen["batch"] == ["first line", "second"]
        seen.clear()
        infer.main(["a prompt", "style.npy", "--experiment-path", "exp", "--steps", "7", "--order", str(order), "--guidance", "2.5"])
        assert seen["steps"] == 7 and seen["order"] == order and seen["guidance"] == 2.5 and seen["one"] == "a prompt"
    seen.clear()
    infer.main(["a prompt", "style.npy", "--experiment-path", "exp", "--steps", "7"])
    assert "order" not in seen   # without the flag: the call of before, argument for argument
    for bad in (["--order", "2"], ["--order", "1"], ["--steps", "4", "--order", "3"], ["--steps", "4", "--order", "0"], ["--steps", "4", "--order", "x"]):
        with pytest.raises(SystemExit):
            infer.main(["a prompt", "style.npy", "--experiment-path", "exp", *bad])


def test_eval_samples_cli_order():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_samples
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    a = eval_samples.parser().parse_args(["--data", "d.pt", "--steps", "10", "20", "--order", "1", "2"])
    assert a.steps == [10, 20] and a.order == [1, 2]
    assert eval_samples.parser().parse_args(["--data", "d.pt", "--steps", "10"]).order == [None]
    with pytest.raises(SystemExit):
        eval_samples.parser().parse_args(["--data", "d.pt", "--steps", "10", "--order", "3"])
    with pytest.raises(SystemExit):   # --order without --steps
        eval_samples.main(["--data", "d.pt", "--order", "2"])


# ---------------------------------------------------------------- the coefficient table the library uses
def _ulp_apart(a, b):
    """distance in float32 ulps between two float32 values of one sign"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("T_", [9, 60])
def test_dpm_coefs_table(T_):
    """First-order rows are the DDIM table's pairs bit for bit with zeros behind them; second-order k0, k1, c4, c5 lie within
    1 float32 ulp of the float64 value from math.log / math.expm1: a double libm result is within an ulp of double, so after one
    rounding to float32 it can land on either neighbour at most."""
    abar = _lib.schedule(T_)[1]
    for S in (1, 2, 3, 4, 9, 20, 60):
        if S > T_:
            continue
        levels = dhg_amd.ddim_levels(T_, S)
        ab = ddim_ref.coefs(levels, T_, abar=abar)
        for order in (1, 2):
            got = _coefs(T_, levels, order)
            assert got.shape == (S, 9)
            want_second = [order == 2 and 0 < j < S - 1 for j in range(S)]
            assert [k == 2.0 for k in got[:, 0]] == want_second and all(k in (1.0, 2.0) for k in got[:, 0])
            if S <= 2 or order == 1:
                assert not (got[:, 0] == 2.0).any()
            for j in range(S):
                pair = np.array([ab[j][0], ab[j][1], ab[j + 1][0], ab[j + 1][1]], np.float32)
                assert np.array_equal(got[j, 1:5].view(np.int32), pair.view(np.int32)), (S, order, j)
                if not want_second[j]:
                    assert np.array_equal(got[j, 5:].view(np.int32), np.zeros(4, np.int32)), (S, order, j)
                    continue
                ref = solver_ref.second_order([(float(a), float(b)) for a, b in ab], j)
                assert all(math.isfinite(v) for v in ref) and ref[0] > 1.0 and ref[1] > 0.0 and 0.0 < ref[2] < 1.0 and ref[3] > 0.0
                for name, g, w in zip(("k0", "k1", "c4", "c5"), got[j, 5:], ref):
                    assert _ulp_apart(g, np.float32(w)) <= 1, (S, j, name, float(g), w)
    # levels of the caller's own choosing, unevenly spread
    got = _coefs(T_, [8, 7, 3, 1, 0], 2)
    assert list(got[:, 0]) == [1.0, 2.0, 2.0, 2.0, 1.0]


def test_solver_ref_table_is_the_library_table():
    """The helper's float32 table against dhw_dpm_coefs: the same rule, so at most the ulp of the test above apart."""
    for T_, S in ((9, 4), (9, 9), (60, 20)):
        levels = dhg_amd.ddim_levels(T_, S)
        got = _coefs(T_, levels, 2)
        want = np.array(solver_ref.table(levels, T_, 2, abar=_lib.schedule(T_)[1]), np.float32)
        assert np.array_equal(got[:, :5], want[:, :5])
        assert np.abs(got[:, 5:].view(np.int32).astype(np.int64) - want[:, 5:].view(np.int32)).max() <= 1


# ---------------------------------------------------------------- the rule on a problem with a known answer
def _gauss_error(S, order, dtype=torch.float64, T_=60):
    levels = dhg_amd.ddim_levels(T_, S)
    start, exact = solver_ref.gaussian_problem(levels, T_)
    out = solver_ref.sample(solver_ref.gaussian_denoiser(0.7, 0.5), None, None, None, levels, T_, start, order=order, dtype=dtype)
    assert out.dtype == dtype and torch.equal(out[..., 2], torch.zeros_like(out[..., 2]))
    return out[..., :2], (out[..., :2].double() - exact).abs().max().item()


@pytest.mark.parametrize("S", [4, 5, 8, 10, 15, 30])
def test_order_two_at_s_calls_beats_order_one_at_twice_as_many(S):
    """T = 60, ddim_levels, the exact denoiser of N(0.7, 0.5^2) data, 4096 starts from default_rng(0), float64; the metric is the
    largest distance of the final output from the exact probability-flow solution mu + s z.  Measured (order 2 at S / order 1 at
    2S): 0.205 / 0.353 (S = 4), 0.120 / 0.299 (5), 0.055 / 0.209 (8), 0.047 / 0.192 (10), 0.050 / 0.155 (15), 0.063 / 0.115 (30)."""
    _, e2 = _gauss_error(S, 2)
    _, e1 = _gauss_error(2 * S, 1)
    print(f"S = {S}: order 2 error {e2:.4f}; order 1 at {2 * S} levels {e1:.4f}")
    assert e2 < e1
    assert _gauss_error(S, 1)[1] > e1   # (order 1 does converge: more levels are closer, so the comparison above is not vacuous)


@pytest.mark.parametrize("S", [4, 9, 20, 60])
@pytest.mark.parametrize("order", [1, 2])
def test_float32_statement_stays_within_16_ulp_of_float64(S, order):
    """The float32 statement (float32 schedule, coefficients rounded once, one rounding per operation) against the float64 one on
    the Gaussian problem.  Bound: 16 float32 ulp at max|x| for the whole call.  Measured: at most 1.3e-6 at S = 4 to 60 with
    max|x| = 2.3 (16 ulp = 3.8e-6)."""
    x64, _ = _gauss_error(S, order)
    x32, _ = _gauss_error(S, order, torch.float32)
    err = (x32.double() - x64).abs().max().item()
    bound = 16 * float(np.spacing(np.float32(x64.abs().max().item())))
    print(f"S = {S} order {order}: float32 against float64 {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_solver_ref_orders_agree_where_the_header_says_so():
    """order 1 of the helper is ddim_ref.sample bit for bit; order 2 equals it at S <= 2; a ragged call is each sample alone."""
    g = torch.Generator().manual_seed(5)
    lat = torch.randn((2, 24, 2), generator=g)
    e_fixed, q_fixed = torch.randn((1, 24, 2), generator=g), torch.rand((1, 24), generator=g)

    def den(sd, x, text, sigma, style):   # depends on x and sigma, so that a step's input matters
        n = x.shape[1]
        return e_fixed[:, :n] * sigma.to(x.dtype) + 0.25 * x, q_fixed[:, :n].expand(x.shape[0], n)

    for S in (1, 2, 4, 9):
        levels = dhg_amd.ddim_levels(T, S)
        want = ddim_ref.sample(den, None, None, None, levels, T, lat)
        assert torch.equal(solver_ref.sample(den, None, None, None, levels, T, lat, order=1), want)
        two = solver_ref.sample(den, None, None, None, levels, T, lat, order=2)
        assert torch.equal(two, want) == (S <= 2)
    levels = dhg_amd.ddim_levels(T, 4)
    full = solver_ref.sample(den, None, None, None, levels, T, lat, order=2)
    rag = solver_ref.sample(den, None, [None, None], [None, None], levels, T, lat, order=2, lengths=[24, 16])
    alone = solver_ref.sample(den, None, None, None, levels, T, lat[1:, :16], order=2)
    assert torch.equal(rag[0], full[0]) and torch.equal(rag[1, :16], alone[0]) and torch.equal(rag[1, 16:], torch.zeros((8, 3)))


# ---------------------------------------------------------------- the host arithmetic alone, under ASan + UBSan
def test_solver_host_code_alone_under_sanitizers(tmp_path):
    """tests/cpp/solver_host_check.cpp (csrc/step/solver_host.h only) built with the host compiler under AddressSanitizer + UBSan
    where the toolchain links them (as tests/test_ddim_cpu.py builds its program), run on the CPU: the table against the values
    this test computes, every refusal, and (inside the program) a message buffer shorter than the message."""
    import shutil
    import subprocess
    import warnings
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "solver_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "solver_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("solver_host_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    Tq = 9
    abar = _lib.schedule(Tq)[1]
    abar.tofile(tmp_path / "abar.f32")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

    def run(T_, order, *levels, file="abar.f32"):
        r = subprocess.run([exe, str(tmp_path / file), str(T_), str(order), *map(str, levels)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip().splitlines()

    for levels in ([8, 5, 2, 0], [8], [8, 0], [8, 4, 0], list(range(8, -1, -1)), [8, 7, 3, 1, 0]):
        for order in (1, 2):
            rows = run(Tq, order, *levels)
            assert len(rows) == len(levels)
            want = np.array(solver_ref.table(levels, Tq, order, abar=abar), np.float32)
            lib = _coefs(Tq, levels, order)
            for j, ln in enumerate(rows):
                tag, kind, *vals = ln.split()
                got = np.array([float(kind)] + [float.fromhex(v) for v in vals], np.float32)
                assert tag == "co" and np.array_equal(got.view(np.int32), lib[j].view(np.int32)), (levels, order, ln)   # the program and the library: one header
                assert np.array_equal(got[:5], want[j, :5]) and np.abs(got[5:].view(np.int32).astype(np.int64) - want[j, 5:].view(np.int32)).max() <= 1
    for T_, order, lv, what in ((Tq, 2, [], "S = 0"), (Tq, 2, [Tq], "levels[0] = 9"), (Tq, 2, [4, 4], "strictly decreasing"), (0, 2, [0], "T = 0"),
                                (Tq, 0, [8, 0], "order = 0"), (Tq, 3, [8, 0], "order = 3"), (Tq, -2, [8], "order = -2")):
        (ln,) = run(T_, order, *lv)
        assert ln.startswith("err ") and what in ln, ln
    # tables the rule cannot serve: two levels whose float32 abar coincide (h = 0, or r = 0), a level whose abar is 1 (log-SNR infinite)
    flat = abar.copy()
    flat[3] = flat[4]
    flat.tofile(tmp_path / "flat.f32")
    (ln,) = run(Tq, 2, 8, 4, 3, 0, file="flat.f32")
    assert ln.startswith("err step 1: h = 0") and "finite and positive" in ln, ln
    (ln,) = run(Tq, 2, 8, 4, 3, 1, 0, file="flat.f32")
    assert ln.startswith("err step 1: h = 0"), ln
    (ln,) = run(Tq, 2, 4, 3, 1, 0, file="flat.f32")
    assert ln.startswith("err step 1: r = 0") and "finite and positive" in ln, ln
    one = abar.copy()
    one[0] = 1.0
    one.tofile(tmp_path / "one.f32")
    (ln,) = run(Tq, 2, 8, 4, 0, file="one.f32")
    assert ln.startswith("err step 1: h = inf"), ln
    assert run(Tq, 1, 8, 4, 3, 0, file="flat.f32")[0].startswith("co 1 ")   # order 1 computes no h: the DDIM table as it is
    assert run(Tq, 2, 4, 3, file="flat.f32")[0].startswith("co 1 ")         # S = 2: no second-order step either
