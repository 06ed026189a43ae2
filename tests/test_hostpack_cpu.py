"""The pure host code every GEMM kernel's weight layout and every state_dict load go through (csrc/host/convert.h,
csrc/host/weight_store.h), pinned on the CPU: tests/cpp/hostpack_check.cpp is compiled with the host C++ compiler (under
AddressSanitizer + UBSan where the toolchain links them), run once, and what it wrote is compared with numpy / torch here."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "hostpack_check.cpp")


def _compiler():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return c
    c = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    assert os.path.exists(c), "no host C++ compiler found"
    return c


def _f2bf_inputs():
    rng = np.random.default_rng(7)
    rnd = np.concatenate([rng.standard_normal(2048).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 2048).astype(np.float32),
                          rng.integers(0, 2 ** 32, 2048, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    rnd = rnd[~np.isnan(rnd)]   # (NaN payloads: checked separately, torch canonicalises them)
    special = np.array([
        0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0xbf808000, 0xbf818000,   # ties to even (down / up), just above / below a tie
        0x00000000, 0x80000000, 0x7f800000, 0xff800000,                           # +-0, +-inf
        0x7f7fffff, 0xff7fffff, 0x7f7f7fff, 0x7f7f8000,                           # the largest finite values (round to inf / stay finite / tie)
        0x00000001, 0x00008000, 0x00018000, 0x007fffff, 0x80000001, 0x00010000,   # denormals
    ], dtype=np.uint32).view(np.float32)
    nans = np.array([0x7fc00000, 0x7f800001, 0xffc12345], dtype=np.uint32).view(np.float32)   # the quiet NaN, NaNs with payloads
    return np.concatenate([rnd, special, nans])


N_NAN = 3   # the tail of _f2bf_inputs


@pytest.fixture(scope="module")
def hostpack(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("hostpack"))
    exe = os.path.join(d, "hostpack_check")
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # The sanitizer runtimes linked into the program itself where the toolchain can (gcc's flags, then clang's), else the shared
    # ones, else a plain build: the comparisons below hold either way, only the memory checking is lost — and that is said aloud.
    for how, extra in (("ASan + UBSan, static runtime", san + ["-static-libasan", "-static-libubsan"]), ("ASan + UBSan, static runtime", san + ["-static-libsan"]),
                       ("ASan + UBSan, shared runtime", san), ("plain (no sanitizer runtime links here)", [])):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    print(f"hostpack_check built: {how}")
    if not extra:
        warnings.warn("hostpack_check was built without AddressSanitizer / UBSan: " + how)
    _f2bf_inputs().tofile(os.path.join(d, "f2bf_in.f32"))
    x = np.array([0.0, -1.5, 3.140625, 65504.0, -2.0 ** -14, 1e-3, 255.0, -0.0], dtype=np.float64)
    x.astype(np.float32).tofile(os.path.join(d, "to_f32_in.f32"))
    x.tofile(os.path.join(d, "to_f32_in.f64"))
    torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().tofile(os.path.join(d, "to_f32_in.bf16"))
    x.astype(np.float16).tofile(os.path.join(d, "to_f32_in.f16"))
    # the program's own sanitizer options; the environment is otherwise inherited untouched.  (Leak checking needs ptrace, which
    # containers often forbid; the instrumented program itself needs no particular place in the link order.)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    r = subprocess.run([exe, d], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}
    return d, lines, x


def _load(d, name, dtype=np.float32):
    return np.fromfile(os.path.join(d, name), dtype=dtype)


def _expected_pack(wf, N, K):
    """pk[((nt*(K/32)+kc)*64+l)*8+j] == wf[(nt*16+(l&15))*K + kc*32 + 8*(l>>4) + j]"""
    nt, kc, l, j = np.meshgrid(np.arange(N // 16), np.arange(K // 32), np.arange(64), np.arange(8), indexing="ij")
    pk = np.empty(N * K, dtype=np.float32)
    pk[(((nt * (K // 32) + kc) * 64 + l) * 8 + j).ravel()] = wf[((nt * 16 + (l & 15)) * K + kc * 32 + 8 * (l >> 4) + j).ravel()]
    return pk


@pytest.mark.parametrize("N,K", [(16, 32), (48, 96)])
def test_pack_mfma_is_the_fragment_index_formula(hostpack, N, K):
    d, _, _ = hostpack
    wf = np.arange(N * K, dtype=np.float32)
    got = _load(d, f"pack_{N}_{K}.f32")
    assert got.shape == (N * K,) and np.array_equal(got, _expected_pack(wf, N, K))
    assert np.array_equal(np.sort(got), wf)   # a permutation: every weight exactly once


def test_conv_flat_then_pack(hostpack):
    d, _, _ = hostpack
    cout = cin = 32
    w = np.arange(cout * cin * 3, dtype=np.float32).reshape(cout, cin, 3)
    flat = w.transpose(0, 2, 1).reshape(cout, 3 * cin)   # [Cout][tap*Cin + c]
    assert np.array_equal(_load(d, "conv_flat.f32"), flat.ravel())
    assert np.array_equal(_load(d, "pack_conv_32_96.f32"), _expected_pack(flat.ravel(), cout, 3 * cin))


def test_f2bf_rounds_like_torch(hostpack):
    d, _, _ = hostpack
    x = _f2bf_inputs()
    got = _load(d, "f2bf_out.u16", np.uint16)
    assert got.shape == x.shape and len(x) > 3000
    ref = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[:-N_NAN], ref[:-N_NAN]), np.flatnonzero(got[:-N_NAN] != ref[:-N_NAN])[:8]
    # A NaN stays a NaN whatever its payload (it never rounds to inf).  Its bits are not compared: torch itself has two answers,
    # 0x7fc0 from its scalar conversion and 0xffff from its vectorised one, and which one runs depends on the build and the CPU.
    for bits in (got[-N_NAN:], ref[-N_NAN:]):
        assert np.isnan((bits.astype(np.uint32) << 16).view(np.float32)).all()


def test_bf2f_and_h2f_over_every_input(hostpack):
    d, _, _ = hostpack
    bits = np.arange(65536, dtype=np.uint32)
    for name, ref in (("bf2f_all.f32", (bits << 16).view(np.float32)), ("h2f_all.f32", bits.astype(np.uint16).view(np.float16).astype(np.float32))):
        got = _load(d, name)
        assert np.array_equal(got, ref, equal_nan=True), name
        ok = ~np.isnan(ref)
        assert np.array_equal(got.view(np.uint32)[ok], ref.view(np.uint32)[ok]), name   # (the sign of zero too)


def test_to_f32_for_each_dtype(hostpack):
    d, lines, x = hostpack
    assert lines["to_f32_known_dtypes"] == ["1"] and lines["to_f32_unknown_dtype"] == ["0"]
    assert np.array_equal(_load(d, "to_f32_out_f32.f32").view(np.uint32), x.astype(np.float32).view(np.uint32))
    assert np.array_equal(_load(d, "to_f32_out_f64.f32").view(np.uint32), x.astype(np.float32).view(np.uint32))
    assert np.array_equal(_load(d, "to_f32_out_bf16.f32"), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert np.array_equal(_load(d, "to_f32_out_f16.f32"), x.astype(np.float16).astype(np.float32))


def test_weight_store(hostpack):
    d, lines, _ = hostpack
    LOADED, UNKNOWN_KEY, SIZE_MISMATCH, BAD_DTYPE = "0", "1", "2", "3"
    assert lines["missing_at_start"] == ["0"]
    assert lines["load_a_f32"] == [LOADED] and lines["missing_after_a"] == ["1"]
    assert lines["load_a_again_bf16"] == [LOADED]                      # loading a key twice: the later tensor wins
    assert np.array_equal(_load(d, "store_a.f32"), np.array([1, 2, 3, 4, 5, -6], dtype=np.float32))
    assert lines["load_unknown_key"] == [UNKNOWN_KEY]
    assert lines["load_wrong_shape"] == [SIZE_MISMATCH] and lines["load_wrong_dim"] == [SIZE_MISMATCH]
    assert lines["load_bad_dtype"] == [BAD_DTYPE] and lines["load_f16_refused"] == [BAD_DTYPE]
    assert lines["missing_after_failures"] == ["1"]                    # a refused load does not count as loaded
    assert lines["load_b_f32"] == [LOADED] and lines["missing_at_end"] == ["-1"]
    assert lines["get_known_first"] == ["0", "size", "4", "fail", "0"]
    assert lines["get_unknown_first"] == ["1", "size_ge_1280", "1", "abs_sum", "0", "fail", "1"]   # zeros, flag raised, reported ...
    assert lines["get_unknown_again_first"] == ["0", "fail", "1"]      # ... once
