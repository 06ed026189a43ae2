"""The tile plan of the stroke kernels (csrc/plan/tile_plan.h) - which compiled ConvBlock / EncoderLayer variant a launch
runs - without a GPU: the header alone under the sanitizers, the case table of tests/blocks_worker.py against the library's plan,
the oddities of the rule as literals, and when the switches are read."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import warnings

from dhg_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blocks_worker as BW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = [256, 0, 0, 0, 1, 1, 0]   # ConvKnobs of the unset environment: wgs, bm, occ, pp, asym, tight, rt


def enc_variants():
    lib, row, out = _lib.lib(), (C.c_int * 11)(), []
    for i in range(lib.dhw_debug_tile_variants(1, 0, row)):
        lib.dhw_debug_tile_variants(1, i, row)
        out.append(tuple(row[:5]))   # f32, DM, BM, fits, chain modes
    return out


def test_tile_plan_alone_under_sanitizers(tmp_path):
    """tests/cpp/tile_plan_check.cpp (csrc/plan/tile_plan.h only) built with the host compiler under AddressSanitizer + UBSan where
    the toolchain links them, run on the CPU: B 1..96 x even row counts 2..1024 x every ConvBlock role x both precisions, every
    switch combination (the grid per combination and the assertions are in the program), and the EncoderLayer row tile under the
    library's fits() table."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    exe = str(tmp_path / "tile_plan_check")
    base = [cxx, "-std=c++17", "-O2", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "tile_plan_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for extra in (san + ["-static-libasan", "-static-libubsan"], san + ["-static-libsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    assert r.returncode == 0, r.stderr
    if not extra:
        warnings.warn("tile_plan_check was built without AddressSanitizer / UBSan (no sanitizer runtime links here)")
    fits = "".join(str(v[3]) for v in enc_variants())
    r = subprocess.run([exe, fits], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    points, enc_points = (int(x) for x in r.stdout.split()[1:])
    assert points > 3 * 10 ** 7 and enc_points > 5 * 10 ** 6, r.stdout
    # a fits() table in which nothing fits must be noticed (the program checks fits of the tile it is given)
    r = subprocess.run([exe, "0" * len(fits)], capture_output=True, text=True)
    assert r.returncode == 1 and "FAILED EncoderLayer" in r.stdout, r.stdout + r.stderr


def test_the_case_table_names_exactly_the_librarys_plan():
    """Every cb<...> / a<...> / bc<...> of every case's `expect` list is the library's plan for that block at (B, L / level) under
    the case's switches, with the chain flag the expected variant carries: the case table is tied to the rule on the CPU (the
    recorded trace profiles/block_variants.txt ties it to the device)."""
    modes = {(dm, bm): m for f32, dm, bm, _, m in enc_variants() if not f32}
    n = 0
    for c in BW.CASES:
        for v in c["expect"]:
            kind, a = BW.expect_args(v)
            if kind == "cb":
                bm, co, nw, occ, upc, ch, cin, tight, pp = a
                knobs = BW.conv_knobs(c)
                if upc:      # a decoder block with the fused input stage: its widths are compiled in
                    shape = (upc, co, {192: 128, 256: 192, 384: 256}[upc])
                elif cin:
                    shape = (cin, co, 0)
                else:        # run-time input width: an encoder block under DHW_CONV_RT, else a decoder block without the fused stage
                    shape = ({128: 128, 192: 128, 256: 192}[co] if knobs[6] else {128: 192, 192: 256, 256: 384}[co], co, 0)
                got = BW.conv_plan("bf16", c["B"], c["L"] // {128: 1, 192: 2, 256: 4}[co], *shape, ch, knobs)
                assert got is not None and got[0] == a, (c["id"], v, got)
            else:
                dm, bm = a[:2]
                got = BW.enc_plan("bf16", dm, c["B"], c["L"] // {192: 2, 256: 4, 384: 8}[dm], BW.enc_bm_min(c, dm), BW.enc_knobs(c, dm))
                assert got == bm, (c["id"], v, got)
                if kind == "bc" and a[2]:
                    assert modes[dm, bm] >> (a[2] - 1) & 1, (c["id"], v, "has_chain() does not give this mode")
            n += 1
    assert n > 150


def _cb(prec, B, n, cin, cout, up_cin=0, chain=False, **kw):
    knobs = list(DEFAULT)
    for k, v in kw.items():
        knobs[("wgs", "bm", "occ", "pp", "asym", "tight", "rt").index(k)] = v
    got = BW.conv_plan(prec, B, n, cin, cout, up_cin, chain, knobs)
    return got and tuple(got[0])


def test_oddities_of_the_rule():
    # the bench shape (B = 64, L = 488): tall tiles at full resolution, BM - 4 rows for dec1, the asymmetric 32-row tiles at L / 4
    assert _cb("bf16", 64, 488, 128, 128) == (128, 128, 8, 1, 0, 0, 128, 0, 0)
    assert _cb("bf16", 64, 488, 192, 128, 128) == (128, 128, 8, 1, 192, 0, 192, 1, 0)
    assert _cb("bf16", 64, 122, 192, 256, chain=True) == (32, 256, 8, 1, 0, 1, 192, 2, 0)
    assert _cb("bf16", 64, 122, 384, 256, 256) == (32, 256, 8, 1, 384, 0, 384, 2, 0)
    # DHW_CONV_BM=32: the run-time-width <32,256,8> even for an encoder block; the 64-row variant for the fused-input dec3
    assert _cb("bf16", 2, 52, 192, 256, bm=32) == (32, 256, 8, 1, 0, 0, 0, 0, 0)
    assert _cb("bf16", 2, 52, 384, 256, 256, bm=32) == (64, 256, 8, 1, 384, 0, 384, 0, 0)
    # DHW_CONV_BM=64 only disables the tall and the 46- / 32-row choices (and not the tall dec1 with the fused input stage)
    assert _cb("bf16", 64, 488, 128, 128, bm=64) == (64, 128, 8, 1, 0, 0, 128, 0, 0)
    assert _cb("bf16", 64, 488, 192, 128, 128, bm=64) == (128, 128, 8, 1, 192, 0, 192, 1, 0)
    assert _cb("bf16", 64, 122, 192, 256, bm=64) == (64, 256, 8, 1, 0, 0, 192, 0, 0)
    # any DHW_CONV_BM or DHW_CONV_OCC forbids the ConvBlock -> EncoderLayer chain, whatever it says (-1: a value that reads as 0)
    assert _cb("bf16", 2, 244, 128, 192, chain=True) == (64, 192, 8, 1, 0, 1, 128, 0, 0)
    for kw in (dict(bm=64), dict(bm=48), dict(bm=-1), dict(occ=2), dict(occ=1), dict(occ=-1)):
        assert _cb("bf16", 2, 244, 128, 192, chain=True, **kw) is None and _cb("bf16", 64, 122, 192, 256, chain=True, **kw) is None, kw
    # fp32: one variant per width, no fused input stage, no chain
    assert _cb("fp32", 2, 122, 192, 256) == (32, 256, 4, 1, 0, 0, 0, 0, 0)
    assert _cb("fp32", 2, 122, 384, 256, 256) is None and _cb("fp32", 2, 122, 192, 256, chain=True) is None
    assert _cb("bf16", 2, 122, 192, 320) is None   # no such width
    # EncoderLayer: d = 384 on 64 rows halves to 32 (fits() is false); bm_min = 32 for enc5 under chain mode 2; 64 rows once they fill the CUs
    assert BW.enc_plan("bf16", 384, 2, 61, 0, [64, 256]) == 32 and BW.enc_plan("bf16", 256, 2, 122, 0, [64, 256]) == 64
    assert BW.enc_plan("bf16", 256, 2, 122, 0, [0, 256]) == 16 and BW.enc_plan("bf16", 256, 2, 122, 32, [0, 256]) == 32
    assert BW.enc_plan("bf16", 192, 64, 244, 0, [0, 256]) == 64 and BW.enc_plan("bf16", 192, 2, 244, 0, [16, 256]) == 32
    assert BW.enc_plan("fp32", 384, 64, 61, 0, [64, 256]) == 16
    lib, o12, o4 = _lib.lib(), (C.c_int * 12)(), (C.c_int * 4)()
    assert lib.dhw_debug_conv_plan(0, 0, 8, 128, 128, 0, 0, (C.c_int64 * 7)(*DEFAULT), o12) == -1
    assert lib.dhw_debug_conv_plan(0, 1, 8, 128, 128, 0, 0, None, o12) == -1 and lib.dhw_debug_enc_plan(0, 192, 1, 8, 0, None, o4) == -1
    assert lib.dhw_debug_tile_variants(2, 0, None) == -1 and lib.dhw_debug_tile_variants(0, -1, None) == lib.dhw_debug_tile_variants(0, 0, (C.c_int * 11)()) >= 32


CHILD = r"""
import ctypes as C, json, os, sys
from dhg_amd import _lib
sys.path.insert(0, sys.argv[1])
import blocks_worker as BW
lib, out = _lib.lib(), []
def knobs():
    k = (C.c_int64 * 12)()
    assert lib.dhw_debug_tile_knobs(k) == 0
    return list(k)
out.append(knobs())
before = BW.conv_plan("bf16", 64, 122, 192, 256, 0, False, [256, 0, 0, 0, 1, 1, 0])
os.environ.update(DHW_CONV_ASYM="1", DHW_CONV_TIGHT="1", DHW_CONV_RT="0", DHW_CONV_WGS="128", DHW_CONV_BM="48", DHW_CONV_OCC="0", DHW_CONV_PP="3",
                  DHW_CONV_STAGGER="5", DHW_ENC_BM="32", DHW_ENC_BM384="16", DHW_ENC_WGS="64")
out.append(knobs())
assert BW.conv_plan("bf16", 64, 122, 192, 256, 0, False, [256, 0, 0, 0, 1, 1, 0]) == before   # the plan entry reads no environment
for k in list(os.environ):
    if k.startswith(("DHW_CONV_", "DHW_ENC_")):
        del os.environ[k]
out.append(knobs())
print(json.dumps(out))
"""


def test_switches_are_read_per_call_or_frozen_once_per_process():
    """dhw_debug_tile_knobs in a process started with DHW_CONV_ASYM=0, DHW_CONV_TIGHT=0, DHW_CONV_RT=1: those three keep the value of
    the first read whatever the environment says later (one freeze for the uniform, ragged and store-policy launchers together);
    every other switch follows the environment from call to call.  And dhw_debug_conv_plan is a function of its arguments alone."""
    import json
    env = {k: v for k, v in os.environ.items() if not k.startswith(("DHW_CONV_", "DHW_ENC_"))}
    env.update(DHW_CONV_ASYM="0", DHW_CONV_TIGHT="0", DHW_CONV_RT="1", PYTHONPATH=os.pathsep.join([ROOT] + env.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "tests")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    first, second, third = json.loads(r.stdout.strip().splitlines()[-1])
    #                wgs  bm occ pp asym tight rt stagger enc: bm192 bm256 bm384 wgs
    assert first == [256, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 256]
    assert second == [128, 48, -1, 3, 0, 0, 1, 5, 32, 32, 16, 64]
    assert third == first
