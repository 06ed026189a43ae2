"""Build libdhw_hip.so in-tree with hipcc for gfx950 (no JIT cache: the .so ships with the snapshot)."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libdhw_hip.so")
# (the slowest units first: the pool takes them in this order, and the longest compile bounds a clean build)
SOURCES = ["train/sgemm_f32.hip", "train/sgemm_bf16.hip", "train/sgemm_group.hip", "convblock.hip", "ragged/convblock_ragged.hip", "enclayer.hip",
           "ragged/enclayer_ragged.hip", "policy/convblock_policy.hip", "policy/enclayer_policy.hip", "gemm.hip", "ragged/gemm_ragged.hip", "ragged/attn_ragged.hip", "persist.hip", "attn.hip", "misc.hip", "style.hip", "textside.hip",
           "train.hip", "train/sgemm_launch.hip", "train/elementwise.hip", "train/film_table.hip", "train/batch.hip", "render/render.hip", "cond/cond.hip", "score/score.hip", "attnmap/attnmap.hip",
           "dhw_api.cpp", "dhw_style_api.cpp", "dhw_train_api.cpp", "plan/tile_knobs.cpp",
           "render/dhw_render_api.cpp", "cond/dhw_cond_api.cpp", "score/dhw_score_api.cpp", "attnmap/dhw_attnmap_api.cpp", "sampler/weights.cpp", "sampler/workspace.cpp", "sampler/denoiser.cpp", "sampler/sample.cpp", "sampler/debug.cpp",
           "step/step.hip", "step/dhw_step_api.cpp", "page/page.hip", "page/dhw_page_api.cpp", "encode/encode.hip", "encode/dhw_encode_api.cpp",
           "prep/prep.hip", "prep/dhw_prep_api.cpp", "train/cond_drop.hip", "moments/moments.hip", "moments/dhw_moments_api.cpp",
           "pairs/pairs.hip", "pairs/dhw_pairs_api.cpp", "dtw/dtw.hip", "dtw/dhw_dtw_api.cpp", "paths/paths.hip", "paths/dhw_paths_api.cpp",
           "truth/truth.hip", "truth/dhw_truth_api.cpp"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
# per-source additions.  dtw.hip: its loop is plain fp32 VALU; packed f32 instructions (v_pk_add_f32 / v_pk_mul_f32), which the SLP
# vectoriser makes of neighbouring features, issue slower there than the two scalar ones they replace
EXTRA_FLAGS = {"dtw/dtw.hip": ["-fno-slp-vectorize"]}


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _obj(objdir: str, s: str) -> str:
    return os.path.join(objdir, s.rsplit(".", 1)[0].replace("/", "_") + ".o")   # (named by path: unique across sub-directories)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    headers = [os.path.join(d, f) for d, _, files in os.walk(CSRC) for f in files if f.endswith(".h")]
    headers += [os.path.join(HERE, "..", "include", f) for f in ("dhw.h", "dhw_debug.h", "dhw_style.h", "dhw_train.h")]
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = _obj(objdir, s)
        # ragged/<f>_ragged.hip: <f>.hip compiled with per-sample lengths (csrc/dhw_kernels.h, DHW_LENS)
        # policy/<f>_policy.hip: <f>.hip compiled with the copy-outs' store policy read at run time (DHW_STORE_RT)
        base = [os.path.join(CSRC, os.path.basename(s).replace("_ragged", "").replace("_policy", ""))] if s.startswith(("ragged/", "policy/")) else []
        if force or _stale(obj, [src] + base + headers):
            cmd = [hipcc, *FLAGS, *EXTRA_FLAGS.get(s, []), "-x", "hip", "-c", src, "-o", obj]
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=8) as ex:
        for w in ex.map(run, jobs):
            if verbose and w:
                print(w)
    objs = [_obj(objdir, s) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
