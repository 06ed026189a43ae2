#!/usr/bin/env python3
"""Writer-image preparation benchmark: B = 1024 seeded synthetic line images of about 300 x 2000 (white page, light specks, dark
pen loops inside margins of their own), H = 96, W = 1400, through one dhw_prep call on device-resident images, next to the
host arithmetic of read_img (remove_whitespace, then the numpy fp64 _resize_cubic) for the first --host-images of them.

  gpu_ms           median of --reps timed calls (at least 20) after 3 warm-up calls, each under device events: the three
                   launches alone, images already on the device (the wrapper's packing and host-to-device copy are not in it)
  floor_ms         the bytes the work must move (every image's h w bytes in, B H W 4 bytes out) over the MI355X's 8.0 TB/s HBM
                   peak; floor_fraction = floor_ms / gpu_ms, gpu_gbytes_per_s = those bytes over gpu_ms
  wrapper_ms       dhg_amd.prepare_images on the host arrays (packing, copy, call), host clock around a device synchronise
  cpu_ms_per_image read_img's arithmetic in a process pool of --workers over --host-images images, host clock, best of 2,
                   divided by the images; cpu_ms_all = that times B
  agree            on those images: crop box and width equal, grey levels at most 1 apart from the float resize (the derived
                   bound, tests/test_prep_cpu.py) and equal to the int64 statement of the rules (tests/prep_ref.py)

    python tools/bench_prep.py [--reps 20] [--workers 16] [--host-images 64] [--out profiles/prep.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, H, W, THRESH, SEED = 1024, 96, 1400, 127, 2026
HBM_PEAK = 8.0e12


def line_image(seed):
    import numpy as np
    g = np.random.Generator(np.random.PCG64(seed))
    h, w = int(g.integers(280, 321)), int(g.integers(1900, 2101))
    img = np.full((h, w), 255, np.uint8)
    n = h * w // 50
    img[g.integers(0, h, n), g.integers(0, w, n)] = g.integers(140, 250, n)      # specks, never dark
    top, bottom, left, right = (int(v) for v in g.integers(10, 60, 4))
    t = np.linspace(0, 1, 8 * w)
    x = left + t * (w - left - right - 1)
    y = top + (h - top - bottom - 1) * (0.5 + 0.5 * np.sin(t * g.uniform(150, 250)) * np.cos(t * g.uniform(5, 30)))
    pen = np.sin(t * g.uniform(300, 500)) > -0.7
    r, c = np.rint(y[pen]).astype(int), np.rint(x[pen]).astype(int)
    for dr in (0, 1, 2):                                                          # a pen three pixels wide
        img[np.minimum(r + dr, h - bottom - 1), c] = g.integers(0, 120, len(r))
    img[top, left] = img[h - bottom - 1, w - right - 1] = 0
    return img


def _cpu_chunk(images):
    sys.path.insert(0, ROOT)
    from dhg_amd.inference import _resize_cubic, remove_whitespace
    out = []
    for img in images:
        crop = remove_whitespace(img, THRESH)
        out.append(_resize_cubic(crop, H * crop.shape[1] // crop.shape[0], H))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--host-images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep.json"))
    a = ap.parse_args(argv)
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if not 1 <= a.host_images <= B:
        ap.error(f"--host-images must be in [1, {B}]")
    sys.path.insert(0, ROOT)
    import ctypes as C
    from concurrent.futures import ProcessPoolExecutor

    import numpy as np
    import prep_ref
    import torch

    import dhg_amd
    from dhg_amd import _lib

    images = [line_image(SEED + b) for b in range(B)]

    # the host's cores first: the pool forks before this process has touched the GPU
    sub = images[:a.host_images]
    chunks = [sub[i::a.workers] for i in range(a.workers)]
    cpu = []
    with ProcessPoolExecutor(a.workers) as ex:
        for _ in range(2):
            t0 = time.perf_counter()
            parts = list(ex.map(_cpu_chunk, chunks))
            cpu.append((time.perf_counter() - t0) * 1e3)
    host = [None] * len(sub)
    for i, p in enumerate(parts):
        host[i::a.workers] = p

    Hin, Win = max(im.shape[0] for im in images), -(-max(im.shape[1] for im in images) // 16) * 16
    packed = np.full((B, Hin, Win), 255, np.uint8)
    for b, im in enumerate(images):
        packed[b, :im.shape[0], :im.shape[1]] = im
    src = torch.from_numpy(packed).cuda()
    sizes = torch.tensor([im.shape for im in images], dtype=torch.int32).cuda()
    out = torch.empty((B, 1, H, W), device="cuda")
    widths, status = (torch.empty((B,), device="cuda", dtype=torch.int32) for _ in range(2))
    boxes = torch.empty((B, 4), device="cuda", dtype=torch.int32)
    lib = _lib.lib()
    need = int(lib.dhw_prep_workspace_bytes(B))
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.dhw_prep(src.data_ptr(), sizes.data_ptr(), B, Hin, Win, H, W, THRESH, out.data_ptr(), widths.data_ptr(), boxes.data_ptr(),
                                status.data_ptr(), ws.data_ptr(), need, stream))

    for _ in range(3):
        call()
    dhg_amd.prepare_images(images, H, W, THRESH)
    torch.cuda.synchronize()
    gpu, wrap = [], []
    for i in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        gpu.append(e0.elapsed_time(e1))
        if i < 3:                                      # (the wrapper moves 700 MB from the host: three calls tell its time)
            t0 = time.perf_counter()
            dhg_amd.prepare_images(images, H, W, THRESH)
            torch.cuda.synchronize()
            wrap.append((time.perf_counter() - t0) * 1e3)

    got, gw, gb, gs = out[:len(sub), 0].cpu().numpy(), widths.cpu().numpy(), boxes.cpu().numpy(), status.cpu().numpy()
    worst, exact = 0, True
    for b, (im, want) in enumerate(zip(sub, host)):
        ref, ow, box, st = prep_ref.prep_ref(im, H, W, THRESH)
        exact = exact and st == gs[b] and ow == gw[b] and box.tolist() == gb[b].tolist() and np.array_equal(ref, got[b])
        exact = exact and want.shape[1] == ow
        worst = max(worst, int(np.abs(got[b][:, :ow].astype(np.int64) - want.astype(np.int64)).max()))
    moved = sum(im.size for im in images) + B * H * W * 4
    gm = float(np.median(gpu))
    floor_ms = moved / HBM_PEAK * 1e3
    per_image = min(cpu) / len(sub)
    res = {"B": B, "H": H, "W": W, "Hin": Hin, "Win": Win, "reps": a.reps, "gpu_ms": round(gm, 4), "gpu_ms_min": round(min(gpu), 4),
           "gpu_ms_max": round(max(gpu), 4), "gpu_images_per_s": round(B / (gm * 1e-3)), "bytes_moved": moved, "floor_ms": round(floor_ms, 4),
           "floor_fraction": round(floor_ms / gm, 3), "gpu_gbytes_per_s": round(moved / (gm * 1e-3) / 1e9, 1),
           "wrapper_ms": round(float(np.median(wrap)), 1), "cpu_workers": a.workers, "cpu_images": len(sub),
           "cpu_ms_per_image": round(per_image, 3), "cpu_ms_all": round(per_image * B, 1), "status_nonzero": int((gs != 0).sum()),
           "mean_width": round(float(gw.mean()), 1), "max_grey_diff_to_float_resize": worst, "agree": bool(exact and worst <= 1),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
