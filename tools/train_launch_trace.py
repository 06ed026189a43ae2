#!/usr/bin/env python3
"""Record every library call of one TrainModel forward + backward on the host, without a GPU and without the library.

Every device action of the update goes through ``_lib.lib().dhw_op_*``; a stub library that only writes the calls down gives the
launch sequence as Python issues it: (name, scalar arguments, every dhw_gemm_desc field), each pointer rewritten as (buffer
ordinal by first appearance, byte offset inside its storage).  Two commits whose traces are equal line for line hand the GPU the
same launches with the same arguments over the same aliasing pattern.  Prints, per configuration, the number of calls,
``last_launches``, ``last_gemm_flops`` and the sha256 of the trace; ``--dump DIR`` writes the traces as text for a diff.
The counts are launches with the stub's return values (1 per paired / grouped GEMM call), not GPU launch counts.
"""
import argparse
import bisect
import ctypes as C
import hashlib
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, L, LT, S, LAYERS = 2, 16, 5, 14, 2       # the smallest shapes that still reach every path
CONFIGS = [((32, 48, 64), "fp32", 0.0), ((32, 48, 64), "bf16", 0.1),         # 48 % 32 != 0: conv3's three-GEMM path, FiLM as its own pass
           ((128, 192, 256), "fp32", 0.0), ((128, 192, 256), "fp32", 0.1)]   # the merged path with the FiLM riding on the GEMMs


def record(patch, channels, precision="fp32", drop_rate=0.0):
    """One forward + backward under ``patch(obj, name, value)`` (pytest's ``monkeypatch.setattr``, or any setter the caller
    undoes) -> (trace lines, last_launches, last_gemm_flops)."""
    from dhg_amd import _lib, spec, train_model as tm
    bases, stores, order, lines = [], {}, {}, []
    real_ptr = torch.Tensor.data_ptr

    def data_ptr(t):        # register the storage and keep it alive: no address is handed out twice during the run
        st = t.untyped_storage()
        if st.nbytes() and st.data_ptr() not in stores:
            bisect.insort(bases, st.data_ptr())
            stores[st.data_ptr()] = st
        return real_ptr(t)

    def ptr(p):
        p = p.value if isinstance(p, C.c_void_p) else p
        if not p:
            return "null"
        i = bisect.bisect_right(bases, p) - 1
        if i < 0 or p >= bases[i] + stores[bases[i]].nbytes():
            raise RuntimeError(f"pointer {p:#x} lies in no registered storage")
        return f"b{order.setdefault(bases[i], len(order))}+{p - bases[i]}"

    def desc(d):
        return "{" + " ".join(f"{n}={ptr(getattr(d, n)) if ty is C.c_void_p else getattr(d, n)!r}" for n, ty in _lib.GemmDesc._fields_) + "}"

    def show(a, ty):
        if isinstance(a, C.Array):
            return "[" + " ".join(desc(d) for d in a) + "]"
        if hasattr(a, "_obj"):       # C.byref(descriptor)
            return desc(a._obj)
        return ptr(a) if ty is C.c_void_p else repr(a)

    class Recorder:
        def __getattr__(self, name):
            types_ = _lib.SIGNATURES[name][1]

            def call(*args):
                lines.append(f"{name}(" + ", ".join(show(a, ty) for a, ty in zip(args[:-1], types_)) + ")")   # (the last argument is the stream)
                return 1 if name in ("dhw_op_gemm2", "dhw_op_gemm_group") else 0
            return call

    rec = Recorder()
    patch(torch.cuda, "is_available", lambda: True)
    patch(torch.cuda, "current_device", lambda: 0)
    patch(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    patch(_lib, "lib", lambda: rec)
    patch(torch.Tensor, "data_ptr", data_ptr)
    model = tm.TrainModel(spec.synthetic_state_dict(LAYERS, *channels, seed=0), num_layers=LAYERS, device="cpu", drop_rate=drop_rate, precision=precision)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, spec.VOCAB, (B, LT), generator=g)
    score, pen = model.forward_device(torch.randn(B, L, 2, generator=g), ids, torch.zeros(B, LT), torch.rand(B, 1, generator=g),
                                      torch.randn(B, S, 1280, generator=g), torch.ones(B, S, 1280))
    model.backward(torch.ones_like(score), torch.ones_like(pen))
    return lines, model.last_launches, model.last_gemm_flops


def digest(lines) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dump", metavar="DIR", help="write each configuration's trace to DIR/<channels>_<precision>_<drop>.txt")
    a = ap.parse_args()
    for channels, precision, drop in CONFIGS:
        undo = []

        def patch(obj, name, value):
            undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)
        try:
            lines, launches, flops = record(patch, channels, precision, drop)
        finally:
            for obj, name, old in reversed(undo):
                setattr(obj, name, old)
        tag = f"{'-'.join(map(str, channels))}_{precision}_{drop}"
        print(f"{tag}: calls {len(lines)} last_launches {launches} last_gemm_flops {flops} sha256 {digest(lines)}")
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, tag + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
