"""The Python side of one library call: the device, the stream, the workspace and the argument rules that every
wrapper of an include/dhw.h entry shares.  ``DeviceCall`` serves the handle entries (``DiffusionModel._device_call``) and, through
``open``, the entries that take the caller's workspace and stream instead of a handle.

Temporaries: every tensor a wrapper makes for a call (a staged input, an output, a ``family=None`` workspace) is allocated inside
the ``with`` block, on ``current_stream(dev)``, the stream the call is enqueued on, so the caching allocator can hand its memory
out again only behind that work.  ``record_stream`` matters only for a tensor the caller allocated elsewhere (on another stream)
and handed in as it is: ``record=True`` marks the call's inputs for the wrappers that did so before this module existed; the
others (the graph-captured ``render_*`` / ``stroke_paths`` among them) stay without it."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

_workspaces = {}   # (family, device index) -> [uint8 workspace tensors, the newest (largest) last]


def workspace(family, dev, need: int):
    """``need`` bytes of workspace on ``dev`` (None for 0): one cached buffer per ``family`` and device, 64 KiB grown by
    doubling.  Outgrown buffers stay referenced (a captured graph may still point at one): at most one per doubling, together
    smaller than the newest.  ``family=None``: a fresh buffer of exactly ``need`` bytes."""
    if not need:
        return None
    if family is None:
        import torch

        return torch.empty(need, dtype=torch.uint8, device=dev)
    bufs = _workspaces.setdefault((family, dev.index), [])
    if not bufs or bufs[-1].numel() < need:
        import torch

        size = 1 << 16
        while size < need:
            size *= 2
        bufs.append(torch.empty(size, dtype=torch.uint8, device=dev))
    return bufs[-1]


def newest_workspace(family, index: int):
    """The buffer the last call of ``family`` on device ``index`` worked in (KeyError when there was none)."""
    return _workspaces[(family, index)][-1]


class DeviceCall:
    """The device side of one library call: the conversions every entry needs, and the tensors the call hands to the library,
    kept so that they outlive the stream's work.  ``handle``: the model's, for the denoiser entries, which build this inside
    their own device block (``DiffusionModel._device_call``); None for the others, which enter it as a context (``open``)."""

    def __init__(self, dev, handle=None, record: bool = False):
        import torch

        self.torch, self.lib = torch, _lib.lib()
        self.dev, self.h, self.record = dev, handle, record
        self.stream = torch.cuda.current_stream(dev.index)   # (the index here and in __enter__: torch need not parse a device)
        self.inputs, self.outputs = [], []

    def __enter__(self):
        self._guard = self.torch.cuda.device(self.dev.index)
        self._guard.__enter__()
        return self

    def __exit__(self, kind, value, trace):
        if self.record and kind is None:
            for x in self.inputs:
                x.record_stream(self.stream)
        return self._guard.__exit__(kind, value, trace)

    def to(self, x, dtype=None):
        """``x`` (or None) as a contiguous tensor of ``dtype`` (None: float32) on the call's device."""
        if x is not None:
            x = x.to(self.dev, self.torch.float32 if dtype is None else dtype).contiguous()
            self.inputs.append(x)
        return x

    def empty(self, shape, dtype=None, wanted: bool = True):
        if not wanted:
            return None
        out = self.torch.empty(shape, device=self.dev, dtype=self.torch.float32 if dtype is None else dtype)
        self.outputs.append(out)
        return out

    def workspace(self, family, entry: str, *dims):
        """(buffer or None, bytes) of what ``entry(*dims)`` (a ``dhw_*_workspace_bytes``) asks for; see ``workspace``."""
        need = int(getattr(self.lib, entry)(*dims))
        ws = workspace(family, self.dev, need)
        if family is None and ws is not None:
            self.inputs.append(ws)
        return ws, need

    @staticmethod
    def ptr(x):
        return x.data_ptr() if x is not None else None

    @staticmethod
    def lens(lens):
        return (C.c_int32 * len(lens))(*lens) if lens is not None else None

    def run(self, entry: str, *args):
        """``entry(handle, *args, stream)`` with a handle, ``entry(*args, stream)`` without: every entry of include/dhw.h that
        launches work ends with the stream, and the denoiser's open with the handle."""
        f, stream = getattr(self.lib, entry), C.c_void_p(self.stream.cuda_stream)
        _lib.check(f(*args, stream) if self.h is None else f(self.h, *args, stream), self.h)


def pick_device(who: str, like=None, device=None):
    """The device of a call: ``device`` when given, else ``like``'s when it is a CUDA tensor, else the current one; always with
    an index.  RuntimeError on a machine without a GPU, then ValueError for a ``device`` that is not a CUDA device (torch's own
    words for it): nothing is opened or allocated for one, so no host pointer can reach a kernel."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs an MI355X (HIP device): there is no CPU path in this package")
    dev = torch.device(device) if device is not None else like.device if like is not None and like.is_cuda else None
    if dev is not None and dev.type != "cuda":
        raise ValueError(f"Expected a cuda device, but got: {dev}")
    if dev is None or dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def open(who: str, like=None, device=None, record: bool = False) -> DeviceCall:
    """The context of a handle-free entry, ``with open(...) as c``: pick the device (``pick_device``, which refuses a machine
    without a GPU in ``who``'s name) and, in the block, be on it; ``record``: see the module text."""
    return DeviceCall(pick_device(who, like, device), record=record)


# ---------------------------------------------------------------- argument rules (host only, ValueError)
def is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))   # (bool is an int to Python, not to a caller)


def is_number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def check_int(name: str, v, lo: int, hi=None) -> int:
    if not is_int(v):
        raise ValueError(f"{name} = {v!r} is not an integer")
    if hi is None and v < lo:
        raise ValueError(f"{name} = {v} must be >= {lo}")
    if hi is not None and not lo <= v <= hi:
        raise ValueError(f"{name} = {v} must lie in [{lo}, {hi}]")
    return int(v)


def check_number(name: str, v, finite: bool = True) -> float:
    """``v`` as a float; ``finite``: rounded to float32 (what the library takes) and finite there."""
    if not is_number(v):
        raise ValueError(f"{name} = {v!r} is not a number")
    if not finite:
        return float(v)
    v = float(np.float32(v))
    if not math.isfinite(v):
        raise ValueError(f"{name} = {v} must be finite")
    return v


def host_ints(name: str, v, N: int):
    """A host list / array / CPU tensor of N integers -> list of int (ValueError otherwise)."""
    host = v.tolist() if hasattr(v, "tolist") else list(v)
    if len(host) != N:
        raise ValueError(f"{name} must hold {N} entries, got {len(host)}")
    for i, x in enumerate(host):
        if not is_int(x):
            raise ValueError(f"{name}[{i}] = {x!r} is not an integer")
        if not -2 ** 31 <= x < 2 ** 31:
            raise ValueError(f"{name}[{i}] = {x} does not fit int32")
    return [int(x) for x in host]


def on_device(v) -> bool:
    import torch

    return isinstance(v, torch.Tensor) and v.is_cuda


def stage_ints(c: DeviceCall, host, given):
    """An optional integer argument as an int32 tensor on the call's device: the checked ``host`` list when there is one, else
    ``given``, a device tensor, which stays on the device unread."""
    if given is None:
        return None
    x = c.torch.tensor(host, dtype=c.torch.int32).to(c.dev) if host is not None else given.to(c.dev, c.torch.int32).contiguous()
    c.inputs.append(x)
    return x
