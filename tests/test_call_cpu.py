"""_call.py on the host: the workspace cache, the argument rules with the message texts the wrappers had before
the module existed, the no-GPU refusal and its hook, and the argument order of DeviceCall.run."""
import ctypes as C

import numpy as np
import pytest
import torch

from dhg_amd import _call, _lib

CPU = torch.device("cpu")


@pytest.fixture
def fresh_cache(monkeypatch):
    monkeypatch.setattr(_call, "_workspaces", {})


def test_workspace_starts_at_64k_doubles_and_keeps_outgrown_buffers(fresh_cache):
    a = _call.workspace("render", CPU, 1)
    assert a.dtype == torch.uint8 and a.numel() == 1 << 16 and a.device == CPU
    assert _call.workspace("render", CPU, 1 << 16) is a          # still fits: the same object
    b = _call.workspace("render", CPU, (1 << 16) + 1)
    assert b is not a and b.numel() == 1 << 17
    c = _call.workspace("render", CPU, 5 * (1 << 16))            # not a power of two: the first one at or above it
    assert c.numel() == 1 << 19
    assert _call.workspace("render", CPU, 1 << 19) is c and _call.workspace("render", CPU, 7) is c
    kept = _call._workspaces[("render", None)]
    assert [t.numel() for t in kept] == [1 << 16, 1 << 17, 1 << 19] and kept[0] is a and kept[1] is b   # outgrown, still referenced
    assert _call.newest_workspace("render", None) is c


def test_workspace_families_do_not_share_and_none_is_fresh(fresh_cache):
    bufs = {f: _call.workspace(f, CPU, 100) for f in ("render", "page", "paths", "dtw", "moments", "pairs")}
    assert len({id(t) for t in bufs.values()}) == 6
    assert all(_call.workspace(f, CPU, 100) is t for f, t in bufs.items())
    x, y = _call.workspace(None, CPU, 100), _call.workspace(None, CPU, 100)
    assert x is not y and x.numel() == y.numel() == 100 and x.data_ptr() != y.data_ptr()
    assert set(_call._workspaces) == {(f, None) for f in bufs}   # (a fresh buffer is not cached)
    assert _call.workspace("render", CPU, 0) is None and _call.workspace(None, CPU, 0) is None


@pytest.mark.parametrize("v,hi,msg", [
    (True, None, "n = True is not an integer"), (8.0, None, "n = 8.0 is not an integer"), ("8", 9, "n = '8' is not an integer"),
    (2, None, "n = 2 must be >= 3"), (2, 9, "n = 2 must lie in [3, 9]"), (10, 9, "n = 10 must lie in [3, 9]"),
    (np.int64(1), None, "n = 1 must be >= 3"), (2 ** 31, 2 ** 31 - 1, f"n = {2 ** 31} must lie in [3, {2 ** 31 - 1}]")])
def test_check_int_refusals(v, hi, msg):
    with pytest.raises(ValueError) as e:
        _call.check_int("n", v, 3, hi)
    assert str(e.value) == msg


def test_check_int_and_number_accept():
    for v, hi in ((3, None), (np.int64(3), None), (np.int32(9), 9), (2 ** 31, None)):
        r = _call.check_int("n", v, 3, hi)
        assert type(r) is int and r == v
    for v in (2, 2.5, np.int64(3), np.float32(0.1), np.float64(-1e30)):
        r = _call.check_number("x", v)
        assert type(r) is float and r == float(np.float32(v))    # (rounded to what the library takes)
    assert _call.check_number("x", 0.1, finite=False) == 0.1 and _call.check_number("x", float("inf"), finite=False) == float("inf")
    assert _call.is_int(np.int64(3)) and not _call.is_int(True) and not _call.is_int(8.0)
    assert _call.is_number(8.0) and _call.is_number(np.float32(1)) and not _call.is_number(False) and not _call.is_number("1")


@pytest.mark.parametrize("v,msg", [
    (True, "x = True is not a number"), ("1", "x = '1' is not a number"), (None, "x = None is not a number"),
    (float("nan"), "x = nan must be finite"), (float("inf"), "x = inf must be finite"), (-np.inf, "x = -inf must be finite"),
    (1e39, "x = inf must be finite")])   # (1e39 is finite as a double and infinite as the float32 the library takes: refused)
@pytest.mark.filterwarnings("ignore:overflow encountered in cast")
def test_check_number_refusals(v, msg):
    with pytest.raises(ValueError) as e:
        _call.check_number("x", v)
    assert str(e.value) == msg
    if msg.endswith("not a number"):
        with pytest.raises(ValueError, match="is not a number"):
            _call.check_number("x", v, finite=False)


@pytest.mark.parametrize("v,msg", [
    ([1, 2], "lengths must hold 3 entries, got 2"), ([1, True, 3], "lengths[1] = True is not an integer"),
    ([1, 2, 8.0], "lengths[2] = 8.0 is not an integer"), (np.array([1.0, 2.0, 3.0]), "lengths[0] = 1.0 is not an integer"),
    ([2 ** 31, 2, 3], f"lengths[0] = {2 ** 31} does not fit int32"), ([1, -2 ** 31 - 1, 3], f"lengths[1] = {-2 ** 31 - 1} does not fit int32")])
def test_host_ints_refusals(v, msg):
    with pytest.raises(ValueError) as e:
        _call.host_ints("lengths", v, 3)
    assert str(e.value) == msg


def test_host_ints_accepts_lists_arrays_and_cpu_tensors():
    for v in ([1, np.int64(3), -2 ** 31], np.array([1, 3, -2 ** 31]), torch.tensor([1, 3, -2 ** 31]), (1, 3, -2 ** 31)):
        r = _call.host_ints("slots", v, 3)
        assert r == [1, 3, -2 ** 31] and all(type(x) is int for x in r)
    assert _call.host_ints("slots", [2 ** 31 - 1], 1) == [2 ** 31 - 1]
    assert not _call.on_device(torch.tensor([1])) and not _call.on_device([1])


def test_open_refuses_a_machine_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for who in ("render_page", "FeatureStats.update", "dynamic time warping"):
        with pytest.raises(RuntimeError) as e:
            with _call.open(who, like=torch.zeros(1)):
                raise AssertionError("the block ran")
        assert str(e.value) == f"{who} needs an MI355X (HIP device): there is no CPU path in this package"
    with pytest.raises(RuntimeError, match="no CPU path"):
        _call.pick_device("FeatureSet", device="cuda:0")


def test_open_looks_torch_up_at_call_time(monkeypatch):
    """The hook of the wrappers' CPU tests: a replaced torch.cuda.is_available / current_device / _lib.lib is what gets called."""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    with pytest.raises(AssertionError, match="a device was touched"):
        with _call.open("render_page"):
            pass
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    with pytest.raises(AssertionError, match="a device was touched"):
        _call.pick_device("render_page", like=torch.zeros(1))
    assert _call.pick_device("render_page", device="cuda:1") == torch.device("cuda", 1)   # (an index given: nothing is asked)


@pytest.mark.parametrize("device", ["cpu", torch.device("cpu"), "meta"])
def test_a_device_that_is_not_cuda_is_refused_before_anything_is_opened(monkeypatch, device):
    """What torch.cuda.device said for encode_strokes / prepare_images before this module, now said for every caller, and
    before a stream is asked for or a byte allocated: a host pointer must never reach a kernel."""
    def boom(*a, **k):
        raise AssertionError("something was opened for a device that is not a CUDA device")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for name in ("current_device", "current_stream", "device"):
        monkeypatch.setattr(torch.cuda, name, boom)
    monkeypatch.setattr(_lib, "lib", boom)
    for f in (_call.pick_device, _call.open):
        with pytest.raises(ValueError) as e:
            f("encode_strokes", like=torch.zeros(1), device=device)
        assert str(e.value) == f"Expected a cuda device, but got: {torch.device(device)}"


class _Stream:
    cuda_stream = 0x1230


class _Guard:
    """Stands in for torch.cuda.device(index)."""
    log = []

    def __init__(self, index):
        self.index = index

    def __enter__(self):
        _Guard.log.append(("enter", self.index))

    def __exit__(self, *exc):
        _Guard.log.append(("exit", self.index, exc[0]))
        return False


def _host_call(monkeypatch, dev=CPU, handle=None, record=False, opened=False):
    """A DeviceCall built by its own __init__ (or by ``open``) on a machine without a GPU: torch.cuda's stream and device
    guard are stand-ins."""
    _Guard.log = []
    asked = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda index: asked.append(index) or _Stream())
    monkeypatch.setattr(torch.cuda, "device", _Guard)
    c = _call.open("who", device=dev, record=record) if opened else _call.DeviceCall(dev, handle, record)
    assert asked == [dev.index] and isinstance(c.stream, _Stream) and c.dev == dev and c.h is handle
    return c


def _stub_call(monkeypatch, handle, code=0):
    seen = []

    class Lib:
        def dhw_entry(self, *args):
            seen.append(args)
            return code

        def dhw_last_error(self, h):
            seen.append(("last_error", h))
            return b"the stub failed"

    lib = Lib()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    return _host_call(monkeypatch, handle=handle), seen


def test_run_puts_the_handle_first_and_the_stream_last(monkeypatch):
    h = C.c_void_p(0xABC0)
    c, seen = _stub_call(monkeypatch, h)
    c.run("dhw_entry", 1, None, 2.5)
    assert len(seen) == 1 and seen[0][0] is h and seen[0][1:4] == (1, None, 2.5)
    assert isinstance(seen[0][4], C.c_void_p) and seen[0][4].value == 0x1230 and len(seen[0]) == 5
    c, seen = _stub_call(monkeypatch, None)
    c.run("dhw_entry", 1, None, 2.5)
    assert seen[0][:3] == (1, None, 2.5) and seen[0][3].value == 0x1230 and len(seen[0]) == 4
    c.run("dhw_entry")
    assert len(seen[1]) == 1 and seen[1][0].value == 0x1230
    assert c.ptr(None) is None and c.ptr(torch.zeros(1)) != 0 and c.lens(None) is None and list(c.lens([8, 16])) == [8, 16]


@pytest.mark.parametrize("handle", [None, C.c_void_p(0xABC0)])
def test_run_turns_a_negative_return_into_dhw_error(monkeypatch, handle):
    c, seen = _stub_call(monkeypatch, handle, code=-3)
    with pytest.raises(_lib.DhwError) as e:
        c.run("dhw_entry", 7)
    assert e.value.code == -3 and "the stub failed" in str(e.value)
    assert seen[-1] == ("last_error", handle)
    c, seen = _stub_call(monkeypatch, handle, code=2)   # (a non-negative code is no error)
    c.run("dhw_entry", 7)


class _Input:
    """Stands in for a tensor the caller hands in."""

    def __init__(self):
        self.recorded = []

    def to(self, dev, dtype):
        return self

    def contiguous(self):
        return self

    def record_stream(self, stream):
        self.recorded.append(stream)


@pytest.mark.parametrize("record", [False, True])
def test_open_is_on_the_device_for_the_block_and_records_inputs_only_when_asked_and_only_on_a_clean_exit(monkeypatch, record):
    dev = torch.device("cuda", 1)
    x = _Input()
    with _host_call(monkeypatch, dev, record=record, opened=True) as c:
        assert _Guard.log == [("enter", 1)] and c.h is None
        assert c.to(x) is x and x.recorded == []                   # (not before the work is enqueued)
    assert _Guard.log == [("enter", 1), ("exit", 1, None)]
    assert x.recorded == ([c.stream] if record else [])
    y = _Input()
    with pytest.raises(KeyError):
        with _host_call(monkeypatch, dev, record=record, opened=True) as c:
            c.to(y)
            raise KeyError("the block failed")
    assert _Guard.log == [("enter", 1), ("exit", 1, KeyError)] and y.recorded == []   # (left the device; nothing was enqueued for y)


def test_device_call_keeps_what_it_hands_out(monkeypatch, fresh_cache):
    c = _host_call(monkeypatch)
    x = torch.arange(6).reshape(2, 3).t()
    y = c.to(x)
    assert y.dtype == torch.float32 and y.is_contiguous() and c.inputs == [y] and c.to(None) is None
    assert c.to(x, torch.int32).dtype == torch.int32
    lens = _call.stage_ints(c, [3, 1], object())
    assert lens.dtype == torch.int32 and lens.tolist() == [3, 1] and _call.stage_ints(c, None, None) is None
    given = torch.tensor([4, 5])
    assert _call.stage_ints(c, None, given).tolist() == [4, 5] and len(c.inputs) == 4
    e = c.empty((2, 2), torch.int32)
    assert e.shape == (2, 2) and e.dtype == torch.int32 and c.outputs == [e] and c.empty((1,), wanted=False) is None
    assert c.empty(3).dtype == torch.float32
