"""The host half of the text-plane reuse decision (csrc/sampler/plane_tag.h), through dhw_debug_plane_tag: needs no
GPU.  A call may reuse the resident plane only when the tag of the plane is valid and equal to the call's in every field, the
schedule fits one chunk of the plane, and the handle's gates are all open."""
import ctypes as C

import pytest

from dhg_amd import _lib

FIELDS = ("valid", "B", "nstreams", "Lt", "S", "T", "t_start", "weights_gen", "film", "plane_gen")
BASE = dict(valid=1, B=64, nstreams=1, Lt=30, S=14, T=60, t_start=60, weights_gen=3, film=0x7F0012345000, plane_gen=2)
ALL_GATES = 7


def host_ok(resident, call, gates=ALL_GATES):
    arr = lambda d: (C.c_int64 * 10)(*[d[f] for f in FIELDS])
    return _lib.lib().dhw_debug_plane_tag(arr(resident), arr(call), gates)


def test_equal_tags_reuse():
    assert host_ok(BASE, BASE) == 1
    assert host_ok(dict(BASE, T=64, t_start=64), dict(BASE, T=64, t_start=64)) == 1
    assert host_ok(dict(BASE, T=1, t_start=1), dict(BASE, T=1, t_start=1)) == 1


@pytest.mark.parametrize("field", FIELDS[1:])
def test_any_field_that_differs_forbids_reuse(field):
    # another batch, sub-batch split, prompt length, style rows, schedule, first iteration; reloaded weights (generation);
    # another schedule's FiLM table; a re-allocated plane (generation)
    assert host_ok(BASE, dict(BASE, **{field: BASE[field] + 1})) == 0
    assert host_ok(dict(BASE, **{field: BASE[field] - 1}), BASE) == 0


def test_a_cleared_tag_forbids_reuse():
    # what every invalidating event does (a dhw_set_* setter, dhw_load, dropped graphs, an error return): valid = 0
    assert host_ok(dict(BASE, valid=0), BASE) == 0
    assert host_ok(dict(BASE, valid=0), dict(BASE, valid=0)) == 0


def test_the_chunk_rule():
    # the plane holds at most 64 steps; a longer schedule runs in chunks that overwrite each other
    for T, want in ((64, 1), (65, 0), (66, 0), (1000, 0)):
        tag = dict(BASE, T=T, t_start=T)
        assert host_ok(tag, tag) == want, T
    tag = dict(BASE, T=100, t_start=10)     # (one chunk would do here; the rule is on T, the conservative side)
    assert host_ok(tag, tag) == 0


@pytest.mark.parametrize("gates", range(ALL_GATES))
def test_every_gate_must_be_open(gates):
    # bit 0: DHW_PLANE_REUSE, bit 1: the all-steps plane in use, bit 2: the fused bf16 text-side kernels serve the call
    assert host_ok(BASE, BASE, gates) == 0


def test_null_arguments_are_an_error():
    assert _lib.lib().dhw_debug_plane_tag(None, None, ALL_GATES) == -1
