"""The launch sequence of one TrainModel forward + backward, recorded on the host against a stub library
(tools/train_launch_trace.py): the number of calls and the algorithmic GEMM FLOPs at the smallest shapes that reach every path —
channels (32, 48, 64): conv3's three-GEMM path and the FiLM as its own pass; (128, 192, 256): the merged path with the FiLM riding
on the GEMMs; sigma_ffn's 2048 -> 32 Linear splits K in both.  The expected values were recorded at the commit before
dhg_amd/train_model became a package; they count launches as Python issues them with the stub's return values, not GPU launches."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import train_launch_trace as tlt  # noqa: E402

WANT = {((32, 48, 64), "fp32", 0.0): (408, 88493568), ((32, 48, 64), "bf16", 0.1): (460, 88493568),
        ((128, 192, 256), "fp32", 0.0): (288, 1070118912), ((128, 192, 256), "fp32", 0.1): (334, 1070118912)}


def test_the_tool_records_the_configurations_pinned_here():
    assert set(tlt.CONFIGS) == set(WANT)


@pytest.mark.parametrize("channels,precision,drop", list(WANT))
def test_launch_count_and_gemm_flops_of_one_update(monkeypatch, channels, precision, drop):
    with monkeypatch.context() as m:
        lines, launches, flops = tlt.record(m.setattr, channels, precision, drop)
    print(f"{channels} {precision} drop {drop}: calls {len(lines)} last_launches {launches} last_gemm_flops {flops}")
    assert (len(lines), launches, flops) == (WANT[channels, precision, drop][0],) * 2 + (WANT[channels, precision, drop][1],)
    with monkeypatch.context() as m:       # a second run in the same process gives the same trace
        again, _, _ = tlt.record(m.setattr, channels, precision, drop)
    assert tlt.digest(again) == tlt.digest(lines)
