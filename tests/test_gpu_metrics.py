"""sample_metrics end to end on the GPU (dhg_amd.sample_metrics next to sample_quality), with the synthetic model and the
random-initialised StyleExtractor of tests/test_gpu_quality.py at its shapes.

Features from random weights are around 1e-10 and the six lines of a set hardly differ: the numbers mean nothing as quality
figures.  The tests pin the path: one loop behind both entries (the same Fréchet distance bit for bit, sample_quality undisturbed),
reproducibility per seed, and that a given real set is used as it is."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import spec

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_quality import LT, L, T, pen_lines, state  # noqa: E402

pytestmark = pytest.mark.gpu

NUMBERS = ("fd", "precision", "recall", "density", "coverage", "kid")


@pytest.fixture(scope="module")
def extractor():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return dhg_amd.StyleExtractor()


@pytest.fixture(scope="module")
def model():
    m = dhg_amd.DiffusionModel(2, precision="bf16", max_B=8, max_L=L, max_Lt=LT).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in spec.synthetic_state_dict(2).items()}, strict=True)
    return m


@pytest.fixture(scope="module")
def data():
    inp = spec.synthetic_inputs(6, L, LT, seed=5)
    return {"strokes": pen_lines(6), "text": torch.from_numpy(inp["text"]), "style": torch.from_numpy(inp["style"])}


def metrics(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # 6 samples for 1280 dimensions
        return dhg_amd.sample_metrics(*a, **k)


def quality(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return dhg_amd.sample_quality(*a, **k)


def bits(s):
    return s.rows().tobytes()


def test_sample_metrics_is_finite_reproducible_and_shares_the_loop_of_sample_quality(model, extractor, data):
    fd0, real0, gen0 = quality(model, data, extractor, n=6, batch=4, seed=3, T=T)
    m = metrics(model, data, extractor, n=6, batch=4, seed=3, k=3, T=T)
    m2 = metrics(model, data, extractor, n=6, batch=4, seed=3, k=3, T=T)
    m3 = metrics(model, data, extractor, n=6, batch=4, seed=4, k=3, T=T)
    fd1, real1, gen1 = quality(model, data, extractor, n=6, batch=4, seed=3, T=T)
    assert all(np.isfinite(m[n]) for n in NUMBERS) and m["k"] == 3 and m["n"] == 6
    assert all(0 <= m[n] <= 1 for n in ("precision", "recall", "coverage")) and m["density"] >= 0
    assert m["real_set"].count == m["gen_set"].count == m["real_stats"].count == m["gen_stats"].count == 6
    assert all(m[n] == m2[n] for n in NUMBERS) and bits(m["gen_set"]) == bits(m2["gen_set"]) and bits(m["real_set"]) == bits(m2["real_set"])
    assert bits(m3["gen_set"]) != bits(m["gen_set"]) and bits(m3["real_set"]) == bits(m["real_set"])
    # the same Fréchet distance and statistics as sample_quality, which gives the same bits before and after
    assert m["fd"] == fd0 == fd1
    assert state(m["real_stats"]) == state(real0) == state(real1) and state(m["gen_stats"]) == state(gen0) == state(gen1)
    # the sets hold the pooled features of the rendered lines
    want = dhg_amd.FeatureSet(1280).update(dhg_amd.line_features(data["strokes"], extractor))
    assert bits(m["real_set"]) == bits(want)
    # the metrics are those of the sets
    pr = dhg_amd.precision_recall(m["real_set"], m["gen_set"], 3)
    assert all(pr[n] == m[n] for n in pr) and dhg_amd.kernel_distance(m["real_set"], m["gen_set"]) == m["kid"]


def test_a_given_real_set_is_used_as_given(model, extractor, data, tmp_path):
    m = metrics(model, data, extractor, batch=6, seed=3, k=2, T=T)
    m["real_set"].save(tmp_path / "real_set.npz")
    m["real_stats"].save(tmp_path / "real_stats.npz")
    given = (dhg_amd.FeatureStats.load(tmp_path / "real_stats.npz"), dhg_amd.FeatureSet.load(tmp_path / "real_set.npz"))
    blank = {**data, "strokes": torch.zeros(6, L, 3)}
    m2 = metrics(model, blank, extractor, batch=6, seed=3, k=2, T=T, real=given)
    assert m2["real_stats"] is given[0] and m2["real_set"] is given[1] and bits(given[1]) == bits(m["real_set"])
    assert all(m2[n] == m[n] for n in NUMBERS) and m2["k"] == 2
    # the set alone: its statistics are computed from its rows (in another order than batch by batch: the distance agrees closely)
    m3 = metrics(model, blank, extractor, batch=6, seed=3, k=2, T=T, real=dhg_amd.FeatureSet.load(tmp_path / "real_set.npz"))
    assert all(m3[n] == m[n] for n in NUMBERS[1:]) and m3["real_stats"].count == 6
    tr = float(np.trace(m["real_stats"].cov()) + np.trace(m["gen_stats"].cov()))
    assert abs(m3["fd"] - m["fd"]) <= 1e-5 * tr
    m4 = metrics(model, data, extractor, batch=6, seed=3, T=T, steps=4)
    assert all(np.isfinite(m4[n]) for n in NUMBERS) and m4["k"] == 3
