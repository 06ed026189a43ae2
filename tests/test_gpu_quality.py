"""The sample-quality metric end to end on the GPU (dhg_amd.line_features, sample_quality, FeatureStats, frechet_distance).

No trained weights exist where this was written: the StyleExtractor is random-initialised and the model holds
``spec.synthetic_state_dict(2)``.  The distances mean nothing as quality figures; the tests pin the plumbing (batching, seeds,
which sampler runs, that nothing of ``sample`` is disturbed) and that the distance reacts to a change of the lines.

Sensitivity, the cases and why: with fewer lines than feature dimensions the covariance is rank-deficient and the distance of a
set to itself is about 1e-7 tr already (square roots of clipped eigenvalues; tests/test_quality_cpu.py), a hundred times the
1e-9 tr asked of a mere reordering.  So the order test runs on a full-rank statistic: 64 lines, and the 48 feature channels of
the largest variance over them.  The changed lines have dy doubled, not dx and dy: dhw_render scales every line to fill its
image (include/dhw.h, rule 7), so a uniform scaling of a line draws the same picture and cannot move any feature."""
import warnings

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import inference, spec

pytestmark = pytest.mark.gpu

L, LT, T = 72, 8, 9


def pen_lines(n, seed=11):
    """n synthetic lines [n,L,3]: rightward strokes on a wavy baseline, a lift every 9 to 15 rows and on the last row."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n, L, 3), np.float32)
    for b in range(n):
        t = np.arange(L) * g.uniform(0.4, 1.1)
        out[b, :, 0] = g.uniform(0.2, 1.2, L)
        out[b, :, 1] = g.uniform(0.5, 1.5) * np.cos(t + g.uniform(0, 6)) + g.normal(0, 0.3, L)
        i = 0
        while i < L:
            i += int(g.integers(9, 16))
            out[b, min(i, L) - 1, 2] = 1
    return torch.from_numpy(out)


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


def state(st):
    return st.count, st._state()[0].tobytes(), st._state()[1].tobytes()


def stats_in_batches(features, batch):
    """The statistics sample_quality accumulates: one update per batch (the last bits of a sum depend on where the calls split)."""
    st = dhg_amd.FeatureStats(1280)
    for lo in range(0, features.shape[0], batch):
        st.update(features[lo:lo + batch])
    return st


def test_line_features_equal_one_unbatched_pass(extractor):
    lines = pen_lines(6)
    want = extractor(dhg_amd.render_strokes(lines)[0])
    got = dhg_amd.line_features(lines, extractor, batch=4)          # one full batch and a partial one
    assert got.is_cuda and tuple(got.shape) == (6, 14, 1280) and torch.equal(got, want)
    lens = [72, 64, 40, 72, 56, 48]
    want = extractor(dhg_amd.render_strokes(lines, lens)[0])
    assert torch.equal(dhg_amd.line_features(lines, extractor, lengths=lens, batch=4), want)
    assert not torch.equal(want, got)
    with pytest.raises(ValueError, match="lengths"):
        dhg_amd.line_features(lines, extractor, lengths=lens[:5])


def test_sample_quality_is_finite_and_reproducible(model, extractor, data):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                             # 6 samples for 1280 dimensions
        fd, real, gen = dhg_amd.sample_quality(model, data, extractor, n=6, batch=4, seed=3, T=T)
        fd2, real2, gen2 = dhg_amd.sample_quality(model, data, extractor, n=6, batch=4, seed=3, T=T)
        fd3, _, gen3 = dhg_amd.sample_quality(model, data, extractor, n=6, batch=4, seed=4, T=T)
    assert np.isfinite(fd) and real.count == gen.count == 6
    assert fd == fd2 and state(real) == state(real2) and state(gen) == state(gen2)
    assert state(gen3) != state(gen)
    assert state(real) == state(stats_in_batches(dhg_amd.line_features(data["strokes"], extractor), 4))


def test_given_real_statistics_are_used_as_they_are(model, extractor, data, tmp_path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fd, real, gen = dhg_amd.sample_quality(model, data, extractor, batch=6, seed=3, T=T)
        real.save(tmp_path / "real.npz")
        given = dhg_amd.FeatureStats.load(tmp_path / "real.npz")
        fd2, real2, gen2 = dhg_amd.sample_quality(model, {**data, "strokes": torch.zeros(6, L, 3)}, extractor, batch=6, seed=3, T=T, real=given)
    assert real2 is given and state(given) == state(real) and state(gen2) == state(gen) and fd2 == fd


def test_steps_select_the_ddim_sampler(model, extractor, data, monkeypatch):
    calls = {"sample": 0, "sample_ddim": 0}
    seen = []

    def counting(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            seen.append((k.get("first_sample"), k.get("L"), a[1].shape[0]))
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(inference, "sample", counting("sample", inference.sample))
    monkeypatch.setattr(inference, "sample_ddim", counting("sample_ddim", inference.sample_ddim))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fd, _, gen = dhg_amd.sample_quality(model, data, extractor, batch=4, T=T, steps=4)
        assert calls == {"sample": 0, "sample_ddim": 2} and seen == [(0, L, 4), (4, L, 2)]
        fd1, _, gen1 = dhg_amd.sample_quality(model, data, extractor, batch=4, T=T, guidance=1.5, diffusion_mode="standard")
        assert calls == {"sample": 2, "sample_ddim": 2}
    assert np.isfinite(fd) and np.isfinite(fd1) and gen.count == gen1.count == 6
    want = inference.sample_ddim(model, data["text"].cuda(), data["style"].cuda(), L=L, T=T, steps=4)
    assert state(gen) == state(stats_in_batches(dhg_amd.line_features(want, extractor), 4))


def test_sample_is_left_alone(model, extractor, data):
    text, style = data["text"].cuda(), data["style"].cuda()
    before = dhg_amd.sample(model, text, style, L=L, T=T, seed=7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dhg_amd.sample_quality(model, data, extractor, batch=4, T=T, steps=3)
        dhg_amd.sample_quality(model, data, extractor, batch=4, T=T)
    after = dhg_amd.sample(model, text, style, L=L, T=T, seed=7)
    assert torch.equal(before, after)


def test_distance_ignores_the_order_and_sees_a_change_of_the_lines(extractor):
    """Printed: the two distances and their ratio.  Asserted: |FD(order)| <= 1e-9 tr; FD(changed lines) > 0 and at least 1e3 times
    max(|FD(order)|, 1e-9 tr).  Measured on an MI355X with the random-initialised extractor (features around 1e-10, tr 3.5e-19):
    FD(order) = -1.3e-31 (3.6e-13 tr), FD(dy doubled) = 6.1e-19, ratio 1.7e9; dx and dy doubled: bit-identical features."""
    lines = pen_lines(64, seed=12)
    tall = lines.clone()
    tall[:, :, 1] *= 2
    f = dhg_amd.line_features(lines, extractor).mean(1)
    g = dhg_amd.line_features(tall, extractor).mean(1)
    top = torch.argsort(f.var(0), descending=True)[:48]
    f, g = f[:, top].contiguous(), g[:, top].contiguous()
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).permutation(64)).cuda()
    a, b, c = (dhg_amd.FeatureStats(48).update(x) for x in (f, f[perm].contiguous(), g))
    tr = float(np.trace(a.cov()))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                              # 64 samples for 48 dimensions: no rank warning
        fd_order, fd_change = dhg_amd.frechet_distance(a, b), dhg_amd.frechet_distance(a, c)
    ratio = fd_change / max(abs(fd_order), 1e-9 * tr)
    same = dhg_amd.line_features(lines * torch.tensor([2.0, 2.0, 1.0]), extractor).mean(1)[:, top]
    print(f"tr {tr:.4g}: FD(order) {fd_order:.3e} ({abs(fd_order) / tr:.1e} tr), FD(dy doubled) {fd_change:.3e}, ratio {ratio:.3e}; "
          f"dx and dy doubled: features bit-identical = {torch.equal(same, f)}")
    assert abs(fd_order) <= 1e-9 * tr
    assert fd_change > 0 and ratio >= 1e3
