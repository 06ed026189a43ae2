"""tests/style_ref.py checked without a GPU: the float64 launch references chained over an image reproduce the PyTorch restatement of the
network (oracle/mobilenet_ref.forward), the bf16 rounding helper is torch's conversion, the input generators put every ReLU6 launch
on both of its clip points at every shape of style_ref's tables, and a wrong variant of each kind of launch exceeds the bound."""
import os
import sys

import pytest
import torch

from oracle import mobilenet_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import style_ref as R  # noqa: E402


def _gen_image_plain(B, H, W, seed):
    return torch.randint(0, 256, (B, 1, H, W), generator=torch.Generator().manual_seed(seed)).float()


def test_launch_table_shape():
    t = R.launch_table()
    assert len(t) == 53 and [e["kind"] for e in t].count(R.POINTWISE) == 34 and [e["kind"] for e in t].count(R.DEPTHWISE) == 17
    assert t[0]["kind"] == R.STEM and t[-1]["kind"] == R.POOL and t[-2]["key"] == "features.18.0"
    assert sum(e["res"] for e in t) == 10
    # the widths only this component asks of the generic GEMM
    assert {320, 576, 960, 1280} <= {e["cout_p"] for e in t if e["kind"] == R.POINTWISE}
    assert max(e["cin_p"] for e in t if e["kind"] == R.POINTWISE) == 960
    keys = dict(mobilenet_ref.key_shapes())
    for e in t[:-1]:
        assert e["key"] + ".weight" in keys and e["bn"] + ".running_var" in keys, e


def test_chained_launch_references_match_the_restatement():
    """[2,1,96,97] through the 53 float64 launch references with weights folded in float64 == mobilenet_ref.forward (float32) to
    1e-4 max|ref|, feature map and pooled output: the criterion of tests/test_gpu_style.py for the fp32 feature map."""
    sd = mobilenet_ref.synthetic_state_dict(0)
    img = _gen_image_plain(2, 96, 97, seed=97)
    ref_out, ref_feat = mobilenet_ref.forward(sd, img.numpy(), return_features=True)
    x, block_in, feat = img, None, None
    for e in R.launch_table():
        w, b = (None, None) if e["kind"] == R.POOL else R.fold64(sd, e)
        if e["kind"] == R.POINTWISE and e["relu6"] and e["key"] != "features.18.0":
            block_in = x                                  # an expansion reads the block's input
        elif e["kind"] == R.DEPTHWISE and e["key"].endswith("conv.0.0"):
            block_in = x                                  # t = 1: the block opens with its depthwise convolution
        if e["kind"] == R.POOL:
            feat = x
        x = R.run(e, x, w, b, res=block_in)[0]
    assert feat.shape == (2, 3, 4, 1280) and x.shape == (2, 14, 1280)
    f = ref_feat.permute(0, 2, 3, 1).double()
    assert float((feat - f).abs().max()) <= 1e-4 * float(f.abs().max())
    assert float((x - ref_out.double()).abs().max()) <= 1e-4 * float(ref_out.abs().max())


def test_round_bf16_is_torchs_conversion():
    u = 2.0 ** -7                                         # one bf16 ulp at 1 (8 significant bits)
    fixed = torch.tensor([0.0, -0.0, 1.0, -1.0, 1.0 + u / 2, 1.0 + 3 * u / 2, 1.0 + u / 2 + 2.0 ** -20, 1.0 + u / 2 - 2.0 ** -20,   # ties: down to even, up to even
                          -(1.0 + u / 2), -(1.0 + 3 * u / 2), 6.0, 6.0 - 2.0 ** -22, 6.0 - 2.0 ** -7, 6.0 - 2.0 ** -6, 5.98828125, 5.9921875,
                          2.0 ** -126, 2.0 ** -100, 3.0e38, 0.1, 127.5, 255.0, 1.0 / 3.0, 2.0 ** 16 + 2.0 ** 8], dtype=torch.float32)
    rnd = torch.randn(4096, generator=torch.Generator().manual_seed(8)) * torch.logspace(-20, 20, 4096, base=2.0)
    for x in (fixed, rnd, torch.rand(4096, generator=torch.Generator().manual_seed(9)) * 6.0):
        got, want = R.round_bf16(x), x.to(torch.bfloat16).to(torch.float32)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert R.round_bf16(torch.tensor([1.0 + u / 2]))[0] == 1.0 and R.round_bf16(torch.tensor([1.0 + 3 * u / 2]))[0] == 1.0 + 2 * u
    assert R.round_bf16(torch.tensor([6.0 - 2.0 ** -22]))[0] == 6.0 and R.round_bf16(torch.tensor([-0.0])).view(torch.int32)[0] == -2 ** 31


def test_pool_bins_are_the_adaptive_pools():
    for Wp in (1, 13, 14, 15, 33, 44):
        cols = R.pool_cols(Wp)
        assert len(cols) == 14 and min(cols) >= 1
        x = torch.zeros(1, 1, 1, Wp, dtype=torch.float64)
        for k in range(Wp):                               # how many bins column k is part of == how often it is counted
            x.zero_()
            x[..., k] = 1.0
            y = torch.nn.functional.adaptive_avg_pool2d(x, (1, 14)).reshape(14)
            assert torch.allclose(y[y > 0], 1.0 / torch.tensor(cols, dtype=torch.float64)[y > 0])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_generators_reach_both_clip_points(bf16):
    """Every ReLU6 launch, at every shape of style_ref's tables, has >= 1 % of its float64 reference outputs at 0
    and >= 1 % at 6; at 70 rows (pointwise) / [2,C,5,7] (depthwise) >= 2 % at 6 and >= 46 % at 0.  The stem reaches 6 only with its
    BatchNorm gamma scaled: STEM_GAMMA_SCALE is the smallest power of two that does it."""
    sd, t = R.scaled_state_dict(0), R.launch_table()
    for i, e in enumerate(t):
        if not e["relu6"]:
            continue
        w, b = R.fold64(sd, e)
        w = R.kernel_weights(e, w.float(), bf16)
        shapes = {R.STEM: R.STEM_SHAPES, R.DEPTHWISE: R.DW_SHAPES, R.POINTWISE: tuple((R.PW_B, h, ww) for h, ww in R.PW_HW)}[e["kind"]]
        for s in shapes:
            f0, f6 = R.clip_fractions(R.run(e, R.gen_input(i, e, *s, bf16), w, b)[0])
            assert f0 >= 0.01 and f6 >= 0.01, (e["name"], s, f0, f6)
            if s in ((R.PW_B, 7, 10), (2, 5, 7)) and e["kind"] != R.STEM:
                assert f0 >= 0.46 and f6 >= 0.02, (e["name"], s, f0, f6)
    if not bf16:
        plain, half = mobilenet_ref.synthetic_state_dict(0), R.scaled_state_dict(0)
        half["features.0.1.weight"] = half["features.0.1.weight"] / 2
        for s in R.STEM_SHAPES:
            img = R.gen_image(*s)
            assert img.min() == 0 and img.max() == 255 and {0.0, 255.0} <= set(img[0, 0, 0].tolist()) | set(img[0, 0, -1].tolist())
            assert R.clip_fractions(R.stem(img, *R.fold64(plain, t[0]))[0])[1] == 0.0
        assert min(R.clip_fractions(R.stem(R.gen_image(*s), *R.fold64(half, t[0]))[0])[1] for s in R.STEM_SHAPES) < 0.01
    # the generated values are bf16 values in bf16 mode
    x = R.gen_input(5, t[5], 2, 5, 7, True)
    assert torch.equal(x, x.to(torch.bfloat16).float())


# ---- the bound can fail: one wrong variant per kind of launch, applied to the float64 reference ---------------------------------------
def _over(var, ref, bnd):
    """(largest |var - ref| / bound, fraction of the elements above the bound); an element the variant leaves undefined counts as above"""
    r = ((var - ref).abs() / bnd).nan_to_num(nan=float("inf"))
    return float(r.max()), float((r > 1.0).double().mean())


def _fp32_case(sd, t, i, shape):
    e = t[i]
    w, b = R.fold64(sd, e)
    w, b = w.float().double(), b.float().double()
    x = R.gen_input(i, e, *shape, False)
    ref, S, K = R.run(e, x, w, b, R.gen_residual(i, e, *shape, False))
    return e, x, w, b, ref, R.bound(ref, S, K)


def test_a_depthwise_tap_shifted_by_one_exceeds_the_bound():
    """the centre tap reads its right neighbour (the two weights swapped): every depthwise launch, every shape"""
    sd, t = R.scaled_state_dict(0), R.launch_table()
    for i in [i for i, e in enumerate(t) if e["kind"] == R.DEPTHWISE]:
        for shape in R.DW_SHAPES:
            e, x, w, b, ref, bnd = _fp32_case(sd, t, i, shape)
            wv = w.clone()
            wv[:, [4, 5]] = w[:, [5, 4]]
            worst, frac = _over(R.run(e, x, wv, b)[0], ref, bnd)
            assert worst > 1e3 and frac > 0.25, (e["name"], shape, worst, frac)


def test_relu6_dropped_from_a_pointwise_launch_exceeds_the_bound():
    """every expansion and features.18 at every row count: all the elements the reference clips"""
    sd, t = R.scaled_state_dict(0), R.launch_table()
    for i in [i for i, e in enumerate(t) if e["kind"] == R.POINTWISE and e["relu6"]]:
        for h, w_ in R.PW_HW:
            e, x, w, b, ref, bnd = _fp32_case(sd, t, i, (R.PW_B, h, w_))
            worst, frac = _over(R.pointwise(x, w, b, None, False)[0], ref, bnd)
            assert worst > 1e3 and frac > 0.25, (e["name"], (h, w_), worst, frac)


def test_a_wrong_stem_padding_value_exceeds_the_bound():
    """zero padding of the RAW image (grey level 0 = -1 after normalisation) instead of the normalised one: every border output"""
    sd, t = R.scaled_state_dict(0), R.launch_table()
    for shape in R.STEM_SHAPES:
        e, img, w, b, ref, bnd = _fp32_case(sd, t, 0, shape)
        xp = torch.nn.functional.pad(img.double() / 127.5 - 1.0, (1, 1, 1, 1), value=-1.0)
        var = torch.nn.functional.conv2d(xp, w.reshape(32, 1, 3, 3), b, stride=2).clamp(0.0, 6.0).permute(0, 2, 3, 1)
        worst, _ = _over(var, ref, bnd)
        inner = _over(var[:, 1:-1, 1:-1], ref[:, 1:-1, 1:-1], bnd[:, 1:-1, 1:-1])[0] if min(ref.shape[1:3]) > 2 else 0.0
        assert worst > 1e3 and inner <= 1.0, (shape, worst, inner)


def test_the_pools_ceil_replaced_by_floor_exceeds_the_bound():
    """bin j = pooled columns [floor(j Wp / 14), floor((j + 1) Wp / 14)): empty bins at Wp < 14, wrong bins wherever 14 does not divide
    Wp; (1,4,44), one pooled column per bin, is the one shape of the table that cannot tell"""
    t = R.launch_table()
    for shape in R.POOL_SHAPES:
        x = R.gen_input(52, t[52], *shape, False).double()
        ref, S, K = R.pool(x)
        p = torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 3)
        Wp, var = p.shape[-1], torch.full_like(ref, float("nan"))
        for j in range(R.BINS):
            w0, w1 = j * Wp // R.BINS, (j + 1) * Wp // R.BINS
            if w1 > w0:
                var[:, j] = p[:, :, :, w0:w1].mean(dim=(2, 3))
        worst, frac = _over(var, ref, R.bound(ref, S, K))
        if Wp % R.BINS == 0:
            assert worst <= 1.0, shape
        else:
            assert worst > 1e3 and frac > 0.05, (shape, worst, frac)
