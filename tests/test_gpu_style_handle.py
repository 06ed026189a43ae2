"""One StyleExtractor handle across image sizes (include/dhw_style.h): the scratch buffers of a handle grow with the largest image it
has seen (csrc/dhw_style_api.cpp ensure_buffers) and every later forward runs over whatever the earlier ones left in them.  No other
test uses one handle at two sizes."""
import numpy as np
import pytest
import torch

import dhg_amd
from oracle import mobilenet_ref

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _img(B, H, W):
    return np.random.Generator(np.random.PCG64(1000 * H + W)).integers(0, 256, size=(B, 1, H, W)).astype(np.float32)


@pytest.fixture(scope="module")
def sd():
    return mobilenet_ref.synthetic_state_dict(0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_one_handle_across_image_sizes(sd, prec):
    """forward (1,96,96), then (2,128,333) — the scratch regrows — then (1,96,96) again over the larger scratch's stale contents:
    the first and third results are bit-identical, the second is bit-identical to a fresh handle's (pooled output and feature map)."""
    ex = dhg_amd.StyleExtractor(sd, precision=prec)
    small, big = _img(1, 96, 96), _img(2, 128, 333)
    a = ex(small).cpu()
    fa = ex.debug_features()
    b = ex(big).cpu()
    fb = ex.debug_features()
    c = ex(small).cpu()
    fc = ex.debug_features()
    fresh = dhg_amd.StyleExtractor(sd, precision=prec)
    b2 = fresh(big).cpu()
    fb2 = fresh.debug_features()
    assert a.shape == (1, 14, 1280) and b.shape == (2, 14, 1280) and fa.shape == (1, 3, 3, 1280) and fb.shape == (2, 4, 11, 1280)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
    assert torch.equal(_bits(a), _bits(c)) and torch.equal(_bits(fa), _bits(fc)), "a forward depends on what an earlier, larger one left in the scratch"
    assert torch.equal(_bits(b), _bits(b2)) and torch.equal(_bits(fb), _bits(fb2)), "a forward after the scratch regrew differs from a fresh handle's"
