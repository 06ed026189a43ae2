"""Host side of the stroke rasteriser (include/dhw.h dhw_render, dhg_amd.render_strokes) that needs no GPU: the symbols
are exported and bound, the workspace size is sane, every argument rule answers DHW_ERR_ARG with the argument's name
before any HIP call, and the Python surface fails loudly without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, vis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


def test_render_symbols_are_exported_and_bound():
    l = _lib.lib()
    for name in ("dhw_render_workspace_bytes", "dhw_render"):
        assert name in _lib.SIGNATURES and hasattr(l, name)
    assert l.dhw_render.restype is C.c_int and l.dhw_render_workspace_bytes.restype is C.c_size_t
    assert callable(dhg_amd.render_strokes) and dhg_amd.render_strokes is vis.render_strokes
    assert callable(vis.save_line_png)


def test_workspace_bytes_positive_and_monotone():
    f = _lib.lib().dhw_render_workspace_bytes
    prev_row = None
    for B in (1, 2, 3, 64, 65, 1000):
        row = [f(B, L) for L in (1, 8, 40, 488, 1000, 4096)]
        assert all(v > 0 for v in row)
        assert all(a < b for a, b in zip(row, row[1:])), (B, row)               # strictly growing in L
        assert prev_row is None or all(a <= b for a, b in zip(prev_row, row))   # never shrinking in B
        assert row[-1] >= B * 4096 * 16                                         # one float4 per stroke at least
        prev_row = row
    assert f(64, 488) > f(1, 488)
    assert f(0, 8) == 0 and f(1, 0) == 0 and f(1, 4097) == 0                    # outside dhw_render's ranges


def _call(**kw):
    a = dict(strokes=FAKE, lens=None, B=2, L=40, H=32, W=128, line_width=2.0, img_out=FAKE, widths_out=None, workspace=FAKE,
             workspace_bytes=None)
    a.update(kw)
    l = _lib.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = max(l.dhw_render_workspace_bytes(max(a["B"], 1), min(max(a["L"], 1), 4096)), 16)
    rc = l.dhw_render(a["strokes"], a["lens"], a["B"], a["L"], a["H"], a["W"], a["line_width"], a["img_out"], a["widths_out"],
                      a["workspace"], a["workspace_bytes"], None)
    return rc, l.dhw_last_error(None).decode()


@pytest.mark.parametrize("bad,name", [
    (dict(B=0), "B"), (dict(B=-3), "B"),
    (dict(L=0), "L"), (dict(L=4097), "L"),
    (dict(H=7), "H"),
    (dict(W=4), "W"), (dict(W=130), "W"), (dict(W=7), "W"),
    (dict(line_width=0.25), "line_width"), (dict(line_width=16.5), "line_width"), (dict(line_width=float("nan")), "line_width"),
    (dict(line_width=6.0, H=8), "line_width"),           # 2m = 8 is not < H
    (dict(line_width=10.0, H=32, W=12), "line_width"),   # 2m = 12 is not < W
    (dict(strokes=None), "strokes"),
    (dict(img_out=None), "img_out"),
    (dict(workspace=None), "workspace"),
    (dict(workspace_bytes=15), "workspace_bytes"),
])
def test_each_argument_rule_is_checked_without_a_gpu(bad, name):
    rc, msg = _call(**bad)
    assert rc == -1, (bad, rc, msg)
    assert re.search(rf"\b{name}\b", msg) and msg.startswith("dhw_render"), (bad, msg)


def test_workspace_one_byte_short_is_rejected():
    need = _lib.lib().dhw_render_workspace_bytes(2, 40)
    rc, msg = _call(workspace_bytes=need - 1)
    assert rc == -1 and "workspace_bytes" in msg


def test_kernel_constants_match_the_kernel_header():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "render", "render.h")).read()
    assert int(re.search(r"constexpr int RENDER_CHUNK = (\d+);", src).group(1)) == vis.RENDER_CHUNK
    assert int(re.search(r"constexpr int RENDER_TILE_W = (\d+);", src).group(1)) == vis.RENDER_TILE_W


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_render_strokes_fails_loudly_without_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU path"):
        dhg_amd.render_strokes(np.zeros((1, 8, 3), np.float32))


def test_render_strokes_rejects_a_bad_shape_before_touching_the_device():
    for bad in (np.zeros((8, 3), np.float32), np.zeros((2, 8, 2), np.float32), torch.zeros(1, 2, 8, 3)):
        with pytest.raises(ValueError, match="strokes"):
            dhg_amd.render_strokes(bad)
    assert vis.render_strokes.__defaults__ == (None, 96, 1400, 2.0)


def test_renderer_option_is_validated(tmp_path):
    import infer
    with pytest.raises(SystemExit):
        infer.main(["hello", "style.npy", "--experiment-path", str(tmp_path), "--renderer", "bogus"])
    for f in (dhg_amd.infer_file, dhg_amd.infer_file_batch):
        with pytest.raises(ValueError, match="renderer"):
            f("hi" if f is dhg_amd.infer_file else ["hi"], "style.npy", experiment_path=str(tmp_path), renderer="bogus")


def test_save_line_png_crops_and_rounds(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    img = np.full((1, 8, 12), 255.0, np.float32)
    img[0, 3, :5] = [0.4, 0.5, 1.5, 2.5, 254.6]
    vis.save_line_png(img, 5, "line")
    got = np.asarray(Image.open(tmp_path / "line.png"))
    assert got.shape == (8, 5) and got.dtype == np.uint8
    assert got[3].tolist() == [0, 0, 2, 2, 255] and (np.delete(got, 3, axis=0) == 255).all()
    vis.save_line_png(torch.from_numpy(img), 0, "empty")       # a row without ink keeps one white column
    assert np.asarray(Image.open(tmp_path / "empty.png")).shape == (8, 1)
