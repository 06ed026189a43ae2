"""Training from a dataset resident on the GPU (include/dhw_train.h dhw_train_batch_draw / dhw_train_batch_gather;
train_model.ResidentData, group_tables, GraphedTrainStep(data=...), fit(resident=True), train.py --resident), what needs no GPU:
the numpy statement of the draw (tests/batch_ref.py) against Random123's known answers and against the properties the draw
must have, the group tables, the symbols, every argument rule of the two entries, make_batches(writers=...), the command line,
and the ValueErrors that are raised before a device is touched."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import dhg_amd
from dhg_amd import _lib, encode, train_model as tm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # a non-NULL, 16-byte aligned address: the argument checks never dereference it


def writers_1_2_3_31(seed=0):
    """Writer ids with groups of 1, 2, 3 and 31 samples (N = 37), shuffled."""
    w = np.array([5] * 1 + [9] * 2 + [2] * 3 + [7] * 31, np.int64)
    return w[np.random.default_rng(seed).permutation(len(w))]


# ---------------------------------------------------------------- the statement
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_statement_reproduces_the_random123_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in batch_ref.philox4x32_10(counter, key)) == want


def test_kernel_uses_the_shared_round_and_the_counter_layout_of_the_statement():
    src = open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "csrc", "train", "batch.hip")).read()
    assert "philox_round(c0, c1, c2, c3, k0, k1)" in src and "0x9E3779B9u" in src and "0xBB67AE85u" in src
    assert "c2 = 0u, c3 = 0u" in src and "2^32" in src            # the free lane of the generator; the bias is stated


def test_group_tables_list_every_group_and_every_position():
    w = writers_1_2_3_31()
    start, size, pos, members = (t.numpy() for t in tm.group_tables(w))
    assert all(t.dtype == np.int32 and t.shape == (37,) for t in (start, size, pos, members))
    assert sorted(members.tolist()) == list(range(37))
    for n in range(37):
        grp = members[start[n]:start[n] + size[n]].tolist()
        assert sorted(grp) == np.flatnonzero(w == w[n]).tolist(), n
        assert grp[pos[n]] == n
    assert sorted(set(size.tolist())) == [1, 2, 3, 31]
    assert [t.tolist() for t in tm.group_tables(torch.tensor([4]))] == [[0], [1], [0], [0]]
    for bad in (np.zeros((2, 2), np.int64), np.zeros(0, np.int64), np.zeros(3, np.float32)):
        with pytest.raises(ValueError, match="writers must be"):
            tm.group_tables(bad)


def test_statement_properties_over_400_draws():
    N, B, T = 37, 5, 60
    w = writers_1_2_3_31()
    tables = tuple(t.numpy() for t in tm.group_tables(w))
    abar = dhg_amd.get_alpha_set(T).numpy().astype(np.float32)
    assert len(abar) == T
    three = set(np.flatnonzero(w == 2).tolist())
    seen_src, seen_idx, seen_iv = set(), set(), set()
    for index in range(400):
        idx, src, alphas, sigma, iv = batch_ref.draw(11, index, N, B, abar, tables)
        assert ((0 <= idx) & (idx < N)).all() and ((0 <= iv) & (iv < T - 1)).all()
        lo, hi = np.minimum(abar[iv], abar[iv + 1]), np.maximum(abar[iv], abar[iv + 1])
        assert ((lo <= alphas) & (alphas <= hi)).all() and alphas.dtype == np.float32
        assert np.array_equal(sigma, np.sqrt(alphas))
        assert np.array_equal(w[src], w[idx])
        big = tables[1][idx] > 1
        assert (src[big] != idx[big]).all() and (src[~big] == idx[~big]).all()
        seen_src |= {int(s) for s, i in zip(src, idx) if int(i) in three}
        seen_idx |= set(idx.tolist())
        seen_iv |= set(iv.tolist())
        plain = batch_ref.draw(11, index, N, B, abar, None)
        assert np.array_equal(plain[0], idx) and np.array_equal(plain[1], idx) and np.array_equal(plain[2], alphas)
    assert seen_src == three and seen_idx == set(range(N)) and seen_iv == set(range(T - 1))
    assert not np.array_equal(batch_ref.draw(11, 0, N, B, abar)[0], batch_ref.draw(12, 0, N, B, abar)[0])     # the seed is the key
    assert batch_ref.draw(11, 1, 1, 3, abar, None)[0].tolist() == [0, 0, 0]


# ---------------------------------------------------------------- the C entries
def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dhw_train.h")).read()
    l = _lib.lib()
    for name in ("dhw_train_batch_draw", "dhw_train_batch_gather"):
        assert re.search(rf"\bint {name}\(", hdr) and name in _lib.SIGNATURES and hasattr(l, name)
    assert len(_lib.SIGNATURES["dhw_train_batch_draw"][1]) == 14 and len(_lib.SIGNATURES["dhw_train_batch_gather"][1]) == 16
    assert "train/batch.hip" in open(os.path.join(ROOT, "diffusion-handwriting-generation.pytorch_amd", "build.py")).read()


def _draw(**kw):
    a = dict(rng=FAKE, N=37, B=5, abar=FAKE, T=60, grp_start=None, grp_size=None, grp_pos=None, members=None, idx=FAKE, style_src=FAKE, alphas=FAKE, sigma=FAKE)
    a.update(kw)
    l = _lib.lib()
    rc = l.dhw_train_batch_draw(*a.values(), None)
    return rc, l.dhw_train_last_error().decode()


def _gather(**kw):
    a = dict(strokes=FAKE, text=FAKE, style=FAKE, idx=FAKE, style_src=FAKE, N=7, B=3, L=24, Lt=5, S=14, x=FAKE, pen=FAKE, ids=FAKE, mask=FAKE, style_out=FAKE)
    a.update(kw)
    l = _lib.lib()
    rc = l.dhw_train_batch_gather(*a.values(), None)
    return rc, l.dhw_train_last_error().decode()


BAD_DRAW = [(dict(N=0), "N = 0"), (dict(N=-1), "N = -1"), (dict(B=0), "B = 0"), (dict(T=1), "T = 1"), (dict(T=0), "T = 0")]
BAD_DRAW += [({k: None}, f"{k} is NULL") for k in ("rng", "abar", "idx", "style_src", "alphas", "sigma")]
BAD_DRAW += [({k: FAKE}, "all NULL or all set") for k in ("grp_start", "grp_size", "grp_pos", "members")]
BAD_DRAW += [(dict(grp_start=FAKE, grp_size=FAKE, grp_pos=FAKE), "all NULL or all set"), (dict(grp_size=FAKE, grp_pos=FAKE, members=FAKE), "all NULL or all set")]


@pytest.mark.parametrize("bad,msg", BAD_DRAW)
def test_each_argument_rule_of_batch_draw_answers_without_a_gpu(bad, msg):
    rc, err = _draw(**bad)
    assert rc == -1 and err.startswith("dhw_train_batch_draw:") and msg in err, (bad, rc, err)


BAD_GATHER = [(dict(N=0), "N = 0"), (dict(B=0), "B = 0"), (dict(L=0), "L = 0"), (dict(L=-8), "L = -8"), (dict(L=12), "L = 12"), (dict(L=20), "L = 20"),
              (dict(Lt=0), "Lt = 0"), (dict(S=0), "S = 0"), (dict(B=2 ** 31 - 1), "too large")]
BAD_GATHER += [({k: None}, f"{k} is NULL") for k in ("strokes", "text", "style", "idx", "style_src", "x", "pen", "ids", "mask", "style_out")]
BAD_GATHER += [({k: FAKE + 8}, f"{k} must be 16-byte aligned") for k in ("strokes", "style", "x", "pen", "style_out")]
BAD_GATHER += [({k: FAKE + 4}, f"{k} must be 8-byte aligned") for k in ("text", "ids")]


@pytest.mark.parametrize("bad,msg", BAD_GATHER)
def test_each_argument_rule_of_batch_gather_answers_without_a_gpu(bad, msg):
    rc, err = _gather(**bad)
    assert rc == -1 and err.startswith("dhw_train_batch_gather:") and msg in err, (bad, rc, err)


# ---------------------------------------------------------------- make_batches(writers=...)
def test_make_batches_writer_key_follows_kept(monkeypatch):
    def fake(lines, L=None, rounds=3, max_abs=15.0, device=None):
        return (torch.zeros(len(lines), L, 3), torch.full((len(lines),), 5, dtype=torch.int32), torch.tensor([0, 4, 0, 8, 0], dtype=torch.int32))
    monkeypatch.setattr(encode, "encode_strokes", fake)
    line = np.array([[0, 0, 0], [1, 1, 0], [2, 1, 1]], np.float32)
    texts = ["Hi there", "dropped by status", "x" * 12, "also dropped", "ok"]
    style = torch.zeros(5, 14, 1280)
    out = dhg_amd.make_batches([line] * 5, texts, style, max_seq_len=40, max_text_len=12, writers=[30, 31, 32, 33, 34])
    assert out["kept"] == [0, 4] and out["writer"].dtype == torch.int64 and out["writer"].tolist() == [30, 34]
    assert set(out) == {"strokes", "text", "style", "kept", "writer"}
    assert set(dhg_amd.make_batches([line] * 5, texts, style, max_seq_len=40, max_text_len=12)) == {"strokes", "text", "style", "kept"}
    for bad in ([1, 2, 3], [1.0] * 5, np.zeros((5, 1), np.int64)):
        with pytest.raises(ValueError, match="writers must hold 5 integer ids"):
            dhg_amd.make_batches([line] * 5, texts, style, max_seq_len=40, max_text_len=12, writers=bad)


# ---------------------------------------------------------------- train.py --resident, fit(resident=True)
def test_train_py_resident_reaches_fit(monkeypatch):
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    cli = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(cli)
    calls = []
    monkeypatch.setattr(tm, "fit", lambda *a, **k: calls.append((a, k)))
    cli.main(["--config", "c.yml", "--data", "d.pt", "--resident"])
    cli.main(["--config", "c.yml", "--data", "d.pt"])
    assert calls[0][0][:2] == ("c.yml", "d.pt") and calls[0][1]["resident"] is True and calls[1][1]["resident"] is False


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    for name in ("is_available", "current_device", "mem_get_info"):
        monkeypatch.setattr(torch.cuda, name, boom)
    monkeypatch.setattr(_lib, "lib", boom)


def test_fit_resident_without_data_raises(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="needs data_path"):
        tm.fit("missing.yml", None, resident=True)


def _data(N=6, L=16, Lt=4, S=2):
    return {"strokes": torch.zeros(N, L, 3), "text": torch.ones(N, Lt, dtype=torch.int64), "style": torch.zeros(N, S, 1280)}


BAD_DATA = [
    (lambda d: d.pop("style"), "must be a torch tensor"),
    (lambda d: d.update(strokes=d["strokes"].numpy()), "must be a torch tensor"),
    (lambda d: d.update(strokes=d["strokes"].double()), r"`strokes` must be float32 \[N, L, 3\]"),
    (lambda d: d.update(strokes=d["strokes"][:, :, :2]), r"`strokes` must be float32"),
    (lambda d: d.update(strokes=d["strokes"][:0]), "1 to 2\\^31 - 1 samples"),
    (lambda d: d.update(strokes=d["strokes"][:, :12]), "multiple of 8"),
    (lambda d: d.update(text=d["text"].int()), r"`text` must be int64 \[6, Lt\]"),
    (lambda d: d.update(text=d["text"][:5]), r"`text` must be int64 \[6, Lt\]"),
    (lambda d: d.update(style=d["style"][:, :, :640]), r"`style` must be float32 \[6, S, 1280\]"),
    (lambda d: d.update(style=d["style"].half()), r"`style` must be float32"),
    (lambda d: d.update(text=d["text"] * 73), "token id out of the embedding's range"),
    (lambda d: d.update(text=d["text"] * -1), "token id out of the embedding's range"),
    (lambda d: d.update(writer=torch.zeros(5, dtype=torch.int64)), r"writers must be an integer array \[6\]"),
    (lambda d: d.update(writer=torch.zeros(6)), r"writers must be an integer array \[6\]"),
]


@pytest.mark.parametrize("k", range(len(BAD_DATA)))
def test_resident_data_refuses_wrong_shapes_and_dtypes_before_any_device_access(monkeypatch, k):
    _no_device(monkeypatch)
    change, msg = BAD_DATA[k]
    d = _data()
    change(d)
    with pytest.raises(ValueError, match=msg):
        tm.ResidentData(d)


def test_resident_data_valid_arguments_get_as_far_as_the_device(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(AssertionError, match="device was touched"):
        tm.ResidentData(_data(), writers=np.arange(6) // 2)


def test_resident_data_names_both_numbers_when_it_does_not_fit(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1000, 2000))
    d = _data()
    need = 6 * 16 * 3 * 4 + 6 * 4 * 8 + 6 * 2 * 1280 * 4
    with pytest.raises(ValueError, match=rf"needs {need} bytes on cuda:0, which has 1000 bytes free"):
        tm.ResidentData(d)


def test_graphed_step_refuses_the_combinations_that_make_no_sense_with_resident_data():
    rd = types.SimpleNamespace(L=16, Lt=4, S=2, N=6, max_token=1)
    abar = torch.linspace(0.9, 0.1, 5)
    with pytest.raises(ValueError, match="device_rng=True"):
        tm.GraphedTrainStep(None, None, 2, 16, 4, 2, device_rng=False, data=rd, alpha_set=abar)
    for shape in ((24, 4, 2), (16, 5, 2), (16, 4, 14)):
        with pytest.raises(ValueError, match=r"holds strokes \[N, 16, 3\], text \[N, 4\], style \[N, 2, 1280\]"):
            tm.GraphedTrainStep(None, None, 2, *shape, data=rd, alpha_set=abar)
    with pytest.raises(ValueError, match="needs alpha_set"):
        tm.GraphedTrainStep(None, None, 2, 16, 4, 2, data=rd)
    with pytest.raises(ValueError, match="alpha_set at construction belongs to a step on resident data"):
        tm.GraphedTrainStep(None, None, 2, 16, 4, 2, alpha_set=abar)
    step = tm.GraphedTrainStep.__new__(tm.GraphedTrainStep)          # (the call's own checks come before it reads anything else)
    step.data = rd
    for kw in (dict(batch={}), dict(alphas=torch.zeros(2, 1)), dict(eps=torch.zeros(2, 16, 2)), dict(style_keep=torch.zeros(2, 2, 1280)), dict(alpha_set=abar)):
        with pytest.raises(ValueError, match=f"call step\\(step=n\\) without {next(iter(kw))}"):
            step(step=1, **kw)
    with pytest.raises(ValueError, match="step .* is required"):
        step()
    step.data = None
    with pytest.raises(ValueError, match="draws no batch"):
        step.last_draw()
