"""Every dhw_op_* / dhw_train_* entry of the training step (include/dhw_train.h) called directly with raw pointers, in both kernel
forms, against the float64 references of tests/train_ops_ref.py.

Every device buffer comes from ONE helper (``alloc``): its size is taken from ``_shapes`` — the shapes the header gives, in one table —
its payload sits ``off`` floats (0 or 1) past a 16-byte boundary inside a larger allocation with 64 floats of canary on each side, outputs
that a call must fully write start as NaN and outputs it adds to start as random values.  After every call: every canary bit-identical,
no NaN left in a fully written output, elements the call does not address bit-identical.

Kernel form (csrc/train/elementwise.hip ``vec4_ok``): off = 0 with C % 4 == 0 and pstride % 4 == 0 reaches the 16-byte form, off = 1 on
one operand or C % 4 != 0 the scalar form; with DHW_TRAIN_VEC4=0 in the environment the launchers take the scalar forms everywhere and
the 16-byte cases skip.  Tolerance: exact where the operation is a copy or one correctly rounded fp32 operation; otherwise the
criterion of tests/test_gpu_train_model.py ``_close``: max |got - ref64| <= 2e-5 max |ref64| per tensor, inputs N(0,1).  The worst
error / bound per entry is printed at the end of the module."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

import dhg_amd  # noqa: F401
from dhg_amd import _lib, train

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 64
TOL = 2e-5
ERR_ARG = -1          # DHW_ERR_ARG (include/dhw.h)
WORST = {}            # entry -> worst observed error / bound
_INT64 = ("ids", "woff", "boff", "rng")
_CANARY_GEN = torch.Generator().manual_seed(20240229)


def _vec4_enabled():
    e = os.environ.get("DHW_TRAIN_VEC4")
    if e is None:
        return True
    m = re.match(r"\s*[+-]?\d+", e)          # atoi, as the launcher reads it
    return (int(m.group()) if m else 0) != 0


def _need_vec4():
    if not _vec4_enabled():
        pytest.skip("DHW_TRAIN_VEC4=0: the launchers take the scalar forms everywhere")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst error / bound per entry (bound = 2e-5 max|ref64|):")
    for k in sorted(WORST):
        print(f"  {k:28s} {WORST[k]:.3f}")


# ---- the one place that knows buffer sizes ----------------------------------------------------------------------------------------
def _shapes(entry, n=0, B=0, L=0, C=0, ps=0, rows=0, mode=0, rows_out=0, cols=0, R=0, V=0, total=0, nflat=0, n_keep=0):
    """name -> shape of every buffer of ``entry`` as include/dhw_train.h states them.  gtab / btab (dgtab / dbtab): the per-sample
    parameter tables [B][pstride] in which gamma and beta (their gradients) are columns."""
    act, tab, bl = (B, L, C), (B, ps), (B, L)
    rows_in = 2 * rows_out if mode in (0, 3) else rows_out // 2
    flat = (n,)
    return {
        "dhw_op_unary": dict(x=flat, y=flat),
        "dhw_op_unary_bwd": dict(dy=flat, x=flat, dx=flat),
        "dhw_op_add": dict(a=flat, b=flat, out=flat),
        "dhw_op_mask_mul": dict(x=flat, mask=flat, y=flat),
        "dhw_op_add_rows": dict(x=act, table=(L, C), out=act),
        "dhw_op_film": dict(x=act, gtab=tab, btab=tab, y=act),
        "dhw_op_film_bwd": dict(dy=act, x=act, gtab=tab, dx=act, dgtab=tab, dbtab=tab),
        "dhw_op_film_act": dict(x=act, gtab=tab, btab=tab, addend=act, y=act),
        "dhw_op_film_act_bwd": dict(dy=act, x=act, gtab=tab, btab=tab, dx=act, dgtab=tab, dbtab=tab),
        "dhw_op_ln_film": dict(x=act, gtab=tab, btab=tab, addend=act, y=act, act_out=act, pe=(L, C), pe_out=act, mean=bl, rstd=bl),
        "dhw_op_ln_film_bwd": dict(dy=act, x=act, mean=bl, rstd=bl, gtab=tab, dx=act, dgtab=tab, dbtab=tab),
        "dhw_op_layernorm": dict(x=(rows, C), y=(rows, C), mean=(rows,), rstd=(rows,)),
        "dhw_op_layernorm_bwd": dict(dy=(rows, C), y=(rows, C), rstd=(rows,), dx=(rows, C)),
        "dhw_op_softmax": dict(s=(B, R, cols), mask=(B, cols), p=(B, R, cols)),
        "dhw_op_softmax_bwd": dict(dp=(B, R, cols), p=(B, R, cols), ds=(B, R, cols)),
        "dhw_op_resample": dict(x=(rows_in, C), y=(rows_out, C)),
        "dhw_op_embedding": dict(ids=(rows,), table=(V, C), y=(rows, C)),
        "dhw_op_embedding_bwd": dict(ids=(rows,), dy=(rows, C), dtable=(V, C)),
        "dhw_op_colsum": dict(dy=(rows, C), db=(C,)),
        "dhw_op_film_table": dict(sigma=(B, 32), flat=(nflat,), woff=(total,), boff=(total,), film=(B, total)),
        "dhw_op_film_table_bwd": dict(dfilm=(B, total), sigma=(B, 32), flat=(nflat,), woff=(total,), boff=(total,), grad_flat=(nflat,), dsigma=(B, 32)),
        "dhw_op_keep_mask": dict(rng=(2,), keep=flat),
        "dhw_train_draw": dict(rng=(2,), eps=(B, L, 2), keep=(n_keep,)),
        "dhw_train_loss": dict(eps=(B, L, 2), score_pred=(B, L, 2), pen=bl, pen_pred=bl, alphas=(B,), out3=(3,), d_score=(B, L, 2), d_pen_pred=bl),
        "dhw_train_adam_dev": dict(p=flat, g=flat, hyper=(9,), sqnorm=(1,)),
    }[entry]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Buf:
    """One device buffer inside its canary margins.  ``val`` None: an output the call must fully write (NaN-filled)."""

    def __init__(self, shape, val, off, dtype):
        assert off in (0, 1)
        self.shape, self.n, self.lo = tuple(shape), int(np.prod(shape)), CANARY + off
        self.hi = self.lo + self.n
        total = self.hi + CANARY
        if dtype == torch.float32:
            host = torch.randn(total, generator=_CANARY_GEN)
        else:
            host = torch.randint(-2 ** 40, 2 ** 40, (total,), generator=_CANARY_GEN, dtype=torch.int64)
        self.must_write = val is None
        host[self.lo:self.hi] = float("nan") if val is None else val.reshape(-1).to(dtype)
        self.host, self.whole = host, host.to(DEV)
        assert self.whole.data_ptr() % 16 == 0
        self.ptr = self.whole.data_ptr() + self.lo * host.element_size()
        self.view = self.whole[self.lo:self.hi]                     # (for the entries that are reached through dhg_amd.train)

    def col(self, c):   # the address of column c of a table's first row
        assert 0 <= c < self.shape[-1]
        return self.ptr + c * self.host.element_size()

    def read(self, what):
        back = self.whole.cpu()
        assert torch.equal(_bits(back[:self.lo]), _bits(self.host[:self.lo])), f"{what}: wrote in front of the buffer"
        assert torch.equal(_bits(back[self.hi:]), _bits(self.host[self.hi:])), f"{what}: wrote past the end of the buffer"
        out = back[self.lo:self.hi].view(self.shape)
        if self.must_write:
            assert not bool(torch.isnan(out).any()), f"{what}: an element of a fully written output was left unwritten"
        return out


class Bufs(dict):
    def p(self, name):
        return self[name].ptr if name in self else None

    def finish(self, what):
        """-> name -> the payload as it is now, every canary checked, no NaN in a buffer that had to be written"""
        torch.cuda.synchronize()
        return {k: b.read((what, k)) for k, b in self.items()}


def alloc(entry, dims, data, off=None):
    """Every buffer of one call.  data: name -> CPU tensor (an input, or what a += output held before) or None (must be fully written).
    off: name -> 1 for a payload one float past the 16-byte boundary."""
    sh, off = _shapes(entry, **dims), off or {}
    assert set(data) <= set(sh) and set(off) <= set(data), (entry, set(data) - set(sh))
    out = Bufs()
    for name, val in data.items():
        assert val is None or tuple(val.shape) == tuple(sh[name]), (entry, name, tuple(val.shape), sh[name])
        out[name] = Buf(sh[name], val, off.get(name, 0), torch.int64 if name in _INT64 else torch.float32)
    return out


def _st():
    return torch.cuda.current_stream().cuda_stream


def call(entry, *args, expect=0):
    rc = getattr(_lib.lib(), entry)(*args, _st())
    assert rc == expect, (entry, rc, _lib.lib().dhw_train_last_error())


def close(entry, got, ref, what, rows=None):
    """max |got - ref| <= 2e-5 max |ref| over the tensor; with ``rows`` (a bool index over the leading dimensions flattened) also over
    those rows alone, so that a few rows of large values do not hide the others."""
    def one(g, r, w):
        assert g.shape == r.shape, (entry, w, g.shape, r.shape)
        err, scale = float((g.double() - r.double()).abs().max()), max(float(r.abs().max()), 1e-6)
        ratio = err / (TOL * scale)
        WORST[entry] = max(WORST.get(entry, 0.0), ratio)
        assert ratio <= 1.0, (entry, w, err, scale, ratio)
    one(got, ref, what)
    if rows is not None and bool(rows.any()) and not bool(rows.all()):
        k = rows.numel()
        one(got.reshape(k, -1)[rows], ref.reshape(k, -1)[rows], (what, "ordinary rows"))


def exact(got, want32, what):
    assert want32.dtype == torch.float32 and torch.equal(got, want32), (what, float((got - want32).abs().max()))


def same_bits(got, before, what):
    assert torch.equal(_bits(got.contiguous()), _bits(before.contiguous())), f"{what}: an element the call does not address changed"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- flat passes ------------------------------------------------------------------------------------------------------------------
FLAT_N = (1, 5, 1024, 1028, 1031)    # one full block of f32x4, one vector more, n % 4 != 0


def _flat_cases(form):
    if form == "vec":
        return [(n, 0) for n in FLAT_N if n % 4 == 0]
    return [(n, 1) for n in FLAT_N] + [(n, 0) for n in FLAT_N if n % 4]


def _unary_input(g, n):
    x = _randn(g, n)
    special = torch.tensor([0.0, -0.0, 20.0, -20.0, 88.0, -88.0])[:n]
    x[:special.numel()] = special
    return x


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_unary_forward(form):
    if form == "vec":
        _need_vec4()
    g = _gen(1)
    for i, ((n, off), kind) in enumerate(itertools.product(_flat_cases(form), (0, 1))):
        x = _unary_input(g, n)
        b = alloc("dhw_op_unary", dict(n=n), dict(x=x, y=None), {("x", "y")[i % 2]: 1} if off else None)
        call("dhw_op_unary", kind, b.p("x"), n, b.p("y"))
        y, ref = b.finish(("unary", n, off, kind))["y"], R.unary(kind, x)
        close("dhw_op_unary", y, ref, (n, off, kind))
        if n > 6:
            close("dhw_op_unary", y[6:], ref[6:], (n, off, kind, "N(0,1) part"))


def test_unary_backward():
    """(one kernel form: the launcher has no 16-byte one)"""
    g = _gen(2)
    for i, (n, off, acc, kind) in enumerate(itertools.product(FLAT_N, (0, 1), (0, 1), (0, 1))):
        x = _unary_input(g, n)
        t = x if kind == 0 else torch.sigmoid(x)
        dy, prev = _randn(g, n), _randn(g, n)
        b = alloc("dhw_op_unary_bwd", dict(n=n), dict(dy=dy, x=t, dx=prev if acc else None), {("dy", "x", "dx")[i % 3]: 1} if off else None)
        call("dhw_op_unary_bwd", kind, b.p("dy"), b.p("x"), n, b.p("dx"), acc)
        close("dhw_op_unary_bwd", b.finish(("unary_bwd", n, off, acc, kind))["dx"], R.unary_bwd(kind, dy, t, prev if acc else None), (n, off, acc, kind))


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_add(form):
    if form == "vec":
        _need_vec4()
    g = _gen(3)
    for i, ((n, off), acc, with_b) in enumerate(itertools.product(_flat_cases(form), (0, 1), (1, 0))):
        a, bb, prev = _randn(g, n), _randn(g, n), _randn(g, n)
        data = dict(a=a, out=prev if acc else None)
        if with_b:
            data["b"] = bb
        names = list(data)
        b = alloc("dhw_op_add", dict(n=n), data, {names[i % len(names)]: 1} if off else None)
        call("dhw_op_add", b.p("a"), b.p("b"), n, b.p("out"), acc)
        out = b.finish(("add", n, off, acc, with_b))["out"]
        if acc:
            close("dhw_op_add", out, R.add(a, bb if with_b else None, prev), (n, off, with_b))
        else:
            exact(out, a + bb if with_b else a, ("add", n, off, with_b))


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_mask_mul(form):
    if form == "vec":
        _need_vec4()
    g = _gen(4)
    s07 = float(np.float32(1.0 / 0.7))
    for i, ((n, off), (scale, acc)) in enumerate(itertools.product(_flat_cases(form), ((1.0, 0), (s07, 0), (s07, 1), (1.0, 1)))):
        x, prev = _randn(g, n), _randn(g, n)
        mask = (torch.rand(n, generator=g) >= 0.3).float()
        b = alloc("dhw_op_mask_mul", dict(n=n), dict(x=x, mask=mask, y=prev if acc else None), {("x", "mask", "y")[i % 3]: 1} if off else None)
        call("dhw_op_mask_mul", b.p("x"), b.p("mask"), scale, n, b.p("y"), acc)
        y = b.finish(("mask_mul", n, off, scale, acc))["y"]
        if scale == 1.0 and not acc:
            exact(y, x * mask, ("mask_mul", n, off))
        else:
            close("dhw_op_mask_mul", y, R.mask_mul(x, mask, scale, prev if acc else None), (n, off, scale, acc))


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_add_rows(form):
    if form == "vec":
        _need_vec4()
        cases = [((3, 5, 8), None), ((2, 3, 4), None)]
    else:
        cases = [((1, 1, 1), None), ((3, 5, 7), None), ((3, 5, 8), "table"), ((2, 3, 4), "x"), ((3, 5, 8), "out"), ((3, 5, 7), "table")]
    g = _gen(5)
    for (B, L, Cc), mis in cases:
        x, table = _randn(g, B, L, Cc), _randn(g, L, Cc)
        b = alloc("dhw_op_add_rows", dict(B=B, L=L, C=Cc), dict(x=x, table=table, out=None), {mis: 1} if mis else None)
        call("dhw_op_add_rows", b.p("x"), b.p("table"), B, L, Cc, b.p("out"))
        exact(b.finish(("add_rows", B, L, Cc, mis))["out"], x + table[None], ("add_rows", B, L, Cc, mis))


# ---- FiLM: gamma / beta rows [B][pstride] -------------------------------------------------------------------------------------------
def _film_params(g, B, Cc, ps):
    """-> (data for alloc, gamma, beta, gcol, bcol): ps == C: a table each; wider: ONE table, gamma at column 4 and beta = gamma + C"""
    gtab = _randn(g, B, ps)
    if ps == Cc:
        btab = _randn(g, B, ps)
        return dict(gtab=gtab, btab=btab), gtab, btab, 0, None
    assert ps >= 2 * Cc + 4
    return dict(gtab=gtab), gtab[:, 4:4 + Cc], gtab[:, 4 + Cc:4 + 2 * Cc], 4, 4 + Cc


def _film_ptrs(b, gcol, bcol):
    return b["gtab"].col(gcol), (b["btab"].col(0) if bcol is None else b["gtab"].col(bcol))


def _grad_tables(g, B, Cc, ps, bcol):
    """what dgamma / dbeta held before the call: random, in the layout of the parameter tables"""
    d = dict(dgtab=_randn(g, B, ps))
    if bcol is None:
        d["dbtab"] = _randn(g, B, ps)
    return d


def _check_grad_tables(entry, out, prev, Cc, gcol, bcol, ref_dg, ref_db, what):
    """dgamma / dbeta against the reference (which holds previous + sum); every other column of the tables bit-identical"""
    close(entry, out["dgtab"][:, gcol:gcol + Cc], ref_dg, (what, "dgamma"))
    touched = torch.zeros(out["dgtab"].shape[1], dtype=torch.bool)
    touched[gcol:gcol + Cc] = True
    if bcol is None:
        close(entry, out["dbtab"], ref_db, (what, "dbeta"))
    else:
        close(entry, out["dgtab"][:, bcol:bcol + Cc], ref_db, (what, "dbeta"))
        touched[bcol:bcol + Cc] = True
    same_bits(out["dgtab"][:, ~touched], prev["dgtab"][:, ~touched], (what, "other columns of the gradient table"))


def _prev_of(prev, Cc, gcol, bcol):
    pg = prev["dgtab"][:, gcol:gcol + Cc]
    return pg, (prev["dbtab"] if bcol is None else prev["dgtab"][:, bcol:bcol + Cc])


def test_film_forward_and_backward():
    """(one kernel form each way)  (2, 65, 66): a second 64-row chunk of one row and a second channel block of two channels — two
    blocks add into one dgamma"""
    g = _gen(6)
    for (B, L, Cc), wide, acc in itertools.product(((1, 1, 1), (3, 5, 7), (2, 65, 66)), (0, 1), (0, 1)):
        ps = 3 * Cc + 4 if wide else Cc
        what = ("film", B, L, Cc, ps, acc)
        pdata, gam, bet, gcol, bcol = _film_params(g, B, Cc, ps)
        x, dy, px = _randn(g, B, L, Cc), _randn(g, B, L, Cc), _randn(g, B, L, Cc)
        dims = dict(B=B, L=L, C=Cc, ps=ps)
        if not acc:   # (the forward has no accumulate: once per shape and stride)
            b = alloc("dhw_op_film", dims, dict(x=x, y=None, **pdata))
            call("dhw_op_film", b.p("x"), *_film_ptrs(b, gcol, bcol), ps, B, L, Cc, b.p("y"))
            close("dhw_op_film", b.finish(what)["y"], R.film(x, gam, bet), what)
        prev = _grad_tables(g, B, Cc, ps, bcol)
        b = alloc("dhw_op_film_bwd", dims, dict(dy=dy, x=x, gtab=pdata["gtab"], dx=px if acc else None, **prev))
        dgp = b["dgtab"].col(gcol)
        dbp = b["dbtab"].col(0) if bcol is None else b["dgtab"].col(bcol)
        call("dhw_op_film_bwd", b.p("dy"), b.p("x"), b["gtab"].col(gcol), ps, B, L, Cc, b.p("dx"), acc, dgp, dbp)
        out = b.finish(what)
        rdx, rdg, rdb = R.film_bwd(dy, x, gam, px if acc else None, *_prev_of(prev, Cc, gcol, bcol))
        close("dhw_op_film_bwd", out["dx"], rdx, (what, "dx"))
        _check_grad_tables("dhw_op_film_bwd", out, prev, Cc, gcol, bcol, rdg, rdb, what)


FILM_ACT_SHAPES = ((1, 1, 4, 4), (3, 5, 8, 24), (2, 17, 64, 256), (2, 65, 68, 208))


def test_film_act_forward():
    """(the forward has the 16-byte kernel only, whatever DHW_TRAIN_VEC4 says: nothing to skip)"""
    g = _gen(7)
    for (B, L, Cc, ps), act, with_add in itertools.product(FILM_ACT_SHAPES, (0, 1), (0, 1)):
        what = ("film_act", B, L, Cc, ps, act, with_add)
        pdata, gam, bet, gcol, bcol = _film_params(g, B, Cc, ps)
        x, addend = _randn(g, B, L, Cc), _randn(g, B, L, Cc)
        data = dict(x=x, y=None, **pdata)
        if with_add:
            data["addend"] = addend
        b = alloc("dhw_op_film_act", dict(B=B, L=L, C=Cc, ps=ps), data)
        call("dhw_op_film_act", b.p("x"), *_film_ptrs(b, gcol, bcol), ps, B, L, Cc, act, b.p("addend"), b.p("y"))
        close("dhw_op_film_act", b.finish(what)["y"], R.film_act(x, gam, bet, act, addend if with_add else None), what)


def test_film_act_forward_refuses_what_its_16_byte_kernel_cannot_take():
    """C % 4 != 0, pstride % 4 != 0 and a pointer that is not 16-byte aligned (x, gamma, beta, addend, y in turn): DHW_ERR_ARG, the
    error names the entry, nothing is launched — y stays NaN.  The same buffers, aligned, are accepted."""
    lib = _lib.lib()
    g = _gen(8)
    B, L, Cc, ps = 3, 5, 8, 24
    pdata, gam, bet, gcol, bcol = _film_params(g, B, Cc, ps)
    x, addend = _randn(g, B, L, Cc), _randn(g, B, L, Cc)
    b = alloc("dhw_op_film_act", dict(B=B, L=L, C=Cc, ps=ps), dict(x=x, addend=addend, y=None, **pdata))
    good = dict(x=b.p("x"), gamma=b["gtab"].col(gcol), beta=b["gtab"].col(bcol), addend=b.p("addend"), y=b.p("y"))

    def run(expect, C_=Cc, ps_=ps, **kw):
        a = dict(good, **kw)
        call("dhw_op_film_act", a["x"], a["gamma"], a["beta"], ps_, B, L, C_, 1, a["addend"], a["y"], expect=expect)

    bad = {"C % 4": dict(C_=6), "pstride % 4": dict(ps_=22)}
    bad.update({f"{k} misaligned": {k: good[k] + 4} for k in good})   # (one float further: still inside the buffer's own margin)
    for what, kw in bad.items():
        run(ERR_ARG, **kw)
        assert b"dhw_op_film_act" in lib.dhw_train_last_error(), what
    torch.cuda.synchronize()
    assert bool(torch.isnan(b["y"].whole[b["y"].lo:b["y"].hi].cpu()).all()), "a refused call wrote y"
    run(0)
    close("dhw_op_film_act", b.finish("film_act after refusals")["y"], R.film_act(x, gam, bet, 1, addend), "after refusals")


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_film_act_backward(form):
    if form == "vec":
        _need_vec4()
        cases = [(s, None) for s in FILM_ACT_SHAPES]
    else:
        cases = [(s, "dy") for s in FILM_ACT_SHAPES] + [((3, 5, 6, 16), None), ((2, 65, 6, 6), None), ((3, 5, 8, 24), "dx")]
    g = _gen(9)
    for ((B, L, Cc, ps), mis), act, acc in itertools.product(cases, (0, 1), (0, 1)):
        what = ("film_act_bwd", form, B, L, Cc, ps, mis, act, acc)
        pdata, gam, bet, gcol, bcol = _film_params(g, B, Cc, ps)
        x, dy, px = _randn(g, B, L, Cc), _randn(g, B, L, Cc), _randn(g, B, L, Cc)
        prev = _grad_tables(g, B, Cc, ps, bcol)
        b = alloc("dhw_op_film_act_bwd", dict(B=B, L=L, C=Cc, ps=ps), dict(dy=dy, x=x, dx=px if acc else None, **pdata, **prev), {mis: 1} if mis else None)
        dgp = b["dgtab"].col(gcol)
        dbp = b["dbtab"].col(0) if bcol is None else b["dgtab"].col(bcol)
        call("dhw_op_film_act_bwd", b.p("dy"), b.p("x"), *_film_ptrs(b, gcol, bcol), ps, B, L, Cc, act, b.p("dx"), acc, dgp, dbp)
        out = b.finish(what)
        rdx, rdg, rdb = R.film_act_bwd(dy, x, gam, bet, act, px if acc else None, *_prev_of(prev, Cc, gcol, bcol))
        close("dhw_op_film_act_bwd", out["dx"], rdx, (what, "dx"))
        _check_grad_tables("dhw_op_film_act_bwd", out, prev, Cc, gcol, bcol, rdg, rdb, what)


# ---- LayerNorm -> FiLM ----------------------------------------------------------------------------------------------------------------
LN_BL = ((1, 1), (3, 3), (2, 8), (2, 9), (3, 13))   # L below the 4 waves of a block, L = 8 and 8 + 1 (the backward's 8-row chunks), 13
LN_VEC_C = (4, 64, 100, 256, 260, 512)              # 260..512: the second register slot of the 16-byte forms
LN_SCALAR_C = (1, 7, 65, 130, 510)                  # 1..8 of the scalar backward's KMAX register slots


def _ln_cases(form):
    """(C, (B, L), wide table, (addend, act_out, pe), accumulate, misaligned operand): every C twice, with complementary options"""
    cs = [(c, None) for c in (LN_VEC_C if form == "vec" else LN_SCALAR_C)]
    if form == "scalar":
        cs += [(100, "x"), (516, None)]
    out = []
    for i, (c, mis) in enumerate(cs):
        opts = (i & 1, (i >> 1) & 1, (i >> 2) & 1)
        out.append((c, LN_BL[i % 5], i % 2, opts, i % 2, mis))
        out.append((c, LN_BL[(i + 2) % 5], 1 - i % 2, tuple(1 - o for o in opts), 1 - i % 2, mis))
    return out


def _ln_input(g, B, L, Cc):
    """N(0,1) rows; with three rows or more, row 1 is scaled by 1e-3 (variance ~1e-6: eps is half of the denominator) and the last row
    is all zero.  -> (x, ordinary rows)"""
    x = _randn(g, B, L, Cc)
    ordinary = torch.ones(B * L, dtype=torch.bool)
    if B * L >= 3:
        xr = x.view(B * L, Cc)
        xr[1] *= 1e-3
        xr[-1] = 0.0
        ordinary[1] = ordinary[-1] = False
    return x, ordinary


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_ln_film_forward(form):
    if form == "vec":
        _need_vec4()
    g = _gen(10)
    for Cc, (B, L), wide, (with_add, with_act, with_pe), _, mis in _ln_cases(form):
        ps = 2 * Cc + 8 if wide else Cc
        what = ("ln_film", form, Cc, B, L, ps, with_add, with_act, with_pe, mis)
        pdata, gam, bet, gcol, bcol = _film_params(g, B, Cc, ps)
        (x, ordinary), addend, pe = _ln_input(g, B, L, Cc), _randn(g, B, L, Cc), _randn(g, L, Cc)
        data = dict(x=x, y=None, mean=None, rstd=None, **pdata)
        if with_add:
            data["addend"] = addend
        if with_act:
            data["act_out"] = None
        if with_pe:
            data.update(pe=pe, pe_out=None)
        b = alloc("dhw_op_ln_film", dict(B=B, L=L, C=Cc, ps=ps), data, {mis: 1} if mis else None)
        call("dhw_op_ln_film", b.p("x"), B, L, Cc, *_film_ptrs(b, gcol, bcol), ps, b.p("addend"), b.p("y"), b.p("act_out"), b.p("pe"), b.p("pe_out"),
             b.p("mean"), b.p("rstd"))
        out = b.finish(what)
        y, ya, yp, mean, rstd = R.ln_film(x, gam, bet, addend if with_add else None, pe if with_pe else None)
        close("dhw_op_ln_film", out["y"], y, (what, "y"), ordinary)
        close("dhw_op_ln_film", out["mean"], mean, (what, "mean"), ordinary)
        close("dhw_op_ln_film", out["rstd"], rstd, (what, "rstd"), ordinary)
        if with_act:
            close("dhw_op_ln_film", out["act_out"], ya, (what, "act_out"), ordinary)
        if with_pe:
            close("dhw_op_ln_film", out["pe_out"], yp, (what, "pe_out"), ordinary)


@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_ln_film_backward(form):
    if form == "vec":
        _need_vec4()
    g = _gen(11)
    for Cc, (B, L), wide, _, acc, mis in _ln_cases(form):
        ps = 2 * Cc + 8 if wide else Cc
        what = ("ln_film_bwd", form, Cc, B, L, ps, acc, mis)
        pdata, gam, bet, gcol, bcol = _film_params(g, B, Cc, ps)
        (x, ordinary), dy, px = _ln_input(g, B, L, Cc), _randn(g, B, L, Cc), _randn(g, B, L, Cc)
        _, mean, rstd = R.layernorm(x)
        mean, rstd = mean.float(), rstd.float()                  # (what the forward saved: the backward's inputs)
        prev = _grad_tables(g, B, Cc, ps, bcol)
        refused = Cc > 512
        b = alloc("dhw_op_ln_film_bwd", dict(B=B, L=L, C=Cc, ps=ps),
                  dict(dy=dy, x=x, mean=mean, rstd=rstd, gtab=pdata["gtab"], dx=px if acc and not refused else None, **prev), {mis: 1} if mis else None)
        dgp = b["dgtab"].col(gcol)
        dbp = b["dbtab"].col(0) if bcol is None else b["dgtab"].col(bcol)
        call("dhw_op_ln_film_bwd", b.p("dy"), b.p("x"), b.p("mean"), b.p("rstd"), b["gtab"].col(gcol), ps, B, L, Cc, b.p("dx"), acc, dgp, dbp,
             expect=ERR_ARG if refused else 0)
        if refused:   # C = 516: more channels than a lane's register slots hold — refused, dx stays NaN, the gradient tables untouched
            assert b"dhw_op_ln_film_bwd" in _lib.lib().dhw_train_last_error()
            torch.cuda.synchronize()
            back = {k: v.whole.cpu()[v.lo:v.hi] for k, v in b.items()}
            assert bool(torch.isnan(back["dx"]).all()), "a refused call wrote dx"
            for k in prev:
                same_bits(back[k], prev[k].reshape(-1), (what, k))
            continue
        out = b.finish(what)
        rdx, rdg, rdb = R.ln_film_bwd(dy, x, mean, rstd, gam, px if acc else None, *_prev_of(prev, Cc, gcol, bcol))
        close("dhw_op_ln_film_bwd", out["dx"], rdx, (what, "dx"), ordinary)
        _check_grad_tables("dhw_op_ln_film_bwd", out, prev, Cc, gcol, bcol, rdg, rdb, what)


def test_layernorm_forward_and_backward():
    """(one kernel form each way)"""
    g = _gen(12)
    for (rows, Cc), acc in itertools.product(((1, 1), (5, 7), (9, 64), (6, 65), (4, 200)), (0, 1)):
        what = ("layernorm", rows, Cc, acc)
        x, ordinary = _ln_input(g, 1, rows, Cc)
        x = x.view(rows, Cc)
        y, mean, rstd = R.layernorm(x)
        if not acc:
            b = alloc("dhw_op_layernorm", dict(rows=rows, C=Cc), dict(x=x, y=None, mean=None, rstd=None))
            call("dhw_op_layernorm", b.p("x"), rows, Cc, b.p("y"), b.p("mean"), b.p("rstd"))
            out = b.finish(what)
            for k, r in (("y", y), ("mean", mean), ("rstd", rstd)):
                close("dhw_op_layernorm", out[k], r, (what, k), ordinary)
        dy, px = _randn(g, rows, Cc), _randn(g, rows, Cc)
        y32, rstd32 = y.float(), rstd.float()
        b = alloc("dhw_op_layernorm_bwd", dict(rows=rows, C=Cc), dict(dy=dy, y=y32, rstd=rstd32, dx=px if acc else None))
        call("dhw_op_layernorm_bwd", b.p("dy"), b.p("y"), b.p("rstd"), rows, Cc, b.p("dx"), acc)
        close("dhw_op_layernorm_bwd", b.finish(what)["dx"], R.layernorm_bwd(dy, y32, rstd32, px if acc else None), (what, "dx"), ordinary)


# ---- softmax ------------------------------------------------------------------------------------------------------------------------
SOFTMAX_COLS = (1, 10, 64, 65, 255, 256, 257, 300)   # register slots 0..3 of the <= 256 kernels, and the loop kernels


def _softmax_mask(B, cols):
    """a different padded tail per sample; sample 0 keeps a single key"""
    mask = torch.zeros(B, cols)
    mask[0, 1:] = 1
    for b in range(1, B):
        tail = min(cols - 1, max(1, cols // 3) + b)
        if tail:
            mask[b, cols - tail:] = 1
    return mask


def test_softmax_forward_and_backward():
    """(B, H, Lq) = (2, 3, 3): 18 rows, 9 per sample — a block of 4 rows has idle waves at the end and a sample boundary inside it.
    The kernel form follows cols alone (<= 256: rows in registers).  Backward out of place and in place (ds == dp, as Tape.attention
    calls it)."""
    g = _gen(13)
    B, H, Lq = 2, 3, 3
    Rr = H * Lq
    for i, cols in enumerate(SOFTMAX_COLS):
        for with_mask, scale in ((0, (1.0, 0.125)[i % 2]), (1, (0.125, 1.0)[i % 2])):
            what = ("softmax", cols, with_mask, scale)
            s = (_randn(g, B, Rr, cols) * 3.0 / scale).clamp(-16.0 / scale, 16.0 / scale)   # |s * scale| <= 16
            mask = _softmax_mask(B, cols)
            dims = dict(B=B, R=Rr, cols=cols)
            data = dict(s=s, p=None)
            if with_mask:
                data["mask"] = mask
            b = alloc("dhw_op_softmax", dims, data)
            call("dhw_op_softmax", b.p("s"), B * Rr, cols, Rr, b.p("mask"), scale, b.p("p"))
            p = b.finish(what)["p"]
            ref = R.softmax(s, mask if with_mask else None, scale)
            close("dhw_op_softmax", p, ref, what)
            assert float((p.double().sum(-1) - 1).abs().max()) <= 1e-6, what
            if with_mask:
                masked = mask[:, None].expand(B, Rr, cols) == 1
                assert bool((p[masked] == 0.0).all()), (what, "a masked key has a probability")
                assert bool((p[~masked] > 0.0).all()), what
            dp, p32 = _randn(g, B, Rr, cols), ref.float()
            want = R.softmax_bwd(dp, p32, scale)
            b = alloc("dhw_op_softmax_bwd", dims, dict(dp=dp, p=p32, ds=None))
            call("dhw_op_softmax_bwd", b.p("dp"), b.p("p"), B * Rr, cols, scale, b.p("ds"))
            close("dhw_op_softmax_bwd", b.finish(what)["ds"], want, (what, "out of place"))
            b = alloc("dhw_op_softmax_bwd", dims, dict(dp=dp, p=p32))
            call("dhw_op_softmax_bwd", b.p("dp"), b.p("p"), B * Rr, cols, scale, b.p("dp"))
            close("dhw_op_softmax_bwd", b.finish(what)["dp"], want, (what, "in place"))


# ---- AvgPool1d(2) / nearest x2 upsampling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["vec", "scalar"])
def test_resample(form):
    """16-byte form: C = 96 gives 24 lanes per row, which does not divide 256; C = 1024 one row per block.  C = 1028 is past the
    16-byte form's 1024 channels."""
    if form == "vec":
        _need_vec4()
        cs = [(4, None), (96, None), (128, None), (1024, None)]
    else:
        cs = [(1, None), (6, None), (1028, None), (96, "x"), (4, "y")]
    g = _gen(14)
    for (Cc, mis), mode, acc in itertools.product(cs, (0, 1, 2, 3), (0, 1)):
        for rows_out in ((1, 2, 11) if mode in (0, 3) else (2, 22)):
            what = ("resample", form, Cc, mis, mode, rows_out, acc)
            dims = dict(mode=mode, rows_out=rows_out, C=Cc)
            x = _randn(g, *_shapes("dhw_op_resample", **dims)["x"])
            prev = _randn(g, rows_out, Cc)
            b = alloc("dhw_op_resample", dims, dict(x=x, y=prev if acc else None), {mis: 1} if mis else None)
            call("dhw_op_resample", mode, b.p("x"), rows_out, Cc, b.p("y"), acc)
            y = b.finish(what)["y"]
            if acc:
                close("dhw_op_resample", y, R.resample(mode, x, prev), what)
            else:
                if mode in (0, 3):
                    want = 0.5 * (x[0::2] + x[1::2]) if mode == 0 else x[0::2] + x[1::2]
                else:
                    want = 0.5 * x.repeat_interleave(2, 0) if mode == 1 else x.repeat_interleave(2, 0)
                exact(y, want, what)


# ---- embedding, column sums ----------------------------------------------------------------------------------------------------------
def test_embedding_gather_and_scatter():
    """ids [2][rows / 2]: id 3 occurs in both rows, several times (its gradient row collects many atomic adds), the first and the last
    table row occur once; the other rows of dtable must come back bit-identical."""
    g = _gen(15)
    for rows, Cc in ((1, 1), (18, 48), (18, 257)):
        V = 1 if rows == 1 else 7
        ids = torch.zeros(rows, dtype=torch.int64) if rows == 1 else torch.tensor([0, 3, 3, 5, 3, 3, 3, 5, 3] + [3, 3, V - 1, 3, 3, 3, 3, 3, 3])
        what = ("embedding", rows, Cc)
        table, dy, prev = _randn(g, V, Cc), _randn(g, rows, Cc), _randn(g, V, Cc)
        b = alloc("dhw_op_embedding", dict(rows=rows, V=V, C=Cc), dict(ids=ids, table=table, y=None))
        call("dhw_op_embedding", b.p("ids"), b.p("table"), rows, Cc, b.p("y"))
        exact(b.finish(what)["y"], table[ids], what)
        b = alloc("dhw_op_embedding_bwd", dict(rows=rows, V=V, C=Cc), dict(ids=ids, dy=dy, dtable=prev))
        call("dhw_op_embedding_bwd", b.p("ids"), b.p("dy"), rows, Cc, b.p("dtable"))
        dt = b.finish(what)["dtable"]
        close("dhw_op_embedding_bwd", dt, R.embedding_bwd(ids, dy, prev), what)
        absent = torch.ones(V, dtype=torch.bool)
        absent[ids] = False
        assert rows == 1 or absent.tolist() == [False, True, True, False, True, False, False]
        same_bits(dt[absent], prev[absent], (what, "rows whose id does not occur"))


def test_colsum():
    g = _gen(16)
    for rows, Cc in ((1, 1), (63, 7), (65, 64), (130, 65), (257, 130)):
        dy, prev = _randn(g, rows, Cc), _randn(g, Cc)
        b = alloc("dhw_op_colsum", dict(rows=rows, C=Cc), dict(dy=dy, db=prev))
        call("dhw_op_colsum", b.p("dy"), rows, Cc, b.p("db"))
        close("dhw_op_colsum", b.finish(("colsum", rows, Cc))["db"], R.colsum(dy, prev), (rows, Cc))


# ---- the FiLM table -------------------------------------------------------------------------------------------------------------------
def _flat_layout(g, total):
    """The 32-float weight rows in permuted order with gaps (every woff a multiple of 4), the biases scattered between them: column j
    owns the 40-float slot perm[j] — 4 floats nobody names, 32 weights, then 4 floats of which one is its bias."""
    perm = torch.randperm(total, generator=g)
    woff = 40 * perm + 4
    boff = 40 * perm + 36 + torch.randint(0, 4, (total,), generator=g)
    return woff, boff, 40 * total + 8


@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_film_table_forward_and_backward(B):
    """B = 17: the forward's second 16-sample block holds one sample; B = 33: a second 32-sample chunk in the weight gradient and
    blockIdx.y = 1 in the sigma gradient.  total = 63 / 65: a partial 64-column block; 4101: the sigma gradient's 64 chunk walkers take
    a second chunk each (workgroup 0) and the last chunk has 5 columns."""
    g = _gen(17 + B)
    for total in (1, 63, 64, 65, 4101):
        what = ("film_table", B, total)
        woff, boff, nflat = _flat_layout(g, total)
        sigma, flat, dfilm = _randn(g, B, 32), _randn(g, nflat), _randn(g, B, total)
        pflat, psig = _randn(g, nflat), _randn(g, B, 32)
        dims = dict(B=B, total=total, nflat=nflat)
        b = alloc("dhw_op_film_table", dims, dict(sigma=sigma, flat=flat, woff=woff, boff=boff, film=None))
        call("dhw_op_film_table", b.p("sigma"), b.p("flat"), b.p("woff"), b.p("boff"), B, total, b.p("film"))
        close("dhw_op_film_table", b.finish(what)["film"], R.film_table(sigma, flat, woff, boff), what)
        b = alloc("dhw_op_film_table_bwd", dims, dict(dfilm=dfilm, sigma=sigma, flat=flat, woff=woff, boff=boff, grad_flat=pflat, dsigma=psig))
        call("dhw_op_film_table_bwd", b.p("dfilm"), b.p("sigma"), b.p("flat"), b.p("woff"), b.p("boff"), B, total, b.p("grad_flat"), b.p("dsigma"))
        out = b.finish(what)
        rflat, rsig = R.film_table_bwd(dfilm, sigma, flat, woff, boff, pflat, psig)
        close("dhw_op_film_table_bwd", out["grad_flat"], rflat, (what, "grad_flat"))
        close("dhw_op_film_table_bwd", out["dsigma"], rsig, (what, "dsigma"))
        named = torch.zeros(nflat, dtype=torch.bool)
        named[(woff[:, None] + torch.arange(32)[None]).reshape(-1)] = True
        named[boff] = True
        assert int((~named).sum()) == 7 * total + 8
        same_bits(out["grad_flat"][~named], pflat[~named], (what, "grad_flat slots no woff / boff names"))
        for k, v in (("dfilm", dfilm), ("sigma", sigma), ("flat", flat)):
            same_bits(out[k], v, (what, k))


# ---- keep masks -----------------------------------------------------------------------------------------------------------------------
SEED = 0x0123456789ABCDEF   # (both key words in use)


def _rng(index):
    return torch.tensor([SEED, index], dtype=torch.int64)


def test_keep_masks_equal_the_philox_reference_bit_for_bit():
    B, per, index = 3, 12, 5
    n = B * per
    got = {}
    for site, p in itertools.product((3, 4), (0.0, 0.3)):
        b = alloc("dhw_op_keep_mask", dict(n=n), dict(rng=_rng(index), keep=None))
        call("dhw_op_keep_mask", b.p("rng"), site, n, per, p, b.p("keep"))
        got[site, p] = b.finish(("keep_mask", site, p))["keep"]
        exact(got[site, p], torch.from_numpy(R.keep_mask(SEED, index, B, per, p, site)), ("keep_mask", site, p))
    assert bool((got[3, 0.0] == 1).all()) and bool((got[4, 0.0] == 1).all())
    assert not torch.equal(got[3, 0.3], got[4, 0.3]), "two dropout sites share one mask"
    assert not torch.equal(got[3, 0.3][:per], got[3, 0.3][per:2 * per]), "two samples share one mask"
    for p in (0.0, 0.3):   # the style mask of dhw_train_draw: word 3 of the counter is 2
        b = alloc("dhw_train_draw", dict(B=B, L=8, n_keep=n), dict(rng=_rng(index), eps=None, keep=None))
        call("dhw_train_draw", b.p("rng"), B, 8, b.p("eps"), n, per, p, b.p("keep"))
        keep = b.finish(("train_draw", p))["keep"]
        exact(keep, torch.from_numpy(R.keep_mask(SEED, index, B, per, p, 2)), ("train_draw keep", p))
    assert not torch.equal(keep, got[3, 0.3])


def test_draws_do_not_depend_on_how_the_batch_is_sharded():
    """sample b of draw d is stream d * B + b: the eps and the keep masks of draw d at B = 4 are those of draws 2d and 2d + 1 at B = 2,
    concatenated — exactly."""
    L, per, d, p = 8, 12, 5, 0.3

    def draw(B, index):
        b = alloc("dhw_train_draw", dict(B=B, L=L, n_keep=B * per), dict(rng=_rng(index), eps=None, keep=None))
        call("dhw_train_draw", b.p("rng"), B, L, b.p("eps"), B * per, per, p, b.p("keep"))
        out = b.finish(("train_draw", B, index))
        k = alloc("dhw_op_keep_mask", dict(n=B * per), dict(rng=_rng(index), keep=None))
        call("dhw_op_keep_mask", k.p("rng"), 3, B * per, per, p, k.p("keep"))
        return out["eps"], out["keep"], k.finish(("keep_mask", B, index))["keep"]

    whole, lo, hi = draw(4, d), draw(2, 2 * d), draw(2, 2 * d + 1)
    for k, name in enumerate(("eps", "style keep", "site keep")):
        assert torch.equal(_bits(whole[k].contiguous()), _bits(torch.cat([lo[k], hi[k]]).contiguous())), name
    assert not torch.equal(lo[0], hi[0]) and not torch.equal(lo[1], hi[1])


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
def test_loss_sums_and_gradients():
    """B 3, L 300: a second trip of the 256-thread loop with a 44-row tail.  pen_pred holds exact 0, exact 1, 1e-30 and 1 - 2^-24, each
    against pen = 0 and pen = 1 (the clamps of the logs at -100 and of the gradient's denominator at 1e-12).  Bounds as
    test_loss_and_its_gradient_match_the_reference."""
    g = _gen(18)
    B, L = 3, 300
    eps, score = _randn(g, B, L, 2), _randn(g, B, L, 2)
    pen = (torch.rand(B, L, generator=g) > 0.5).float()
    pp = 0.02 + 0.96 * torch.rand(B, L, generator=g)
    alphas = 0.05 + 0.9 * torch.rand(B, generator=g)
    edge = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24]
    for b_, l0 in ((0, 3), (1, 250), (2, 292)):                 # (first trip of the loop, the 256 boundary, the tail)
        for k, v in enumerate(edge):
            pp[b_, l0 + 2 * k], pp[b_, l0 + 2 * k + 1] = v, v
            pen[b_, l0 + 2 * k], pen[b_, l0 + 2 * k + 1] = 0.0, 1.0
    assert float(pp[0, 9]) == 1.0 - 2.0 ** -24 and float(pp[0, 7]) == float(np.float32(1e-30)) and float(pp[0, 5]) == 1.0
    out3, ds, dp = R.loss(eps, score, pen, pp, alphas)
    got3 = []
    for grads in (1, 0):
        data = dict(eps=eps, score_pred=score, pen=pen, pen_pred=pp, alphas=alphas, out3=None)
        if grads:
            data.update(d_score=None, d_pen_pred=None)
        b = alloc("dhw_train_loss", dict(B=B, L=L), data)
        call("dhw_train_loss", b.p("eps"), b.p("score_pred"), b.p("pen"), b.p("pen_pred"), b.p("alphas"), B, L, b.p("out3"), b.p("d_score"), b.p("d_pen_pred"))
        out = b.finish(("loss", grads))
        print("loss sums: got", out["out3"].tolist(), "ref", out3.tolist())
        assert np.allclose(out["out3"].numpy(), out3.numpy(), rtol=2e-6, atol=0), (out["out3"], out3)
        got3.append(out["out3"])
        if grads:
            for k, r in (("d_score", ds), ("d_pen_pred", dp)):
                err = ((out[k].double() - r).abs() / (1e-8 + 1e-5 * r.abs())).max()
                WORST["dhw_train_loss " + k + " (rtol 1e-5, atol 1e-8)"] = float(err)
                assert np.allclose(out[k].numpy(), r.numpy(), rtol=1e-5, atol=1e-8), (k, float(err))
    assert np.allclose(got3[0].numpy(), got3[1].numpy(), rtol=2e-6, atol=0)


# ---- the gradient norm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", [(1, 0), (3, 0), (1029, 0), (3700001, 0), (4099, 1)])
def test_squared_gradient_norm_of_ones_is_the_element_count(n, off):
    """dhw_train_adam_dev through train.Adam.step_dev with lr 0 and no clipping on an all-ones gradient: every partial sum is an integer
    below 2^24, so sqnorm must be n EXACTLY — a dropped tail element or a dropped pass shows.  3 700 001: n / 4 > 7 * 512 * 256, the
    8-deep pass, then the 2-deep one, a last vector and one tail element; (4099, off 1): the gradient one float past a 16-byte
    boundary — the scalar branch.  p stays as it was, m = (1 - beta1) g, v = (1 - beta2) g^2."""
    g = _gen(19)
    p0 = _randn(g, n)
    b = alloc("dhw_train_adam_dev", dict(n=n), dict(p=p0, g=torch.ones(n), hyper=torch.zeros(9), sqnorm=torch.full((1,), float("nan"))), {"g": 1} if off else None)
    assert (b["g"].ptr % 16 != 0) == bool(off)
    ad = train.Adam([b["p"].view], weight_decay=0.0, max_norm=0.0)
    hyper = ad.hyper(0.0)
    assert hyper[0] == 0.0 and hyper[7] == 0.0 and hyper[8] == 1.0
    b["hyper"].view.copy_(torch.tensor(hyper))
    ad.step_dev([b["g"].view], b["hyper"].view, b["sqnorm"].view)
    out = b.finish(("adam_dev", n, off))
    assert float(out["sqnorm"][0]) == float(n), (float(out["sqnorm"][0]), n)
    same_bits(out["p"], p0, "p at lr 0")
    same_bits(out["g"], torch.ones(n), "g")
    m, v = ad.m[0].cpu(), ad.v[0].cpu()
    b1, b2 = np.float32(0.9), np.float32(0.98)
    assert torch.allclose(m, torch.full((n,), float(np.float32(1) - b1)), rtol=2e-7, atol=0)
    assert torch.allclose(v, torch.full((n,), float(np.float32(1) - b2)), rtol=2e-7, atol=0)
