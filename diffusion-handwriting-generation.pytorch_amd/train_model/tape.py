"""The tape engine: ``Var`` / ``_ViewVar`` (a tensor and its gradient buffer) and ``Tape`` — the raw launch wrappers over
include/dhw_train.h ``dhw_op_*`` and every differentiable op, each of which appends its backward closure."""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from .. import _lib
from ..train import _stream, _tcheck

_F = 4  # bytes per element


# DHW_TRAIN_FUSE_DSILU=0: SiLU's backward as its own pass again instead of a factor in the consuming GEMM's data-gradient output (A/B)
FUSE_DSILU = os.environ.get("DHW_TRAIN_FUSE_DSILU", "1") != "0"


class Var:
    """A node of the tape: a device tensor and its lazily allocated (zero-initialised) gradient.  ``leaf``: a network input
    whose gradient nobody needs (the backward sweep skips the kernels that would only produce it)."""
    __slots__ = ("d", "g", "leaf", "pre")

    def __init__(self, d: torch.Tensor, leaf: bool = False):
        self.d = d
        self.g = None
        self.leaf = leaf
        self.pre = None     # self = SiLU(pre): a GEMM that consumes self sends its data gradient straight to pre (dhw_gemm_desc.dsilu_of)

    def grad(self) -> torch.Tensor:
        if self.g is None:
            self.g = torch.zeros_like(self.d)
        return self.g


class _ViewVar(Var):
    """A reshaped alias of another Var: shares the data AND the gradient storage (reshape_up is a pure view)."""
    __slots__ = ("base", "shape")

    def __init__(self, base: Var, shape):
        super().__init__(base.d.view(*shape), base.leaf)
        self.base, self.shape = base, shape

    def grad(self):
        if self.g is None:
            self.g = self.base.grad().view(*self.shape)
        return self.g


def splits_k(R: int, N: int, K: int) -> bool:
    """Few output tiles and a long contraction (sigma_ffn's 2048 -> 32): the output is zeroed and the GEMM splits K over workgroups
    with atomics, instead of one workgroup walking all of K.  Such an output takes no addend, SiLU or FiLM rider."""
    return -(-R // 64) * -(-N // 64) < 64 and K >= 512


class Tape:
    """Forward ops append their backward closure; ``backward()`` replays them in reverse.  Every backward kernel ADDS into
    the input's gradient buffer (zero-initialised on first touch), which is how autograd's fan-in sums arise."""

    def __init__(self, device, bf16: bool = False):
        self.dev = device
        self.bf16 = int(bf16)   # GEMM operands rounded to bf16 inside the kernel (fp32 accumulation); everything else stays fp32
        self.lib = _lib.lib()
        self.st = _stream(device)
        self.steps = []
        self.launches = 0
        self.flops = 0          # algorithmic FLOPs of every GEMM issued (2 M N K per batch entry)

    # ---- raw kernel wrappers ---------------------------------------------------------------------------------------
    def new(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, device=self.dev, dtype=torch.float32)

    def gemm(self, *args, **kw):
        """One GEMM launch; arguments as ``gemm_desc``."""
        d = self.gemm_desc(*args, **kw)
        _tcheck(self.lib.dhw_op_gemm(C.byref(d), self.st))
        self.launches += 1

    def gemm_pair(self, first, second):
        """Two independent GEMMs — ``first`` / ``second``: (args, kwargs) of ``gemm_desc``, or None — as ONE launch where the
        library can pair them (dhw_op_gemm2: a layer's weight gradient, first, with its data gradient)."""
        if first is None or second is None:
            one = first if second is None else second
            return self.gemm(*one[0], **one[1])
        d0, d1 = self.gemm_desc(*first[0], **first[1]), self.gemm_desc(*second[0], **second[1])
        n = self.lib.dhw_op_gemm2(C.byref(d0), C.byref(d1), self.st)     # (returns the launches it issued: 1, or 2 where the forms do not pair)
        _tcheck(n)
        self.launches += n

    def gemm_group(self, items):
        """Up to six independent GEMMs — ``items``: (args, kwargs) of ``gemm_desc`` (None entries are skipped), dispatched in that
        order — as one launch where the library can group them (dhw_op_gemm_group)."""
        items = [it for it in items if it is not None]
        for i in range(0, len(items), 6):
            chunk = items[i:i + 6]
            if len(chunk) == 1:
                self.gemm(*chunk[0][0], **chunk[0][1])
                continue
            descs = [self.gemm_desc(*a, **k) for a, k in chunk]
            arr = (_lib.GemmDesc * len(descs))(*descs)
            n = self.lib.dhw_op_gemm_group(arr, len(descs), self.st)
            _tcheck(n)
            self.launches += n

    def gemm_desc(self, A, a_off, sam, sak, Bm, b_off, sbk, sbn, Cm, c_off, scm, scn, M, N, K, *, bias=None, alpha=1.0, acc=False,
                  nzo=1, nzi=1, za=(0, 0), zb=(0, 0), zc=(0, 0), a_shift=0, b_shift=0, lr=0, taps=1, a_tap_shift=0, sbt=0, b_z_shift=0,
                  rowsum=None, addend=None, act_out=None, dsilu_of=None, film=None):
        """See dhw_gemm_desc (include/dhw_train.h).  Extents are checked here, on the host, before the launch.  ``film``: (gamma
        pointer, beta pointer, table row stride, rows per sample, act, out tensor, addend tensor or None) — FiLM (+ SiLU) (+ addend)
        of the written value as a further output of the pass."""
        Kt = K // taps

        def extent(off, s0, n0, s1, n1, z, tap_stride=0):
            return off + (n0 - 1) * s0 + (n1 - 1) * s1 + (nzo - 1) * z[0] + (nzi - 1) * z[1] + (taps - 1) * tap_stride
        if extent(a_off, sam, M, sak, Kt, za) >= A.numel() or extent(b_off, sbk, Kt, sbn, N, zb, sbt) >= Bm.numel() \
                or extent(c_off, scm, M, scn, N, zc) >= Cm.numel() or min(a_off, b_off, c_off) < 0:
            raise ValueError("gemm operand extents exceed their buffers")
        if max(A.numel(), Bm.numel(), Cm.numel()) >= 2 ** 31:
            raise ValueError("gemm operands are addressed with 32-bit element offsets")
        if (a_shift or a_tap_shift) and (lr < 1 or M % lr):
            raise ValueError("a row-shifted gemm needs whole samples of lr rows")
        if (b_shift or b_z_shift) and (lr < 1 or Kt % lr):
            raise ValueError("a row-shifted gemm needs whole samples of lr rows")
        d = _lib.GemmDesc(A.data_ptr() + a_off * _F, sam, sak, za[0], za[1], a_shift, a_tap_shift,
                          Bm.data_ptr() + b_off * _F, sbk, sbn, zb[0], zb[1], sbt, b_shift, b_z_shift,
                          Cm.data_ptr() + c_off * _F, scm, scn, zc[0], zc[1],
                          M, N, K, nzo, nzi, lr, taps, bias.data_ptr() if bias is not None else None, alpha, int(acc), self.bf16,
                          act_out.data_ptr() if act_out is not None else None, addend.data_ptr() if addend is not None else None,
                          dsilu_of.data_ptr() if dsilu_of is not None else None, rowsum.data_ptr() if rowsum is not None else None)
        if film is not None:
            fg, fb, fps, frows, fact, fout, fadd = film
            if fout.numel() != Cm.numel() or scn != 1 or nzo * nzi != 1 or acc:
                raise ValueError("a FiLM output rides on an unbatched row-major GEMM without accumulation")
            d.film_gamma, d.film_beta, d.film_pstride, d.film_rows, d.film_act = fg, fb, fps, frows, int(fact)
            d.film_out, d.film_addend = fout.data_ptr(), fadd.data_ptr() if fadd is not None else None
        d._keep = (A, Bm, Cm, bias, act_out, addend, dsilu_of, rowsum, film)   # (the operands outlive the descriptor's use)
        self.flops += 2 * M * N * K * nzo * nzi
        return d

    def into(self, v: "Var"):
        """(gradient buffer of v, accumulate flag): the first writer overwrites a fresh buffer, later ones add."""
        if v.g is not None:
            return v.g, 1
        if isinstance(v, _ViewVar):
            base, _ = self.into(v.base)
            v.g = base.view(*v.shape)
        else:
            v.g = torch.empty_like(v.d)
        return v.g, 0

    def call(self, fn, *args):
        _tcheck(getattr(self.lib, fn)(*args, self.st))
        self.launches += 1

    def _grad_to(self, v: "Var", dy: torch.Tensor, take: bool = True) -> bool:
        """d v (+)= dy, where the gradient buffer dy is dead afterwards (its owner's consumers ran before it in the reverse sweep):
        with ``take``, a v without a gradient simply TAKES the buffer (later fan-in adds go into it; never a _ViewVar, whose gradient
        lives inside its base's) and True is returned; else one add."""
        if take and v.g is None and not isinstance(v, _ViewVar):
            v.g = dy
            return True
        dv, acc = self.into(v)
        self.call("dhw_op_add", dy.data_ptr(), None, dy.numel(), dv.data_ptr(), acc)
        return False

    def _addend_grad(self, addend: "Var | None", dy: torch.Tensor):
        """The backward of ``addend`` riding on an op's output pass: d addend (+)= dy (nothing to do for a network input)."""
        if addend is not None and not addend.leaf:
            self._grad_to(addend, dy)

    def _dgrad_dest(self, x: "Var"):
        """Where a GEMM's data gradient into x goes: (buffer, accumulate flag, ``dsilu_of`` tensor or None).  x = SiLU(u): the GEMM
        writes d u (+)= (.) * SiLU'(u) in its output pass, and x's own backward has nothing to do."""
        dx, acc = self.into(x.pre if x.pre is not None else x)
        return dx, acc, x.pre.d if x.pre is not None else None

    def _linear_grads(self, x: "Var", W: "Var", b: "Var | None", dy: torch.Tensor):
        """(weight-gradient item, data-gradient item or None for a network input) of y = x W^T + b, as (args, kwargs) of
        ``gemm_desc``: dW += dy^T x with db += column sums of dy riding along, and dx (+)= dy W.  Both read dy, neither the
        other's output: they can share a launch."""
        (R, K), N = x.d.shape, W.d.shape[0]
        dgrad = None
        if not x.leaf:
            dx, acc, pre = self._dgrad_dest(x)
            dgrad = ((dy, 0, N, 1, W.d, 0, K, 1, dx, 0, K, 1, R, K, N), dict(acc=acc, dsilu_of=pre))
        return ((dy, 0, 1, N, x.d, 0, K, 1, W.grad(), 0, K, 1, N, K, R), dict(acc=True, rowsum=b.grad() if b is not None else None)), dgrad

    # ---- differentiable ops ------------------------------------------------------------------------------------------
    def linear(self, x: Var, W: Var, b: Var | None, addend: Var | None = None, silu_out: bool = False, film=None):
        """nn.Linear on rows: x [R, K], W [N, K] (torch layout) -> [R, N]; ``addend`` [R, N]: the residual added to the result
        in the GEMM's output pass (y = x W^T + b + addend).  ``film`` = (table, col_g, col_b, B, act, addend): returns
        film_cols(y, ...) instead, evaluated in the same pass."""
        (R, K), N = x.d.shape, W.d.shape[0]
        split = splits_k(R, N, K)
        if film is not None and split:                    # (the FiLM as its own pass)
            return self.film_cols(self.linear(x, W, b, addend), *film)
        if (addend is not None or silu_out) and split:    # (separate passes)
            y = self.linear(x, W, b)
            y = self.add(y, addend) if addend is not None else y
            return (y, self.silu(y)) if silu_out else y
        y = Var(torch.zeros(R, N, device=self.dev) if split else self.new(R, N))
        act = self.new(R, N) if silu_out else None     # ``silu_out``: also returns SiLU(y), written by the same GEMM pass
        fout, frider = self._film_rider(R, N, film) if film is not None else (None, None)
        self.gemm(x.d, 0, K, 1, W.d, 0, 1, K, y.d, 0, N, 1, R, N, K, bias=b.d if b is not None else None, acc=split,
                  addend=addend.d if addend is not None else None, act_out=act, film=frider)

        def bwd():
            self.gemm_pair(*self._linear_grads(x, W, b, y.g))      # (one launch where the forms pair)
            self._addend_grad(addend, y.g)
        self.record(y, bwd)
        if film is not None:
            return self._film_record(y, fout, film)
        return (y, self.unary(0, y, act)) if silu_out else y

    def linear_group(self, specs):
        """Independent nn.Linears — ``specs``: [(x, W, b)], e.g. the q / k / v projections of one attention — as ONE launch forward
        and, backward, one launch for their weight gradients and every data gradient whose destination no other member writes
        (two projections of the same input add into the same gradient buffer: the second one follows in its own launch)."""
        if any(x.leaf or splits_k(x.d.shape[0], W.d.shape[0], x.d.shape[1]) for x, W, _ in specs):
            return [self.linear(x, W, b) for x, W, b in specs]
        ys, items = [], []
        for x, W, b in specs:
            (R, K), N = x.d.shape, W.d.shape[0]
            y = Var(self.new(R, N))
            ys.append(y)
            items.append(((x.d, 0, K, 1, W.d, 0, 1, K, y.d, 0, N, 1, R, N, K), dict(bias=b.d if b is not None else None)))
        self.gemm_group(items)

        def bwd():
            grads = [self._linear_grads(x, W, b, y.g) for (x, W, b), y in zip(specs, ys) if y.g is not None]
            group, later, written = [wgrad for wgrad, _ in grads], [], set()
            for _, dgrad in grads:
                dx = dgrad[0][8]      # (Cm of gemm_desc)
                (later if dx.data_ptr() in written else group).append(dgrad)
                written.add(dx.data_ptr())
            if group:
                self.gemm_group(group)
            for a, k in later:
                self.gemm(*a, **k)
        self.steps.append(bwd)
        return ys

    def conv3(self, x: Var, W: Var, b: Var, L: int, addend: Var | None = None, silu_out: bool = False, defer: list | None = None, film=None):
        """nn.Conv1d(k=3, padding='same') on C-last rows: x [B*L, Cin], W [Cout, Cin, 3] -> [B*L, Cout].  W (and its gradient) may
        have any strides: TrainModel keeps the Conv1d weights as [tap][Cout][Cin] in memory (unit stride along Cin), which makes the
        weight the 16-byte-load operand of all three GEMMs; a torch-contiguous W works too (scalar loads, stride-3 stores)."""
        (R, Cin), Cout = x.d.shape, W.d.shape[0]
        sco, sci, st = W.d.stride()
        y = Var(self.new(R, Cout))
        merged = Cin % 32 == 0 and Cout % 32 == 0      # the three taps as one contraction over K = 3 Cin (dhw_gemm_desc.taps)
        act = self.new(R, Cout) if silu_out and merged else None
        fout, frider = self._film_rider(R, Cout, film) if film is not None and merged else (None, None)   # (``film``: as in ``linear``)
        if merged:
            fwd = ((x.d, 0, Cin, 1, W.d, 0, sci, sco, y.d, 0, Cout, 1, R, Cout, 3 * Cin),
                   dict(bias=b.d, taps=3, a_shift=-1, a_tap_shift=1, sbt=st, lr=L, addend=addend.d if addend is not None else None, act_out=act, film=frider))
            if defer is not None:      # (the caller launches it together with other independent GEMMs: gemm_group)
                defer.append(fwd)
            else:
                self.gemm(*fwd[0], **fwd[1])
        else:
            for t in range(3):
                self.gemm(x.d, 0, Cin, 1, W.d, t * st, sci, sco, y.d, 0, Cout, 1, R, Cout, Cin, bias=b.d if t == 0 else None, acc=t > 0,
                          a_shift=t - 1, lr=L, addend=addend.d if addend is not None and t == 0 else None)

        def bwd():
            dy, dW, db = y.g, W.grad(), b.grad()
            gco, gci, gt = dW.stride()
            dx, acc, pre = self._dgrad_dest(x) if merged else (*self.into(x), None)    # (the three-GEMM path writes d x itself)
            # dx[r] += sum_t dy[r - (t-1)] W[:, :, t];  dW[:, :, t] += dy^T x[r + (t-1)]
            if merged:   # (weight gradient — the taps as the inner batch index, db riding along — and data gradient in one launch)
                self.gemm_pair(((dy, 0, 1, Cout, x.d, 0, Cin, 1, dW, 0, gco, gci, Cout, Cin, R),
                                dict(acc=True, nzi=3, zc=(0, gt), b_shift=-1, b_z_shift=1, lr=L, rowsum=db)),
                               ((dy, 0, Cout, 1, W.d, 0, sco, sci, dx, 0, Cin, 1, R, Cin, 3 * Cout),
                                dict(acc=acc, taps=3, a_shift=1, a_tap_shift=-1, sbt=st, lr=L, dsilu_of=pre)))
            else:
                for t in range(3):
                    self.gemm(dy, 0, Cout, 1, W.d, t * st, sco, sci, dx, 0, Cin, 1, R, Cin, Cout, acc=acc or t > 0, a_shift=1 - t, lr=L)
                    self.gemm(dy, 0, 1, Cout, x.d, 0, Cin, 1, dW, t * gt, gco, gci, Cout, Cin, R, acc=True, b_shift=t - 1, lr=L,
                              rowsum=db if t == 1 else None)
            self._addend_grad(addend, dy)
        self.record(y, bwd)
        if film is not None:
            return self._film_record(y, fout, film) if merged else self.film_cols(y, *film)
        return (y, self.unary(0, y, act)) if silu_out else y       # (three-GEMM path: act is None, SiLU as its own pass)

    def unary(self, kind: int, x: Var, out: torch.Tensor | None = None) -> Var:
        """kind 0: SiLU, 1: sigmoid.  ``out``: the values are there already, written by the pass that produced x (``silu_out`` of
        linear / conv3 / ln_film_cols) — only the backward is recorded (after x's, so it runs first and adds into x.g)."""
        y = Var(out if out is not None else torch.empty_like(x.d), leaf=x.leaf)     # a function of inputs only needs no gradient either
        n = x.d.numel()
        if out is None:
            self.call("dhw_op_unary", kind, x.d.data_ptr(), n, y.d.data_ptr())
        if kind == 0 and not x.leaf and FUSE_DSILU:
            y.pre = x
        saved = x.d if kind == 0 else y.d
        def bwd():
            if x.leaf:
                return
            dx, acc = self.into(x)
            self.call("dhw_op_unary_bwd", kind, y.g.data_ptr(), saved.data_ptr(), n, dx.data_ptr(), acc)
        self.record(y, bwd)
        return y

    def silu(self, x):
        return self.unary(0, x)

    def sigmoid(self, x):
        return self.unary(1, x)

    def add(self, a: Var, b: Var) -> Var:
        y = Var(torch.empty_like(a.d))
        self.call("dhw_op_add", a.d.data_ptr(), b.d.data_ptr(), a.d.numel(), y.d.data_ptr(), 0)

        def bwd():
            # d a = d b = d y: at most one of the two takes y's dead buffer, the other one needs a copy / an add — one launch per
            # residual add in the backward instead of two
            taken = self._grad_to(a, y.g)
            self._grad_to(b, y.g, take=not taken)
        self.record(y, bwd)
        return y

    def add_rows(self, x: Var, table: torch.Tensor, B: int) -> Var:
        R, Cc = x.d.shape
        y = Var(torch.empty_like(x.d))
        self.call("dhw_op_add_rows", x.d.data_ptr(), table.data_ptr(), B, R // B, Cc, y.d.data_ptr())
        self.record(y, lambda: self._grad_to(x, y.g))     # d x = d y
        return y

    def film(self, x: Var, gamma: Var, beta: Var, B: int) -> Var:
        """x * gamma[b] + beta[b] (conditioning.py:23-26); gamma, beta [B, C]."""
        R, Cc = x.d.shape
        L = R // B
        y = Var(torch.empty_like(x.d))
        self.call("dhw_op_film", x.d.data_ptr(), gamma.d.data_ptr(), beta.d.data_ptr(), Cc, B, L, Cc, y.d.data_ptr())
        def bwd():
            dx, acc = self.into(x)
            self.call("dhw_op_film_bwd", y.g.data_ptr(), x.d.data_ptr(), gamma.d.data_ptr(), Cc, B, L, Cc, dx.data_ptr(), acc,
                      gamma.grad().data_ptr(), beta.grad().data_ptr())
        self.record(y, bwd)
        return y

    def _cols(self, t: torch.Tensor, col_g: int, col_b: int):
        """The addresses of columns col_g and col_b in the first row of a [B, TOT] table (or of its gradient)."""
        return t.data_ptr() + col_g * _F, t.data_ptr() + col_b * _F

    def _film_rider(self, R: int, Cc: int, spec):
        """``spec`` = (table, col_g, col_b, B, act, addend): the FiLM output tensor of a GEMM that evaluates film_cols in its own
        output pass, and the ``film`` tuple of ``gemm_desc``."""
        table, col_g, col_b, B, act, addend = spec
        out = self.new(R, Cc)
        return out, (*self._cols(table.d, col_g, col_b), table.d.shape[1], R // B, bool(act), out, addend.d if addend is not None else None)

    def _film_record(self, u: Var, out: torch.Tensor, spec) -> Var:
        """The Var of the FiLM output ``out`` of ``u`` — written by film_cols' own pass or by the GEMM that produced u — and its
        backward (the FiLM output is recomputed there, not stored)."""
        table, col_g, col_b, B, act, addend = spec
        R, Cc = u.d.shape
        L, TOT = R // B, table.d.shape[1]
        y = Var(out)

        def bwd():
            dx, acc = self.into(u)
            self.call("dhw_op_film_act_bwd", y.g.data_ptr(), u.d.data_ptr(), *self._cols(table.d, col_g, col_b), TOT, B, L, Cc, int(act),
                      dx.data_ptr(), acc, *self._cols(table.grad(), col_g, col_b))
            self._addend_grad(addend, y.g)
        self.record(y, bwd)
        return y

    def film_cols(self, x: Var, table: Var, col_g: int, col_b: int, B: int, act: bool = False, addend: Var | None = None) -> Var:
        """``film`` with gamma / beta taken from columns [col, col + C) of a [B, TOT] table (dhw_op_film_table); ``act``: followed
        by SiLU in the same pass (the ConvBlock's ``SiLU(affine(conv(.)))``, cnn.py:70-80) — one launch each way instead of two,
        the FiLM output is recomputed in the backward instead of stored."""
        R, Cc = x.d.shape
        out = torch.empty_like(x.d)
        self.call("dhw_op_film_act", x.d.data_ptr(), *self._cols(table.d, col_g, col_b), table.d.shape[1], B, R // B, Cc, int(act),
                  addend.d.data_ptr() if addend is not None else None, out.data_ptr())
        return self._film_record(x, out, (table, col_g, col_b, B, act, addend))

    def ln_film_cols(self, x: Var, table: Var, col_g: int, col_b: int, B: int, addend: Var | None = None, silu_out: bool = False,
                     pe: torch.Tensor | None = None):
        """LayerNorm followed by FiLM (every EncoderLayer / TextStyleEncoder pairs them: model.py:44-58, text_style.py:98-110) in one
        pass each way; the normalised rows are recomputed in the backward from the saved mean / rstd."""
        R, Cc = x.d.shape
        L, TOT = R // B, table.d.shape[1]
        y = Var(torch.empty_like(x.d))
        mean, rstd = self.new(R), self.new(R)
        act = torch.empty_like(x.d) if silu_out else None
        ype = torch.empty_like(x.d) if pe is not None else None     # ``pe`` [L, C]: also returns y + pe[l] (add_rows of the result) from the same pass
        self.call("dhw_op_ln_film", x.d.data_ptr(), B, L, Cc, *self._cols(table.d, col_g, col_b), TOT,
                  addend.d.data_ptr() if addend is not None else None, y.d.data_ptr(), act.data_ptr() if silu_out else None,
                  pe.data_ptr() if pe is not None else None, ype.data_ptr() if pe is not None else None, mean.data_ptr(), rstd.data_ptr())

        def bwd():
            dx, acc = self.into(x)
            self.call("dhw_op_ln_film_bwd", y.g.data_ptr(), x.d.data_ptr(), mean.data_ptr(), rstd.data_ptr(), self._cols(table.d, col_g, col_b)[0], TOT, B, L, Cc,
                      dx.data_ptr(), acc, *self._cols(table.grad(), col_g, col_b))
            self._addend_grad(addend, y.g)
        self.record(y, bwd)
        outs = [y]
        if silu_out:
            outs.append(self.unary(0, y, act))
        if pe is not None:
            yp = Var(ype)
            self.record(yp, lambda: self._grad_to(y, yp.g))     # d y (+)= d (y + pe)
            outs.append(yp)
        return outs[0] if len(outs) == 1 else tuple(outs)

    def layernorm(self, x: Var) -> Var:
        R, Cc = x.d.shape
        y = Var(torch.empty_like(x.d))
        mean, rstd = self.new(R), self.new(R)
        self.call("dhw_op_layernorm", x.d.data_ptr(), R, Cc, y.d.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        def bwd():
            dx, acc = self.into(x)
            self.call("dhw_op_layernorm_bwd", y.g.data_ptr(), y.d.data_ptr(), rstd.data_ptr(), R, Cc, dx.data_ptr(), acc)
        self.record(y, bwd)
        return y

    def resample(self, mode: int, x: Var) -> Var:
        """mode 0: AvgPool1d(2); mode 2: Upsample(x2, nearest) — over the row axis of C-last rows (L even)."""
        R, Cc = x.d.shape
        Ro = R // 2 if mode == 0 else R * 2
        y = Var(self.new(Ro, Cc))
        self.call("dhw_op_resample", mode, x.d.data_ptr(), Ro, Cc, y.d.data_ptr(), 0)
        def bwd():
            dx, acc = self.into(x)
            self.call("dhw_op_resample", mode + 1, y.g.data_ptr(), R, Cc, dx.data_ptr(), acc)
        self.record(y, bwd)
        return y

    def embedding(self, ids: torch.Tensor, table: Var) -> Var:
        R = ids.numel()
        Cc = table.d.shape[1]
        y = Var(self.new(R, Cc))
        self.call("dhw_op_embedding", ids.data_ptr(), table.d.data_ptr(), R, Cc, y.d.data_ptr())
        self.record(y, lambda: self.call("dhw_op_embedding_bwd", ids.data_ptr(), y.g.data_ptr(), R, Cc, table.grad().data_ptr()))
        return y

    def attention(self, q: Var, k: Var, v: Var, B: int, H: int, mask: torch.Tensor | None) -> Var:
        """scaled_dp_attn over heads (attention.py:26-45, 77-87): q [B*Lq, H*D], k / v [B*Lk, H*D] -> [B*Lq, H*D].
        Heads are addressed by strides (no split / merge copies)."""
        HD = q.d.shape[1]
        D = HD // H
        Lq, Lk = q.d.shape[0] // B, k.d.shape[0] // B
        scale = 1.0 / math.sqrt(D)
        S = self.new(B, H, Lq, Lk)
        P = self.new(B, H, Lq, Lk)
        o = Var(self.new(B * Lq, HD))
        zq, zk, zs = (Lq * HD, D), (Lk * HD, D), (H * Lq * Lk, Lq * Lk)
        self.gemm(q.d, 0, HD, 1, k.d, 0, 1, HD, S, 0, Lk, 1, Lq, Lk, D, nzo=B, nzi=H, za=zq, zb=zk, zc=zs)             # S = Q K^T
        self.call("dhw_op_softmax", S.data_ptr(), B * H * Lq, Lk, H * Lq, mask.data_ptr() if mask is not None else None, scale, P.data_ptr())
        self.gemm(P, 0, Lk, 1, v.d, 0, HD, 1, o.d, 0, HD, 1, Lq, D, Lk, nzo=B, nzi=H, za=zs, zb=zk, zc=zq)             # O = P V

        def bwd():
            do = o.g
            dP = S   # the scores are dead after the softmax: reuse their buffer
            dv, av = self.into(v)
            self.gemm_group([((P, 0, 1, Lk, do, 0, HD, 1, dv, 0, HD, 1, Lk, D, Lq), dict(acc=av, nzo=B, nzi=H, za=zs, zb=zq, zc=zk)),     # dV (+)= P^T dO
                             ((do, 0, HD, 1, v.d, 0, 1, HD, dP, 0, Lk, 1, Lq, Lk, D), dict(nzo=B, nzi=H, za=zq, zb=zk, zc=zs))])          # dP = dO V^T
            self.call("dhw_op_softmax_bwd", dP.data_ptr(), P.data_ptr(), B * H * Lq, Lk, scale, dP.data_ptr())                # dS (in place)
            dq, aq = self.into(q)
            dk, ak = self.into(k)
            if dq.data_ptr() == dk.data_ptr():   # (q and k are the same tensor's gradient: the two updates of it stay ordered)
                self.gemm(dP, 0, Lk, 1, k.d, 0, HD, 1, dq, 0, HD, 1, Lq, D, Lk, acc=aq, nzo=B, nzi=H, za=zs, zb=zk, zc=zq)
                self.gemm(dP, 0, 1, Lk, q.d, 0, HD, 1, dk, 0, HD, 1, Lk, D, Lq, acc=1, nzo=B, nzi=H, za=zs, zb=zq, zc=zk)
            else:
                self.gemm_group([((dP, 0, Lk, 1, k.d, 0, HD, 1, dq, 0, HD, 1, Lq, D, Lk), dict(acc=aq, nzo=B, nzi=H, za=zs, zb=zk, zc=zq)),   # dQ (+)= dS K
                                 ((dP, 0, 1, Lk, q.d, 0, HD, 1, dk, 0, HD, 1, Lk, D, Lq), dict(acc=ak, nzo=B, nzi=H, za=zs, zb=zq, zc=zk))])  # dK (+)= dS^T Q
        self.record(o, bwd)
        return o

    def dropout(self, x: Var, keep: torch.Tensor, p: float) -> Var:
        """nn.Dropout(p) with the keep-mask supplied (1 = kept)."""
        y = Var(torch.empty_like(x.d), leaf=x.leaf)
        n = x.d.numel()
        scale = 1.0 / (1.0 - p)
        self.call("dhw_op_mask_mul", x.d.data_ptr(), keep.data_ptr(), scale, n, y.d.data_ptr(), 0)
        def bwd():
            if x.leaf:
                return
            dx, acc = self.into(x)
            self.call("dhw_op_mask_mul", y.g.data_ptr(), keep.data_ptr(), scale, n, dx.data_ptr(), acc)
        self.record(y, bwd)
        return y

    def backward(self):
        for step in reversed(self.steps):
            step()
        self.steps = []

    def mark(self, fn):
        """A position of the forward: ``fn`` runs when the backward sweep comes back to it, i.e. when every backward kernel of the ops
        recorded AFTER this point has been enqueued (the gradient-bucket markers)."""
        self.steps.append(fn)

    def record(self, out: Var, fn):
        """fn runs in the backward sweep iff a gradient reached ``out``."""
        self.steps.append(lambda: fn() if out.g is not None else None)
