"""The network: ``TrainModel`` — the parameters in flat buffers laid out by gradient bucket, the FiLM table, and the reference's
modules as chains of ``Tape`` ops."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from .tape import Tape, Var, _ViewVar

# DHW_TRAIN_FILM_RIDER=0: a ConvBlock's affine (+ SiLU) (+ conv_skip) as its own pass behind the GEMM again instead of a further output of the GEMM (A/B)
FILM_RIDER = os.environ.get("DHW_TRAIN_FILM_RIDER", "1") != "0"

# Gradient buckets, in the order the backward sweep completes them (TrainModel lays the flat buffers out in this order, so a
# bucket is ONE contiguous range = one all-reduce):
#   0  decoder ConvBlocks + skip convolutions          final once the sweep is back at the end of the bottleneck layers
#   1  bottleneck EncoderLayers + att_dense            ... at the end of enc5
#   2  encoder ConvBlocks / EncoderLayers + input_dense ... in front of input_dense
#   3  text side (TextStyleEncoder, every layer's text_dense: evaluated once, first, for all layers) + all FiLM Linears (their
#      gradient is ONE kernel over the whole [B, 2 x 9280] table, the last but two of the sweep)
#   4  sigma MLP (the first module of the forward) + the two heads' odd-sized tensors (kept last so that every other tensor starts
#      16-byte aligned: the GEMMs take the 16-byte-load forms and film_table reads weight rows as f32x4)
N_BUCKETS = 5


def grad_bucket(name: str) -> int:
    if name.startswith(("sigma_ffn.", "output_dense.", "pen_lifts_dense.")):
        return 4
    if ".gamma_emb." in name or ".beta_emb." in name or name.startswith("text_style_model.") or ".text_dense." in name:
        return 3
    if name.startswith(("dec1.", "dec2.", "dec3.", "skip_conv")):
        return 0
    if name.startswith(("att_layers.", "att_dense.")):
        return 1
    if name.startswith(("enc1.", "enc2.", "enc3.", "enc4.", "enc5.", "input_dense.")):
        return 2
    raise ValueError(f"no gradient bucket rule for parameter {name}")


def positional_encoding(length: int, dim: int, pos_factor: float) -> torch.Tensor:
    """PosEmbeddings.forward(arange(length)) (attention.py:14-23) -> [length, dim] on the host (a constant table)."""
    half = dim // 2
    freq = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    e = torch.arange(length)[:, None] * freq[None, :] * pos_factor
    return torch.cat((e.sin(), e.cos()), dim=-1).float()

class TrainModel:
    """``DiffusionModel`` (model.py:61-199) for training: parameters as fp32 device tensors under the reference's names."""

    STYLE_DROP = 0.3   # text_style.py:88

    def __init__(self, state_dict: dict, num_layers: int = 2, device=None, drop_rate: float = 0.0, seed: int = 0, precision: str = "fp32"):
        """``drop_rate``: the EncoderLayers' dropout (model.py:23; configs/best.yml trains with 0.0, the class default is 0.1).
        ``precision``: "fp32" — exact-f32 MFMA everywhere, the mode the gradient fixtures pin — or "bf16": mixed precision, every
        GEMM (Linear / Conv1d / attention, forward and backward) contracts bf16-rounded operands with fp32 accumulation; weights,
        activations in memory, gradients, optimizer state and all non-GEMM arithmetic stay fp32 — with one exception: a bias
        gradient is summed inside its layer's weight-gradient GEMM from the bf16-rounded dy tile (dhw_gemm_desc.rowsum), so it
        carries the same operand rounding as that weight gradient (tests: the bf16 cases of the GEMM sweep)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        self.precision = precision
        if not 0.0 <= drop_rate < 1.0:
            raise ValueError("drop_rate must be in [0, 1)")
        if not torch.cuda.is_available():
            raise RuntimeError("TrainModel needs the MI355X: the training step has no CPU path")
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.num_layers, self.drop_rate = num_layers, float(drop_rate)
        # {seed, draw index} of the device generator behind the dropout masks (and GraphedTrainStep's eps draw)
        self.seed = seed
        self.rng = torch.tensor([seed, 0], dtype=torch.int64, device=self.dev)
        self._masks, self._site = None, 3
        self.names = list(state_dict.keys())
        shapes = {k: tuple(np.shape(v)) for k, v in state_dict.items()}
        # Conv1d weights [Cout, Cin, 3] are kept as [tap][Cout][Cin] in the flat buffers (unit stride along Cin: the weight is then
        # the 16-byte-load operand of the forward, data-gradient and weight-gradient GEMMs alike; in torch's layout it was a stride-3
        # gather / scatter).  Their named views are the permuted views, so shapes and values are the reference's everywhere.
        conv_w = {k for k in shapes if len(shapes[k]) == 3 and shapes[k][2] == 3}
        host = {}
        for k, v in state_dict.items():
            h = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().to("cpu", torch.float32)
            host[k] = (h.permute(2, 0, 1).contiguous() if k in conv_w else h).reshape(-1)
        # ONE flat fp32 buffer for all parameters and one for all gradients (40 MB each): a single memset clears the
        # gradients, a single kernel pair clips and applies Adam.  The tensors sit in it in the order the backward sweep COMPLETES
        # their gradients (grad_bucket; state_dict order inside a bucket, odd-sized tensors last), so each of the N_BUCKETS
        # gradient buckets is one contiguous range that can be all-reduced the moment its marker fires (GradBucketReducer).
        # self.names / state_dict() stay in the reference's order: the layout is private to the flat buffers.
        self.layout = sorted(self.names, key=lambda k: (grad_bucket(k), host[k].numel() % 4 != 0))   # (stable: state_dict order otherwise)
        self.flat = torch.cat([host[k] for k in self.layout]).to(self.dev)
        self.flat_grad = torch.zeros_like(self.flat)
        self.p, self.offset, off = {}, {}, 0
        self.bucket_ranges, self.bucket_hook = [], None     # [start, end) of each bucket; bucket_hook(i): called when bucket i < N_BUCKETS - 1 is final
        for b in range(N_BUCKETS):
            n_b = sum(host[k].numel() for k in self.layout if grad_bucket(k) == b)
            start = self.bucket_ranges[-1][1] if self.bucket_ranges else 0
            self.bucket_ranges.append((start, start + n_b))
        self._shapes, self._conv_w = shapes, conv_w
        self.sizes = {k: host[k].numel() for k in self.layout}     # elements per tensor; with self.layout, the whole layout of a flat buffer
        for k in self.layout:
            n = self.sizes[k]
            if off % 4 and n % 4 == 0:
                raise ValueError(f"parameter {k} would start unaligned in the flat buffer (an odd-sized tensor precedes it)")
            self.offset[k] = off
            v = Var(self._view(self.flat, k))
            v.g = self._view(self.flat_grad, k)
            self.p[k] = v
            off += n
        # every AffineTransformLayer's gamma / beta Linear as columns of one [B, TOT] table (dhw_op_film_table): column ->
        # (weight row, bias) offsets inside the flat buffer; film_cols[name] = (first gamma column, first beta column)
        woff, boff, self.film_cols, col = [], [], {}, 0
        for k in self.names:
            if k.endswith(".gamma_emb.weight"):
                base, Cc = k[:-len(".gamma_emb.weight")], shapes[k][0]
                if shapes[k][1] != 32:
                    raise ValueError("the FiLM Linears take the 32-wide sigma embedding")
                self.film_cols[base] = (col, col + Cc)
                for kind in ("gamma_emb", "beta_emb"):
                    woff.append(self.offset[f"{base}.{kind}.weight"] + 32 * torch.arange(Cc, dtype=torch.int64))
                    boff.append(self.offset[f"{base}.{kind}.bias"] + torch.arange(Cc, dtype=torch.int64))
                col += 2 * Cc
        self.film_total = col
        woff_all = torch.cat(woff)
        if bool((woff_all % 4 != 0).any()):   # film_table_fwd_kernel reads each 32-float weight row as f32x4 from flat + offset
            raise ValueError("the FiLM weight rows are not 16-byte aligned in the flat parameter buffer (unexpected state_dict sizes / order)")
        self.film_woff, self.film_boff = woff_all.to(self.dev), torch.cat(boff).to(self.dev)
        self.c1 = self.p["input_dense.weight"].d.shape[0]
        self.style_drop = self.STYLE_DROP   # (0.0 = the TextStyleEncoder's Dropout in eval mode: dhg_amd.DiffusionModel's differentiable forward)
        self._pe = {}
        self.tape = None

    # ---- parameters ------------------------------------------------------------------------------------------------------
    def parameters(self):
        """The flat parameter buffer (every named parameter is a view into it, in state_dict order; Conv1d weights as
        [tap][Cout][Cin], their named views permuted back to [Cout, Cin, 3])."""
        return [self.flat]

    def grads(self):
        return [self.flat_grad]

    def zero_grad(self):
        self.flat_grad.zero_()   # one memset

    def _view(self, buf, k):
        """Tensor ``k`` inside a flat buffer laid out like ``self.flat``, in the reference's shape (a Conv1d weight: the permuted view
        of its [tap][Cout][Cin] storage) — the one statement of the layout rule."""
        piece = buf[self.offset[k]:self.offset[k] + self.sizes[k]]
        return piece.view(3, *self._shapes[k][:2]).permute(1, 2, 0) if k in self._conv_w else piece.view(self._shapes[k])

    def named_views(self, buf) -> dict:
        """The named, reference-ordered views of any flat buffer laid out like ``self.flat`` (the gradients, Adam's moments, an EMA
        of the weights): what ``state_dict`` gives for the parameters themselves."""
        if buf.dim() != 1 or buf.numel() != self.flat.numel():
            raise ValueError(f"a flat buffer of this model holds {self.flat.numel()} elements, got shape {tuple(buf.shape)}")
        return {k: self._view(buf, k) for k in self.names}

    def state_dict(self):
        return self.named_views(self.flat)

    def ema_state_dict(self, opt):
        """The state_dict of the averaged weights ``opt`` keeps for this model (``Adam(model.parameters(), ema_decay=...)``)."""
        if getattr(opt, "ema", None) is None:
            raise ValueError("this optimizer keeps no EMA (ema_decay=None)")
        return self.named_views(opt.ema[0])

    def pe(self, L, dim, factor):
        key = (L, dim, factor)
        if key not in self._pe:
            self._pe[key] = positional_encoding(L, dim, factor).to(self.dev)
        return self._pe[key]

    def prepare_tables(self, L: int, Lt: int):
        """Upload the positional-encoding tables a (L, Lt) batch needs (model.py:40-44) ahead of a graph capture."""
        c2, c3 = self.p["enc3.text_dense.weight"].d.shape[0], self.p["enc5.text_dense.weight"].d.shape[0]
        for d, Lx, f in ((c2, L // 2, 4), (c3, L // 4, 2), (2 * c2, L // 8, 1)):
            self.pe(Lx, d, f)
            self.pe(Lt, d, 1.0)

    # ---- modules ---------------------------------------------------------------------------------------------------------
    def _lin(self, t, x, name, addend=None, silu_out=False):
        return t.linear(x, self.p[name + ".weight"], self.p.get(name + ".bias"), addend, silu_out)

    def _ffn(self, t, x, name, addend=None, x_act=None):
        """ff_network (utils/nn.py:145-175): SiLU -> Linear -> SiLU -> Linear (+ the residual that follows it, in the last GEMM).
        ``x_act``: SiLU(x) where the pass that produced x wrote it already; the inner SiLU comes out of the first GEMM's pass."""
        _, ha = self._lin(t, x_act if x_act is not None else t.silu(x), name + ".1", silu_out=True)
        return self._lin(t, ha, name + ".3", addend)

    def _film_table(self, t, sigma, B):
        """gamma / beta of all AffineTransformLayers for this sigma: one launch forward, two backward (instead of 76 small
        GEMMs forward and 228 GEMM / bias-sum launches backward)."""
        table = Var(t.new(B, self.film_total))
        args = (self.flat.data_ptr(), self.film_woff.data_ptr(), self.film_boff.data_ptr(), B, self.film_total)
        t.call("dhw_op_film_table", sigma.d.data_ptr(), *args, table.d.data_ptr())
        t.record(table, lambda: t.call("dhw_op_film_table_bwd", table.g.data_ptr(), sigma.d.data_ptr(), *args, self.flat_grad.data_ptr(),
                                       sigma.grad().data_ptr()))
        self._film = table

    def _ln_affine(self, t, x, name, B, addend=None, silu_out=False, pe=None):
        """affine(layernorm(x)) (+ addend) as one fused pass (LN statistics span at most 512 channels here)."""
        return t.ln_film_cols(x, self._film, *self.film_cols[name], B, addend, silu_out, pe)

    def _mha(self, t, q, k, v, name, B, H, mask=None, addend=None):
        qp, kp, vp = t.linear_group([(x, self.p[f"{name}.{w}.weight"], self.p[f"{name}.{w}.bias"]) for x, w in ((q, "wq"), (k, "wk"), (v, "wv"))])
        return self._lin(t, t.attention(qp, kp, vp, B, H, mask), name + ".dense", addend)

    def _convblock(self, t, x, name, B, L, x_act=None):
        """cnn.py:64-87.  ``x_act``: SiLU(x) where the pass that produced x wrote it already.  Every affine (+ SiLU) (+ conv_skip)
        rides on the output pass of the GEMM in front of it (dhw_gemm_desc.film_out), or follows it as its own pass (FILM_RIDER off)."""
        film = lambda k, act, addend=None: (self._film, *self.film_cols[f"{name}.affine{k}"], B, act, addend)   # noqa: E731
        conv = lambda v, n, defer=None, fl=None: t.conv3(v, self.p[f"{name}.{n}.weight"], self.p[f"{name}.{n}.bias"], L, defer=defer, film=fl)   # noqa: E731
        ride = lambda fl: fl if FILM_RIDER else None                          # noqa: E731
        own = lambda y, fl: y if FILM_RIDER else t.film_cols(y, *fl)          # noqa: E731
        xa = x_act if x_act is not None else t.silu(x)
        both = []                      # conv_skip(x) and conv1(SiLU(x)) are independent: one launch
        skip, h = conv(x, "conv_skip", both), conv(xa, "conv1", both, ride(film(1, True)))
        if both:
            t.gemm_group(both)
        h = own(h, film(1, True))                                                           # SiLU(affine1(conv1(.)))
        h = own(conv(h, "conv2", None, ride(film(2, True))), film(2, True))                 # SiLU(affine2(conv2(.)))
        fc = t.linear(h, self.p[name + ".fc.weight"], self.p[name + ".fc.bias"], film=ride(film(3, False, skip)))
        return own(fc, film(3, False, skip))                                                # affine3(fc(h)) + conv_skip(x)

    def _drop(self, t, v, B):
        """EncoderLayer.drop (model.py:23): identity at rate 0; otherwise the next caller-supplied keep-mask (parity tests) or a
        mask drawn on the device for this site of this update."""
        if self.drop_rate == 0.0:
            return v
        if self._masks is not None:
            keep = next(self._masks).to(self.dev, torch.float32).contiguous().view_as(v.d)
        else:
            keep = torch.empty_like(v.d)
            t.call("dhw_op_keep_mask", self.rng.data_ptr(), self._site, v.d.numel(), v.d.numel() // B, self.drop_rate, keep.data_ptr())
        self._site += 1
        return t.dropout(v, keep, self.drop_rate)

    def _encoder(self, t, x, text, mask, name, B, H, pos_factor, td=None):
        """EncoderLayer.forward (model.py:36-58); ``text`` is SiLU(text features) already; ``td``: text_dense(text) where the
        caller has evaluated it (all layers' text_dense in one launch: they share their input)."""
        d = x.d.shape[1]
        Lx, Lt = x.d.shape[0] // B, text.d.shape[0] // B
        tx, text_pe = self._ln_affine(t, td if td is not None else self._lin(t, text, name + ".text_dense"), name + ".affine0", B, pe=self.pe(Lt, d, 1.0))   # text: SiLU(text features), shared
        x_pe = t.add_rows(x, self.pe(Lx, d, pos_factor), B)
        x2 = self._mha(t, x_pe, text_pe, tx, name + ".mha", B, H, mask)
        # the residual adds and the positional-encoding adds ride on the passes / GEMMs around them
        x2, x2_pe = self._ln_affine(t, self._drop(t, x2, B), name + ".affine1", B, addend=x, pe=self.pe(Lx, d, pos_factor))
        if self.drop_rate == 0.0:
            x3, x3a = self._ln_affine(t, self._mha(t, x2_pe, x2_pe, x2, name + ".mha2", B, H, addend=x2), name + ".affine2", B, silu_out=True)
            x4 = self._ffn(t, x3, name + ".ffn", addend=x3, x_act=x3a)
        else:       # (the dropout sits between the GEMM and the add)
            x3 = self._mha(t, x2_pe, x2_pe, x2, name + ".mha2", B, H)
            x3, x3a = self._ln_affine(t, t.add(x2, self._drop(t, x3, B)), name + ".affine2", B, silu_out=True)
            x4 = t.add(self._drop(t, self._ffn(t, x3, name + ".ffn", x_act=x3a), B), x3)
        return self._ln_affine(t, x4, name + ".affine3", B)

    def _text_style(self, t, ids, style, keep, B):
        """TextStyleEncoder.forward (text_style.py:96-110)."""
        n = "text_style_model"
        S = style.d.shape[1]
        st = t.dropout(style, keep, self.style_drop)                          # [B, S, 1280]
        up = _ViewVar(st, (B * S * 5, st.d.shape[2] // 5))                      # reshape_up(., 5): a pure view of the same rows
        stf = self._ffn(t, up, n + ".style_ffn")
        stf = self._ln_affine(t, stf, n + ".affine1", B)
        tx = t.embedding(ids, self.p[n + ".emb.weight"])
        tx = self._ln_affine(t, tx, n + ".affine2", B)
        tx, txa = self._ln_affine(t, self._mha(t, tx, stf, stf, n + ".mha", B, 8, addend=tx), n + ".affine3", B, silu_out=True)
        return self._ln_affine(t, self._ffn(t, tx, n + ".text_ffn", x_act=txa), n + ".affine4", B)

    # ---- forward / backward ----------------------------------------------------------------------------------------------
    def check_tokens(self, text: torch.Tensor):
        if text.is_cuda:
            raise ValueError("token ids are validated on the host: pass a CPU tensor")
        if int(text.min()) < 0 or int(text.max()) >= self.p["text_style_model.emb.weight"].d.shape[0]:
            raise ValueError("token id out of the embedding's range")

    def forward(self, strokes: torch.Tensor, text: torch.Tensor, sigma: torch.Tensor, style: torch.Tensor, style_keep: torch.Tensor | None = None,
                drop_masks=None):
        """strokes [B, L, 2], text int64 [B, Lt] (host), sigma [B, 1] (= sqrt(abar), train.py:49), style [B, S, 1280];
        ``style_keep``: the Dropout(0.3) keep-mask [B, S, 1280] (drawn here when omitted); ``drop_masks``: with drop_rate > 0,
        the EncoderLayers' keep-masks in call order (3 per layer: enc3, enc5, att_layers...), else drawn on the device.
        -> (score [B, L, 2], pen [B, L])."""
        dev = self.dev
        self._masks = iter(drop_masks) if drop_masks is not None else None
        f = lambda a: a.to(dev, torch.float32).contiguous()   # noqa: E731
        self.check_tokens(text)
        mask = (text == 0).to(torch.float32).to(dev).contiguous()          # create_padding_mask (utils/nn.py:189), host side
        if style_keep is None:
            style_keep = (torch.rand(style.shape) >= self.style_drop).float()
        return self.forward_device(f(strokes), text.to(dev, torch.int64).contiguous(), mask, f(sigma), f(style), f(style_keep))

    def forward_device(self, strokes, ids, mask, sigma, style, keep):
        """``forward`` on device-resident fp32 inputs (ids int64, mask = 1 at padding): kernel launches only."""
        dev = self.dev
        B, L, _ = strokes.shape
        if L % 8:
            raise ValueError("the stroke length must be a multiple of 8 (three AvgPool1d(2) stages)")
        t = self.tape = Tape(dev, bf16=self.precision == "bf16")
        self._site = 3
        x_in, sig_in, sty = Var(strokes.view(B * L, 2), leaf=True), Var(sigma.view(B, 1), leaf=True), Var(style, leaf=True)

        sigma_v = self._ffn(t, sig_in, "sigma_ffn")                                     # [B, 32]
        t.mark(lambda: self._bucket_done(3))       # the sweep is back here: text side, text_dense and the FiLM table are done
        self._film_table(t, sigma_v, B)
        txt = t.silu(self._text_style(t, ids, sty, keep, B))                  # SiLU([B*Lt, 2 c2]): every EncoderLayer's text_dense starts
                                                                                       # with it (model.py:38) — once, not once per layer
        # every EncoderLayer's text_dense (model.py:38) reads the same SiLU(text features): one launch for all of them
        enc_names = ["enc3", "enc5"] + [f"att_layers.{i}" for i in range(self.num_layers)]
        td = dict(zip(enc_names, t.linear_group([(txt, self.p[n + ".text_dense.weight"], self.p[n + ".text_dense.bias"]) for n in enc_names])))
        t.mark(lambda: self._bucket_done(2))       # ... encoder + input_dense done
        x, xa = self._lin(t, x_in, "input_dense", silu_out=True)
        h1 = self._convblock(t, x, "enc1", B, L, x_act=xa)
        h2 = self._convblock(t, t.resample(0, h1), "enc2", B, L // 2)
        h2 = self._encoder(t, h2, txt, mask, "enc3", B, 3, 4, td=td["enc3"])
        h3 = self._convblock(t, t.resample(0, h2), "enc4", B, L // 4)
        h3 = self._encoder(t, h3, txt, mask, "enc5", B, 4, 2, td=td["enc5"])
        t.mark(lambda: self._bucket_done(1))       # ... att_dense + bottleneck layers done
        x = self._lin(t, t.resample(0, h3), "att_dense")
        for i in range(self.num_layers):
            x = self._encoder(t, x, txt, mask, f"att_layers.{i}", B, 6, 1, td=td[f"att_layers.{i}"])
        t.mark(lambda: self._bucket_done(0))       # ... decoder + skip convolutions done
        # upsample(x) + skip_conv(h): the add rides on the skip convolution's output pass
        # (and SiLU of the sum, which the decoder block's conv1 starts with, is its second output)
        for i, h, Lr in ((3, h3, L // 4), (2, h2, L // 2), (1, h1, L)):
            x, xa = t.conv3(h, self.p[f"skip_conv{i}.weight"], self.p[f"skip_conv{i}.bias"], Lr, addend=t.resample(2, x), silu_out=True)
            x = self._convblock(t, x, f"dec{i}", B, Lr, x_act=xa)
        self._score = self._lin(t, x, "output_dense")
        self._pen = t.sigmoid(self._lin(t, x, "pen_lifts_dense.0"))
        return self._score.d.view(B, L, 2), self._pen.d.view(B, L)

    def _bucket_done(self, i: int):
        if self.bucket_hook is not None:
            self.bucket_hook(i)

    def backward(self, d_score: torch.Tensor, d_pen: torch.Tensor):
        """Accumulate every parameter gradient for the upstream gradients of the two outputs.  ``self.bucket_hook(i)`` (if set) is
        called from inside the sweep as soon as gradient bucket i = 0 .. N_BUCKETS - 2 is final; the last bucket is final on return."""
        self._score.g = d_score.contiguous().view_as(self._score.d)
        self._pen.g = d_pen.contiguous().view_as(self._pen.d)
        self.tape.backward()
        self.last_launches, self.last_gemm_flops = self.tape.launches, self.tape.flops
        self.tape = None
