"""Float64 references of ONE denoiser block from its own inputs.  TEST INFRASTRUCTURE ONLY.

Every block of the sampler hot path (reference model.py:121-182, restated in fp32 by oracle/ref_cpu.py) is stated here in
plain float64 from its definition, as a function of
  * the inputs the launch actually read (on the GPU side: the device's own taps of the producing blocks, converted to
    float64 without change), and
  * the weights as the handle holds them (``Weights``: rounded to bf16 where csrc/sampler/weights.cpp packs them in the
    handle's element type - ``upload_packed`` - and float32 where it uploads float32 - ``upload_f32`` / ``UPF``: every bias,
    the FiLM projections, the embedding, input_dense, sigma_ffn and the two heads).

Beside each exact reference stands its ROUNDING MODEL: the same arithmetic with round-to-nearest-even bf16 applied at
exactly the points where the fused kernel stores or stages bf16 (``rnd=bf16_round``; the exact reference is ``rnd=exact``).
Every ``r(...)`` below cites the kernel line it stands for.  The model exists only to size the tolerance of the GPU test
(tests/test_gpu_blocks.py): it is not a second implementation to compare bit for bit.

``mut`` (a dict, CPU tests only) switches on one WRONG variant of a block - what a subtly broken kernel would compute - so
that tests/test_block_ref_cpu.py can prove that the bound tells them apart.

Activations are channels-last [B, L, C] float64 torch tensors.  Paths below are relative to
diffusion-handwriting-generation.pytorch_amd/csrc/.
"""
from __future__ import annotations

import math

import torch

LN_EPS = 1e-6  # model.py:25, text_style.py:80
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ rounding
def exact(x: torch.Tensor) -> torch.Tensor:
    return x


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even to bfloat16 (8 significant bits, float32's exponent range, gradual underflow), on float64
    values and without passing through float32 (float64 -> float32 -> bf16 rounds twice: a value just above a bf16 tie
    would first land on the tie and then go to even)."""
    x = x.to(F64).contiguous()
    bits = x.view(torch.int64)
    drop = 45  # float64 keeps 52 stored mantissa bits, bf16 7
    lsb = (bits >> drop) & 1
    rounded = ((bits + lsb + ((1 << (drop - 1)) - 1)) >> drop) << drop   # (a carry into the exponent is the right result)
    out = rounded.view(F64).clone()
    small = x.abs() < 2.0 ** -126                                        # bf16 denormals: a fixed quantum of 2^-133
    if small.any():
        out[small] = torch.round(x[small] * 2.0 ** 133) * 2.0 ** -133    # torch.round: half to even
    big = out.abs() >= 2.0 ** 128
    if big.any():
        out[big] = torch.sign(out[big]) * math.inf
    nan = torch.isnan(x)
    if nan.any():
        out[nan] = math.nan
    return out


# ------------------------------------------------------------------------------------------------ weights
_F32_KEYS = ("input_dense.", "sigma_ffn.", "output_dense.", "pen_lifts_dense.", "text_style_model.emb.")


def packed_as_element_type(key: str) -> bool:
    """True for the tensors sampler/weights.cpp uploads with upload_packed (MFMA-fragment order, the handle's element type):
    every Conv1d / Linear WEIGHT of the ConvBlocks, EncoderLayers, skip convolutions, att_dense and the TextStyleEncoder
    (weights.cpp:222-225, 248-255, 328-338).  Everything else is float32 on every handle: biases (upload_f32,
    weights.cpp:226-229, 256-263, 324-327), the FiLM gamma/beta projections (weights.cpp:303-316), sigma_ffn, input_dense, the
    heads and the embedding (UPF, weights.cpp:318-322)."""
    if not key.endswith(".weight") or key.startswith(_F32_KEYS):
        return False
    return ".gamma_emb." not in key and ".beta_emb." not in key


class Weights:
    """state_dict (name -> fp32 array / tensor) as a handle of precision ``prec`` holds it, in float64."""

    def __init__(self, sd, prec: str = "fp32"):
        assert prec in ("fp32", "bf16")
        self.prec = prec
        self.raw = {k: torch.as_tensor(v).to(F64) for k, v in sd.items()}
        self.held = {k: (bf16_round(v) if prec == "bf16" and packed_as_element_type(k) else v) for k, v in self.raw.items()}

    def w(self, key):
        return self.held[key]

    def num_layers(self) -> int:
        n = 0
        while f"att_layers.{n}.text_dense.weight" in self.raw:
            n += 1
        return n


# ------------------------------------------------------------------------------------------------ primitives
def silu(x):
    return x / (1.0 + torch.exp(-x))


def layer_norm(x):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS)


def lin(W: Weights, name, x):
    return x @ W.w(name + ".weight").T + W.w(name + ".bias")


def film_rows(W: Weights, name, sig):
    """conditioning.py:16-19: (gamma, beta) [B,1,C] from the sigma embedding sig [B,1,32] (float32 projections: the FiLM table
    kernel evaluates them in fp32 for every handle)."""
    s = sig.reshape(sig.shape[0], 1, -1)
    return lin(W, name + ".gamma_emb", s), lin(W, name + ".beta_emb", s)


def film(W: Weights, name, x, sig, mut=None):
    g, b = film_rows(W, name, sig)
    if mut and mut.get("film_swap") and x.shape[0] > 1:   # WRONG: samples 0 and 1 read each other's FiLM row
        idx = list(range(x.shape[0]))
        idx[0], idx[1] = 1, 0
        g, b = g[idx], b[idx]
    return x * g + b


def conv3(W: Weights, name, x, mut=None):
    """Conv1d k = 3, 'same' zero padding (cnn.py:33-47) on [B,L,Cin]: out[l] = b + sum_tap w[:,:,tap] x[l-1+tap].
    mut: {"shift": 1} reads x[l+tap] (one row late); {"halo": (rows, side)} reads ZERO instead of the neighbour on `side`
    (-1 / +1) for each output row in `rows` - the row a tile would miss if its halo were one row short; {"tail": t [B,1,Cin]} reads
    t instead of zero as the row behind the last one - what a ragged tile reads when its halo row past the sample's end is not zeroed."""
    w = W.w(name + ".weight")
    B, L, _ = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1))
    if mut and "tail" in mut:
        xp = torch.cat((xp[:, :-1], mut["tail"][:, :1]), dim=1)
    off = 1 if (mut and mut.get("shift")) else 0
    if off:
        xp = torch.nn.functional.pad(xp, (0, 0, 0, off))
    out = W.w(name + ".bias").expand(B, L, -1).clone()
    for tap in range(3):
        src = xp[:, tap + off:tap + off + L]
        if mut and "halo" in mut:
            rows, side = mut["halo"]
            if tap - 1 == side:
                src = src.clone()
                src[:, rows] = 0
        out = out + src @ w[:, :, tap].T
    return out


def avg_pool(x, rnd=exact, mut=None):
    """AvgPool1d(2) (model.py:93): the side output of enc1 / enc3 / enc5's copy-out, 0.5 * (a + b) of the two STORED rows rounded
    to the element type (epilogue.h tile_copy_out_pool; enc_bc_core.h:384 for the tile enc5 hands to att_dense in LDS)."""
    B, L, C = x.shape
    if mut and mut.get("pool_off"):   # WRONG: pairs (1,2), (3,4), ...
        x = torch.cat((x[:, 1:], x[:, -1:]), dim=1)
    return rnd(0.5 * (x[:, 0::2] + x[:, 1::2]))


def upsample(x, mut=None):
    """Upsample(scale 2, nearest) (model.py:169-175): out[l] = x[l // 2]  (convblock_core.h:199, lrow >> 1)."""
    L2 = 2 * x.shape[1]
    idx = torch.arange(L2)
    idx = (idx + 1) // 2 if (mut and mut.get("up_round")) else idx // 2   # WRONG variant: (l + 1) / 2
    return x[:, idx.clamp(max=x.shape[1] - 1)]


def pos_embeddings(n: int, dim: int, pos_factor: float, args: str = "f32") -> torch.Tensor:
    """attention.py:15-23 -> [n, dim] float64, all sines then all cosines.
    args = "f32": frequency and angle evaluated in float32 exactly as the reference (and pe_table, sampler/weights.cpp:119-133,
    which builds the handle's PE.W tables) does, sine / cosine of that angle in float64 - the function the handle holds.
    args = "f64": everything in float64 (the angle reaches ~1e3 rad, where one float32 ulp is 6e-5: the two differ by that much)."""
    half = dim // 2
    c = math.log(10000) / (half - 1)
    if args == "f32":
        f = torch.exp(torch.arange(half) * -c)                      # float32, as ref_cpu.pos_embeddings
        e = (torch.arange(n)[:, None] * f[None, :] * pos_factor).to(F64)
    else:
        f = torch.exp(torch.arange(half, dtype=F64) * -c)
        e = torch.arange(n, dtype=F64)[:, None] * f[None, :] * pos_factor
    return torch.cat((e.sin(), e.cos()), dim=-1)


def pos_bias(W: Weights, wname, n, dim, pos_factor, args="f32"):
    """(x + PE) W = x W + PE W: the handle keeps PE W as a float32 per-position bias table built from the UNROUNDED float32 weight
    (pe_times_w, sampler/weights.cpp:135-146, 264-269), whatever the handle's element type."""
    t = pos_embeddings(n, dim, pos_factor, args) @ W.raw[wname + ".weight"].T
    return t.to(torch.float32).to(F64) if W.prec == "bf16" else t


def attention(q, k, v, heads, mask=None, rnd=exact, mut=None):
    """attention.py:26-46: softmax(q k^T / sqrt(depth) + mask * -1e9) v per head.  q [B,Lq,d], k / v [B,Lk,d]; mask [B,Lk] bool,
    True = padded token.  Rounding model: the probabilities enter the PV product as bf16 (attn_core.h:317 frag_from_f32 of
    exp2(s - m), un-normalised; the row sum psum is taken from the unrounded values, attn_core.h:313-315) and the division by
    the sum happens on the fp32 accumulator (enc_a_core.h:319-323, enc_bc_core.h:218-222).
    mut: {"drop_tail": KB} leaves out the last partial block of KB keys; {"unmask": True} attends padded keys;
      {"drop_key": j} leaves out key j (j < 0: from the end); {"unmask_from": j0} ignores the padding mask for keys >= j0;
      {"alias": KB} keys and values j >= KB are those of j - KB (a later key block reads the first block's staged tile);
      {"extra_key": (k_row [d], v_row [d])} one more key behind the last (a padded tile row the mask does not cut);
      {"vt_stride": (lpad, wrong)} the values are read from their transposed store [d][lpad] (zero past Lk) with row stride `wrong`."""
    m = mut or {}
    B, Lq, d = q.shape
    if "alias" in m and k.shape[1] > m["alias"]:
        kb, n = m["alias"], k.shape[1]
        k = torch.cat((k[:, :kb], k[:, :n - kb]), dim=1)
        v = torch.cat((v[:, :kb], v[:, :n - kb]), dim=1)
    if "extra_key" in m:
        k = torch.cat((k, m["extra_key"][0].expand(B, 1, d)), dim=1)
        v = torch.cat((v, m["extra_key"][1].expand(B, 1, d)), dim=1)
    if "vt_stride" in m:
        lpad, wrong = m["vt_stride"]
        vt = torch.zeros(B, d * lpad + lpad, dtype=F64)
        vt[:, :d * lpad].view(B, d, lpad)[:, :, :v.shape[1]] = v.transpose(1, 2)
        idx = torch.arange(d)[:, None] * wrong + torch.arange(v.shape[1])[None, :]
        v = vt[:, idx].transpose(1, 2)
    Lk = k.shape[1]
    D = d // heads
    qh = q.reshape(B, Lq, heads, D).transpose(1, 2)
    kh = k.reshape(B, Lk, heads, D).transpose(1, 2)
    vh = v.reshape(B, Lk, heads, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    if mask is not None and not m.get("unmask"):
        mk = mask.to(F64).clone()
        if "unmask_from" in m:
            mk[:, m["unmask_from"]:] = 0
        s = s + mk[:, None, None, :] * -1e9
    if "drop_key" in m:
        s = s.clone()
        s[..., m["drop_key"]] = -math.inf
    if m.get("drop_tail") and Lk % m["drop_tail"]:
        keep = Lk - Lk % m["drop_tail"]
        s, vh = s[..., :keep], vh[:, :, :keep]
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = (rnd(e) @ vh) / e.sum(dim=-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, Lq, d)


# ------------------------------------------------------------------------------------------------ small blocks
def sigma_ffn(W: Weights, sigma):
    """model.py:134 (utils/nn.py:145-175): float32 on every handle (misc.hip sigma_ffn kernel) -> [B,1,32]."""
    s = sigma.to(F64).reshape(-1, 1, 1)
    return lin(W, "sigma_ffn.3", silu(lin(W, "sigma_ffn.1", silu(s))))


def input_dense(W: Weights, strokes, rnd=exact):
    """model.py:139: Linear(2 -> c1) with float32 weights, stored in the element type (misc.hip input_dense kernel; fused into
    enc1's staging in the sampling loop, convblock_core.h:262)."""
    return rnd(lin(W, "input_dense", strokes))


def att_dense(W: Weights, pooled, rnd=exact):
    """model.py:100: Linear(c3 -> 2 c2) on AvgPool(enc5) (enc_bc_core.h:398-403, or the generic GEMM)."""
    return rnd(lin(W, "att_dense", pooled))


def heads(W: Weights, dec1):
    """model.py:179-182: eps = output_dense(x) [B,L,2], pen = sigmoid(pen_lifts_dense(x)) [B,L]: float32 weights on the float32
    dec1 activation (heads_core.h) - no bf16 anywhere."""
    eps = lin(W, "output_dense", dec1)
    pen = torch.sigmoid(lin(W, "pen_lifts_dense.0", dec1)).squeeze(-1)
    return eps, pen


def up_skip(W: Weights, skip_name, low, h, rnd=exact, mut=None):
    """Decoder input x = Upsample(low) + skip_conv(h) (model.py:169-175), stored in the element type: convblock_core.h:228
    round_to<T>(acc + bias + low) in the fused input stage; the same sum is the output of the stand-alone skip_conv_up GEMM."""
    return rnd(upsample(low, mut) + conv3(W, skip_name, h))


# ------------------------------------------------------------------------------------------------ ConvBlock
def conv_block(W: Weights, name, x, sig, rnd=exact, out_f32=False, up=None, mut=None):
    """cnn.py:64-87 on x [B,L,Cin] (already held in the element type), or with the decoder input stage up = (skip_name, low, h).
    Rounding points (convblock_core.h): the staged x of a decoder block :228; SiLU(x) tile :233 / :264 / :314 (silu_piece);
    h1 tile :357 (epilogue_pairs with SiLU -> H1); h2 tile :391; the stored output :480 (store_tiles<T>) - dec1 keeps fp32 (:441).
    The one-launch-per-GEMM path (sampler/denoiser.cpp:178-208) stores the same three tensors h1, h2, out.
    WRONG variants of a ragged tile (the sample ends at row n = x.shape[1]; the buffers hold other rows behind it):
      {"x_tail": t [B,2,Cin], "leak": "conv1"}  conv1 reads x row n from the buffer instead of zero (the x halo is not cut at the end);
      {"x_tail": t, "leak": "conv2"}            conv2 reads h1 row n as a tile computes it from x rows n - 1 .. n + 1, instead of zero;
      {"up_tail": (low rows [B,1,C], h rows [B,2,Ch])}   the decoder input stage evaluates x row n from the low-resolution row and
                                                the skip rows past the end, and conv1 reads it."""
    m = mut or {}
    r = rnd
    tail, leak = m.get("x_tail"), m.get("leak", "conv1")
    if up is not None:
        if "up_tail" in m:
            n = up[2].shape[1]
            xe = up_skip(W, up[0], torch.cat((up[1], m["up_tail"][0]), dim=1), torch.cat((up[2], m["up_tail"][1]), dim=1), r)
            x, tail = xe[:, :n], xe[:, n:]
        else:
            x = up_skip(W, up[0], up[1], up[2], r, m.get("up"))
    xs = r(silu(x))
    fm = m.get("film")   # (a per-sample FiLM row mix-up hits all three affines of the block: one row pointer, gam = film + b * film_bs)
    c1, c2 = m.get("conv1"), m.get("conv2")
    if tail is not None and leak == "conv1":
        c1 = dict(c1 or {}, tail=r(silu(tail[:, :1])))
    h1 = r(silu(film(W, name + ".affine1", conv3(W, name + ".conv1", xs, c1), sig, fm)))
    if tail is not None and leak == "conv2":
        h1e = r(silu(film(W, name + ".affine1", conv3(W, name + ".conv1", torch.cat((xs, r(silu(tail))), dim=1)), sig, fm)))
        c2 = dict(c2 or {}, tail=h1e[:, x.shape[1]:x.shape[1] + 1])
    h2 = r(silu(film(W, name + ".affine2", conv3(W, name + ".conv2", h1, c2), sig, fm)))
    out = film(W, name + ".affine3", lin(W, name + ".fc", h2), sig, fm) + conv3(W, name + ".conv_skip", x)
    return out if out_f32 else r(out)


# ------------------------------------------------------------------------------------------------ EncoderLayer
class LayerOut:
    def __init__(self, out, x2, x3, k1=None, v1=None):
        self.out, self.x2, self.x3, self.k1, self.v1 = out, x2, x3, k1, v1


def text_half(W: Weights, name, text, sig, rnd=exact, pe_args="f32", mut=None):
    """The text half of an EncoderLayer (model.py:38-42) -> (k1, v1) [B,Lt,d] as the layer stores them: tl = FiLM0(LN(text_dense(
    SiLU(text)))), k1 = Wk(tl + PE), v1 = Wv tl.  Rounding points: textside.hip text_layer_kernel - SiLU(text) :374, tl :404 (the LDS
    operand tile of the two projections), k1 :432, v1 :453 (both staged in the element type and copied out); the generic path
    (sampler/denoiser.cpp enc_layer_text :224-252) stores the same three tensors, with SiLU applied to the staged operand.
    mut: {"pe_clamp": True} WRONG: token Lt - 1 gets the position row of token Lt - 2 (the clamp of :431 one row early)."""
    r = rnd
    Lt = text.shape[1]
    d = W.w(name + ".mha.wk.weight").shape[0]
    tl = r(film(W, name + ".affine0", layer_norm(lin(W, name + ".text_dense", r(silu(text)))), sig))
    pb = pos_bias(W, name + ".mha.wk", Lt, d, 1.0, pe_args)
    if mut and mut.get("pe_clamp") and Lt > 1:
        pb = torch.cat((pb[:Lt - 1], pb[Lt - 2:Lt - 1]))
    k1 = r(lin(W, name + ".mha.wk", tl) + pb)
    v1 = r(lin(W, name + ".mha.wv", tl))
    return k1, v1


def encoder_layer(W: Weights, name, x, text, sig, mask, heads_n, pos_factor, rnd=exact, pe_args="f32", mut=None):
    """model.py:35-58.  x [B,Lk,d] stroke rows, text [B,Lt,2 c2] the TextStyleEncoder output, mask [B,Lt] bool (True = padded).
    Rounding points:
      text half: text_half() above - its k1 / v1 are outputs of the layer too ("<layer>.k1", "<layer>.v1");
      enc_a (enc_a_core.h): q1 :279, a1 :322-323, x2 :364, [q2 | k2 | v2] :415 / :437; probabilities attn_core.h:317;
      enc_bc (enc_bc_core.h): a2 :221-222, x3 :281, SiLU(x3) :283-284 (of the UNROUNDED x3), FFN hidden :316, out :350.
    LayerNorm statistics, FiLM and residual sums are fp32 on the accumulators (ln_rows)."""
    m = mut or {}
    r = rnd
    d = x.shape[-1]
    Lk, Lt = x.shape[1], text.shape[1]
    pf = m.get("pos_factor", pos_factor)   # WRONG variant: another layer's factor
    k1, v1 = text_half(W, name, text, sig, r, pe_args, m.get("text"))
    q1 = r(lin(W, name + ".mha.wq", x) + pos_bias(W, name + ".mha.wq", Lk, d, pf, pe_args))
    a1 = r(attention(q1, k1, v1, heads_n, mask, r, m.get("cross")))
    x2 = r(film(W, name + ".affine1", layer_norm(lin(W, name + ".mha.dense", a1)), sig) + x)
    q2 = r(lin(W, name + ".mha2.wq", x2) + pos_bias(W, name + ".mha2.wq", Lk, d, pf, pe_args))
    k2 = r(lin(W, name + ".mha2.wk", x2) + pos_bias(W, name + ".mha2.wk", Lk, d, pf, pe_args))
    v2 = r(lin(W, name + ".mha2.wv", x2))
    a2 = r(attention(q2, k2, v2, heads_n, None, r, m.get("self")))
    x3u = film(W, name + ".affine2", layer_norm(x2 + lin(W, name + ".mha2.dense", a2)), sig)
    x3 = r(x3u)
    f = r(silu(lin(W, name + ".ffn.1", r(silu(x3u)))))
    out = r(film(W, name + ".affine3", layer_norm(lin(W, name + ".ffn.3", f) + x3), sig))
    return LayerOut(out, x2, x3, k1, v1)


# ------------------------------------------------------------------------------------------------ TextStyleEncoder
class TextOut:
    def __init__(self, out, style, t2):
        self.out, self.style, self.t2 = out, style, t2


def text_style_encoder(W: Weights, text, style, sig, rnd=exact, mut=None):
    """text_style.py:91-104 (eval) from the call's own inputs: token ids [B,Lt] and the float32 style vector [B,S,1280].
    Rounding points: the style cast (misc.hip cast kernel), SiLU(style) operand / hidden layer / LayerNorm output of the two
    style GEMMs and the embedding LayerNorm (sampler/denoiser.cpp:420-441: each a stored activation); then textside.hip
    text_style_kernel: s and t1 :125-126 (stage_film_384), V^T :183, K :199, q :211, the attention output :232, t1 again as the
    residual :257, t2 :270, SiLU of the rounded t2 :272-273, the FFN hidden layer :300, out :320.
    mut (WRONG variants of the style attention, attn_once's mask :48 and the zero fill of V^T :183 / of the staged rows :114):
      {"drop_last_key": True} key S5 - 1 is masked away; {"unmasked_pad": True} key S5 - a zero-filled style row, so K is the
      projection's bias and V is 0 - takes part in the softmax."""
    r = rnd
    n = "text_style_model"
    B, S, C = style.shape
    st = r(style.to(F64).reshape(B, S * 5, C // 5))   # reshape_up(., 5), utils/nn.py:115-127
    hid = r(silu(lin(W, n + ".style_ffn.1", r(silu(st)))))
    s = r(film(W, n + ".affine1", r(layer_norm(lin(W, n + ".style_ffn.3", hid))), sig))
    t1 = r(film(W, n + ".affine2", r(layer_norm(W.w(n + ".emb.weight")[text.long()])), sig))
    q = r(lin(W, n + ".mha.wq", t1))
    k = r(lin(W, n + ".mha.wk", s))
    v = r(lin(W, n + ".mha.wv", s))
    am = None
    if mut and mut.get("drop_last_key"):
        am = {"drop_key": -1}
    elif mut and mut.get("unmasked_pad"):
        am = {"extra_key": (r(W.w(n + ".mha.wk.bias")), torch.zeros(q.shape[-1], dtype=F64))}
    mh = r(attention(q, k, v, 8, None, r, am))
    t2 = r(film(W, n + ".affine3", layer_norm(t1 + lin(W, n + ".mha.dense", mh)), sig))
    hid2 = r(silu(lin(W, n + ".text_ffn.1", r(silu(t2)))))
    out = r(film(W, n + ".affine4", layer_norm(lin(W, n + ".text_ffn.3", hid2)), sig))
    return TextOut(out, s, t2)


# ------------------------------------------------------------------------------------------------ the launch sequence, block by block
LAYER_GEOM = {"enc3": (3, 4.0), "enc5": (4, 2.0)}   # heads, pos_factor (model.py:88-90); att_layers.*: (6, 1.0) (model.py:104-109)


def layer_geom(name):
    return LAYER_GEOM.get(name, (6, 1.0))


def block_names(num_layers: int):
    return (["sigma_ffn", "text_style_model", "input_dense", "enc1", "enc1.pool", "enc2", "enc3", "enc3.pool", "enc4", "enc5",
             "enc5.pool", "att_dense"] + [f"att_layers.{i}" for i in range(num_layers)] + ["dec3", "dec2", "dec1", "heads"])


def block_output(W: Weights, name, get, inputs, rnd=exact, fused_up=True, pe_args="f32", mut=None):
    """Output(s) of block `name` as {tap name: tensor}, from its OWN inputs: get(tap) returns the stored output of a producing
    block (float64, unchanged), inputs = dict(strokes, text, sigma, style).  fused_up: the decoder blocks evaluate
    Upsample + skip_conv themselves (one reference spans both); otherwise "skip_convK+up" is a block of its own."""
    nl = W.num_layers()
    text = inputs["text"]
    mask = text == 0
    sig = None if name == "sigma_ffn" else get("sigma_ffn")
    if name == "sigma_ffn":
        return {name: sigma_ffn(W, inputs["sigma"])}
    if name == "text_style_model":
        o = text_style_encoder(W, text, inputs["style"], sig, rnd, mut)
        return {name: o.out, name + ".style": o.style, name + ".t2": o.t2}
    if name == "input_dense":
        return {name: input_dense(W, inputs["strokes"].to(F64), rnd)}
    if name.endswith(".pool"):
        return {name: avg_pool(get(name[:-5]), rnd, mut)}
    if name in ("enc1", "enc2", "enc4"):
        src = {"enc1": "input_dense", "enc2": "enc1.pool", "enc4": "enc3.pool"}[name]
        return {name: conv_block(W, name, get(src), sig, rnd, mut=mut)}
    if name in ("enc3", "enc5") or name.startswith("att_layers."):
        if name.startswith("att_layers."):
            i = int(name.split(".")[1])
            src = "att_dense" if i == 0 else f"att_layers.{i - 1}"
        else:
            src = {"enc3": "enc2", "enc5": "enc4"}[name]
        hn, pf = layer_geom(name)
        o = encoder_layer(W, name, get(src), get("text_style_model"), sig, mask, hn, pf, rnd, pe_args, mut)
        return {name: o.out, name + ".x2": o.x2, name + ".x3": o.x3, name + ".k1": o.k1, name + ".v1": o.v1}
    if name == "att_dense":
        return {name: att_dense(W, get("enc5.pool"), rnd)}
    dec = {"dec3": ("skip_conv3", f"att_layers.{nl - 1}" if nl else "att_dense", "enc5"), "dec2": ("skip_conv2", "dec3", "enc3"),
           "dec1": ("skip_conv1", "dec2", "enc1")}
    if name in dec:
        sk, low, h = dec[name]
        if fused_up:
            return {name: conv_block(W, name, None, sig, rnd, out_f32=name == "dec1", up=(sk, get(low), get(h)), mut=mut)}
        return {name: conv_block(W, name, get(sk + "+up"), sig, rnd, out_f32=name == "dec1", mut=mut)}
    if name.endswith("+up"):
        sk = name[:-3]
        _, low, h = {v[0]: v for v in dec.values()}[sk]
        return {name: up_skip(W, sk, get(low), get(h), rnd, mut)}
    if name == "heads":
        eps, pen = heads(W, get("dec1"))
        return {"eps": eps, "pen": pen}
    raise KeyError(name)


def forward_taps(W: Weights, inputs, rnd=exact, pe_args="f32"):
    """Every block in launch order, each fed with the previous blocks' outputs: the reference's own taps (and, with
    rnd = bf16_round, stand-ins for the device's taps at the same shapes)."""
    taps = {}
    for name in block_names(W.num_layers()):
        taps.update(block_output(W, name, taps.__getitem__, inputs, rnd, True, pe_args))
    return taps


# ------------------------------------------------------------------------------------------------ error measures
ROW_FLOOR = 1e-3   # rows whose norm is below this share of the block's largest row norm are measured against that floor


def row_error(got, ref):
    """(worst per-row relative L2 error over channels, share of rows measured against the floor)."""
    cols = ref.shape[-1] if ref.dim() > 1 else 1   # (a vector such as pen [B*L]: one value per row)
    got = got.reshape(-1, cols)
    ref = ref.reshape(-1, cols)
    nrm = ref.norm(dim=-1)
    floor = ROW_FLOOR * nrm.max()
    err = (got - ref).norm(dim=-1) / torch.maximum(nrm, floor)
    return err.max().item(), (nrm < floor).double().mean().item()


def max_error(got, ref):
    """max |got - ref| / max |ref|."""
    return ((got - ref).abs().max() / ref.abs().max()).item()
