"""CPU yardstick of the attention maps (include/dhw.h dhw_attention, rules 2-4), built on ``oracle.ref_cpu.forward``'s taps.
TEST INFRASTRUCTURE ONLY.  tests/test_align_cpu.py proves it first: its probabilities, pushed through the rest of the layer,
reproduce the oracle's own ``<layer>.x2`` tap."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu

HEADS = {"enc3": 3, "enc5": 4}          # att_layers.*: 6
POS_FACTOR = {"enc3": 4, "enc5": 2}     # att_layers.*: 1
SHIFT = {"enc3": 1, "enc5": 2}          # att_layers.*: 3


def layer_names(num_layers: int) -> list:
    return ["enc3", "enc5"] + [f"att_layers.{i}" for i in range(num_layers)]


def input_tap(name: str) -> str:
    """The tap that holds the layer's input."""
    if name == "enc3":
        return "enc2"
    if name == "enc5":
        return "enc4"
    i = int(name.split(".")[1])
    return "att_dense" if i == 0 else f"att_layers.{i - 1}"


def head_mean(P: torch.Tensor) -> torch.Tensor:
    """Rule 3: (((P0 + P1) + P2) + ...) * (1/H) in fp32, head order.  P [B,H,Lq,Lt]."""
    P = P.float()
    acc = P[:, 0].clone()
    for h in range(1, P.shape[1]):
        acc = acc + P[:, h]
    return acc * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(P.shape[1]), dtype=torch.float32))


def first_argmax(mean: torch.Tensor) -> torch.Tensor:
    """Rule 3: the smallest k at which mean[b,q,:] is largest, int32."""
    return torch.from_numpy(np.argmax(mean.numpy(), axis=-1).astype(np.int32))


def _uniform(sd, strokes, text, sigma, style, name):
    taps = {}
    with torch.no_grad():
        ref_cpu.forward(sd, strokes, text, sigma.reshape(-1, 1), style, taps=taps)
        x = taps[input_tap(name)]
        sig = taps["sigma_ffn"]
        heads, pf = HEADS.get(name, 6), POS_FACTOR.get(name, 1.0)
        b, n, d = x.shape
        depth = d // heads
        t = ref_cpu._lin(sd, name + ".text_dense", F.silu(taps["text_style_model"]))
        t = ref_cpu.film(sd, name + ".affine0", ref_cpu._ln(t), sig)
        q = ref_cpu._lin(sd, name + ".mha.wq", x + ref_cpu.pos_embeddings(n, d, pf))
        k = ref_cpu._lin(sd, name + ".mha.wk", t + ref_cpu.pos_embeddings(t.shape[1], d, 1.0))
        v = ref_cpu._lin(sd, name + ".mha.wv", t)
        qh = q.view(b, n, heads, depth).transpose(1, 2)
        kh = k.view(b, -1, heads, depth).transpose(1, 2)
        vh = v.view(b, -1, heads, depth).transpose(1, 2)
        mask = torch.eq(text.long(), 0).float()[:, None, None, :]
        logits = qh @ kh.transpose(-1, -2) / math.sqrt(depth) + mask * -1e9
        P = torch.softmax(logits, dim=-1)
        # the rest of the cross-attention half of the layer, from these probabilities (model.py:46-48)
        o = (P @ vh).transpose(1, 2).reshape(b, n, d)
        x2 = ref_cpu.film(sd, name + ".affine1", ref_cpu._ln(ref_cpu._lin(sd, name + ".mha.dense", o)), sig) + x
    return P, x2, taps[name + ".x2"]


def attention(sd, strokes, text, sigma, style, name, lengths=None) -> dict:
    """probs [B,H,Lq,Lt], mean [B,Lq,Lt], token [B,Lq] int32 of layer ``name``; with ``lengths`` every sample runs alone at
    its own length and rows past it are 0 / -1 (rule 4).  Also x2 / x2_tap of the uniform run (the helper's own proof)."""
    if lengths is None:
        P, x2, x2_tap = _uniform(sd, strokes, text, sigma, style, name)
        mean = head_mean(P)
        return dict(probs=P, mean=mean, token=first_argmax(mean), x2=x2, x2_tap=x2_tap)
    B, L = strokes.shape[:2]
    sh = SHIFT.get(name, 3)
    heads, Lt = HEADS.get(name, 6), text.shape[1]
    P = torch.zeros((B, heads, L >> sh, Lt))
    mean = torch.zeros((B, L >> sh, Lt))
    token = torch.full((B, L >> sh), -1, dtype=torch.int32)
    for b, n in enumerate(lengths):
        one = attention(sd, strokes[b:b + 1, :n], text[b:b + 1], sigma.reshape(-1)[b:b + 1], style[b:b + 1], name)
        P[b, :, :n >> sh] = one["probs"][0]
        mean[b, :n >> sh] = one["mean"][0]
        token[b, :n >> sh] = one["token"][0]
    return dict(probs=P, mean=mean, token=token)


def spread(P: torch.Tensor, text: torch.Tensor, lengths=None, shift: int = 0) -> float:
    """The reference's own contrast: the median over valid rows of max - min over the valid (non-pad) keys.  A bound below
    it can tell this map from a flat one."""
    vals = []
    for b in range(P.shape[0]):
        keys = (text[b] != 0).nonzero().flatten()
        if keys.numel() < 2:
            continue
        n = P.shape[2] if lengths is None else lengths[b] >> shift
        r = P[b, :, :n][..., keys]
        vals.append((r.max(dim=-1).values - r.min(dim=-1).values).flatten())
    return float(torch.cat(vals).median())
