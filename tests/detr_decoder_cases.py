"""Seeded weights and inputs for the DETR decoder tests, and the float64 restatement of the decoder (detr/models/transformer.py:86-124
over the post-norm layer :212-233) they are compared with.  numpy only for the data; torch float64 on the CPU for the restatement.
No GPU, no library.

Weights as tests/detr_encoder_cases.py makes them (Xavier-uniform matrices, 0.1 randn biases, LayerNorm 1 +- 0.2 / 0.1) under the
decoder's key names: `layers.N.<LAYER_KEYS>`, `norm.weight`, `norm.bias`.
"""
import numpy as np
import torch

import detr_encoder_cases as ec
from hoigen_amd import synth

FULL, SMALL, G18 = ec.FULL, ec.SMALL, ec.G18
# the fixtures' case (tests/golden/make_golden_detr_decoder.py): G18's grid and rectangle mask, 100 queries; the decoder's own seeds
G19 = dict(B=3, gh=13, gw=17, visible=G18["visible"], Q=100, wseed=19, xseed=190, enc_wseed=18)

LAYER_KEYS = ec.LAYER_KEYS + ("multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight",
                              "multihead_attn.out_proj.bias", "norm3.weight", "norm3.bias")


def weights(cfg=FULL, seed=19):
    """state dict of the reference's TransformerDecoder -> float32 numpy arrays"""
    D, F = cfg["d_model"], cfg["d_ff"]
    shapes = {"in_proj_weight": (3 * D, D), "in_proj_bias": (3 * D,), "out_proj.weight": (D, D), "out_proj.bias": (D,),
              "linear1.weight": (F, D), "linear1.bias": (F,), "linear2.weight": (D, F), "linear2.bias": (D,)}
    names = [f"layers.{l}.{k}" for l in range(cfg["layers"]) for k in LAYER_KEYS] + ["norm.weight", "norm.bias"]
    sd = {}
    for name in names:
        key = name.split(".", 2)[2] if name.startswith("layers.") else name
        short = key.split(".", 1)[1] if key.startswith(("self_attn.", "multihead_attn.")) else key
        shape = shapes.get(short, (D,))
        s = synth._seed_of(seed, "decoder." + name)
        if len(shape) == 2:
            sd[name] = (np.sqrt(6.0 / (shape[0] + shape[1])) * ec._uniform(shape, s)).astype(np.float32)
        elif key.startswith("norm") and key.endswith("weight"):
            sd[name] = synth.hg_normal(shape, s, 0.2, 1.0)
        else:
            sd[name] = synth.hg_normal(shape, s, 0.1)
    return sd


def inputs(B, gh, gw, Q, D, seed):
    """query_embed [Q, D], memory, pos [S, B, D] (the reference's layouts) float32"""
    S = gh * gw
    return (synth.hg_normal((Q, D), synth._seed_of(seed, "query_embed")), synth.hg_normal((S, B, D), synth._seed_of(seed, "memory")),
            synth.hg_normal((S, B, D), synth._seed_of(seed, "pos")))


def src_map(B, gh, gw, D, seed):
    """src, pos_embed [B, D, gh, gw] float32 for the whole Transformer"""
    return (synth.hg_normal((B, D, gh, gw), synth._seed_of(seed, "src_map")), synth.hg_normal((B, D, gh, gw), synth._seed_of(seed, "pos_map")))


def decoder_fp64(sd, cfg, memory, pos, mask, query_pos, tgt=None, layers=None):
    """The decoder in float64 on the CPU: (the stream after every layer - after norm3 - as a list of [B * Q, D] tensors with batch-major
    rows, hs [L, Q, B, D] = the final norm of each).  memory, pos [S, B, D]; query_pos [Q, D] or [Q, B, D]; tgt [Q, B, D] or None (zeros);
    mask uint8 / bool [B, S] or None.  Every step is the reference's (transformer.py:219-233)."""
    D, H = cfg["d_model"], cfg["heads"]
    hd = D // H
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    mem = t(memory).transpose(0, 1).contiguous()          # [B, S, D]
    p = t(pos).transpose(0, 1).contiguous() if pos is not None else torch.zeros_like(mem)
    B, S, _ = mem.shape
    qp = t(query_pos)
    qp = (qp[:, None, :].expand(-1, B, -1) if qp.dim() == 2 else qp).transpose(0, 1).contiguous()      # [B, Q, D]
    Q = qp.shape[1]
    x = t(tgt).transpose(0, 1).contiguous() if tgt is not None else torch.zeros(B, Q, D, dtype=torch.float64)
    vis = torch.ones(B, S, dtype=torch.bool) if mask is None else ~torch.as_tensor(np.asarray(mask)).bool()

    def ln(v, w, b):
        mu = v.mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        return (v - mu) / torch.sqrt(var + 1e-5) * w + b

    def mha(prefix, g, q_in, k_in, v_in, keys_visible):
        w, b = g(prefix + ".in_proj_weight"), g(prefix + ".in_proj_bias")
        q, k, v = q_in @ w[:D].T + b[:D], k_in @ w[D:2 * D].T + b[D:2 * D], v_in @ w[2 * D:].T + b[2 * D:]
        heads = lambda a: a.view(B, a.shape[1], H, hd).permute(0, 2, 1, 3)
        s = heads(q) @ heads(k).transpose(-1, -2) / np.sqrt(hd)
        if keys_visible is not None:
            s = s.masked_fill(~keys_visible[:, None, None, :], float("-inf"))
        att = (torch.softmax(s, -1) @ heads(v)).permute(0, 2, 1, 3).reshape(B, q_in.shape[1], D)
        return att @ g(prefix + ".out_proj.weight").T + g(prefix + ".out_proj.bias")

    nw, nb = t(sd["norm.weight"]), t(sd["norm.bias"])
    streams, hs = [], []
    for l in range(cfg["layers"] if layers is None else layers):
        g = lambda key: t(sd[f"layers.{l}.{key}"])
        x = ln(x + mha("self_attn", g, x + qp, x + qp, x, None), g("norm1.weight"), g("norm1.bias"))
        x = ln(x + mha("multihead_attn", g, x + qp, mem + p, mem, vis), g("norm2.weight"), g("norm2.bias"))
        ff = torch.relu(x @ g("linear1.weight").T + g("linear1.bias")) @ g("linear2.weight").T + g("linear2.bias")
        x = ln(x + ff, g("norm3.weight"), g("norm3.bias"))
        streams.append(x.reshape(B * Q, D).clone())
        hs.append(ln(x, nw, nb).transpose(0, 1).clone())      # [Q, B, D]
    return streams, torch.stack(hs)


rel_l2 = ec.rel_l2
