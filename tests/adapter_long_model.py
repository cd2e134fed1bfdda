"""The rounding model of the instance adapter (tests/test_adapter_rounding_model.py) restated for sequences of 225 .. 640 tokens that are
their own memory (hoigen_amd/csrc/hg_adapter_long.hip): the keys arrive in chunks of 224, the softmax keeps a running maximum m, sum l and
output o across them, and the probabilities of a chunk are rounded to fp16 relative to the running maximum of THAT moment, not to the
final one.  Everything else is rm.model's arithmetic.  With priors a token's keys (at most 32) are one chunk: rm.model itself.

Wrong kernels (`mut`): "drop_last" - the last key chunk never read; "double" - the first key of every chunk but the first counted in
the chunk before it as well; "no_rescale" - l and o not rescaled when the maximum moves.
"""
import numpy as np
import torch

import test_adapter_rounding_model as rm
from oracle import clip_oracle as co

KCH = 224
LENGTHS = (225, 448, 449, 577, 640)
FAMILIES = ("unit", "small", "outlier", "ramp", "ramp_rev")
MUTANTS = ("drop_last", "double", "no_rescale")


def make_stream(kind, n_seq, L, D, seed):
    """rm.make_stream and two more families: `ramp` = the unit stream x linspace(0.25, 2, L) along the tokens (the largest scores sit in
    the last key chunk: the running maximum moves in every chunk), `ramp_rev` = the same downwards (it settles in the first)."""
    if kind in ("ramp", "ramp_rev"):
        x = rm.make_stream("unit", n_seq, L, D, seed)
        w = torch.linspace(0.25, 2.0, L, dtype=torch.float32)
        if kind == "ramp_rev":
            w = w.flip(0)
        return (x * w[None, :, None]).contiguous()
    return rm.make_stream(kind, n_seq, L, D, seed)


def chunked_attention(q, k, v, Hm, mut=None, kch=KCH):
    """softmax(q k^T) v of one head over key chunks with a running maximum; q [n, L, 32] already scaled, fp16 values in float64"""
    L = k.shape[1]
    bounds = list(range(0, L, kch)) + [L]
    chunks = list(zip(bounds[:-1], bounds[1:]))
    if mut == "drop_last":
        chunks = chunks[:-1]
    m = torch.full(q.shape[:2] + (1,), float("-inf"), dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for i, (a, b) in enumerate(chunks):
        if mut == "double" and i + 1 < len(chunks):
            b += 1
        s = q @ k[:, a:b].transpose(1, 2)
        m_new = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        alpha = torch.zeros_like(m) if i == 0 else torch.exp(m - m_new)
        if mut == "no_rescale" and i > 0:
            alpha = torch.ones_like(m)
        p = torch.exp(s - m_new)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        o = o * alpha + Hm(p) @ v[:, a:b]
        m = m_new
    return o / l


def _decoder_self(tgt, sd, lp, Hm, mut):
    """rm._decoder with the sequence as its own memory and the chunked softmax"""
    t16 = Hm(tgt)
    wi, bi = Hm(sd[lp + "multihead_attn.in_proj_weight"]), sd[lp + "multihead_attn.in_proj_bias"]
    q = Hm((t16 @ wi[:64].T + bi[:64]) * 32 ** -0.5)
    k = Hm(t16 @ wi[64:128].T + bi[64:128])
    v = Hm(t16 @ wi[128:].T + bi[128:])
    o = torch.empty_like(q)
    for h in range(2):
        sl = slice(32 * h, 32 * h + 32)
        o[..., sl] = chunked_attention(q[..., sl], k[..., sl], v[..., sl], Hm, mut)
    t2 = Hm(o) @ Hm(sd[lp + "multihead_attn.out_proj.weight"]).T + sd[lp + "multihead_attn.out_proj.bias"]
    tgt = co.layer_norm(tgt + t2, sd[lp + "norm2.weight"], sd[lp + "norm2.bias"])
    hid = torch.relu(Hm(tgt) @ Hm(sd[lp + "linear1.weight"]).T + sd[lp + "linear1.bias"])
    return tgt + Hm(hid) @ Hm(sd[lp + "linear2.weight"]).T + sd[lp + "linear2.bias"]


def model_self(x, sd, pre, mode=0, mut=None, centre=None):
    """rm.model for modes 0 and 1, memory = the sequence, MFMA roundings, the softmax over key chunks.  Returns {"a": update}."""
    assert mode in (0, 1)
    x = x.double()
    H = rm.H
    if mode == 0:
        xin = H(x)
    else:
        mu = (x.float().mean(-1) if centre is None else centre.float()).double()[..., None]
        xin = H(x - mu) + mu
    down = torch.relu(xin @ H(sd[pre + "down_proj.weight"]).T + sd[pre + "down_proj.bias"])
    lp = pre + "mhsa."
    down = co.layer_norm(_decoder_self(down, sd, lp, H, mut), sd[lp + "norm3.weight"], sd[lp + "norm3.bias"])
    a = (H(down) @ H(sd[pre + "up_proj.weight"]).T + sd[pre + "up_proj.bias"]) * sd[pre + "scale"]
    return {"a": (x + a).float().double() - x}
