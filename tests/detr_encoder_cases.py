"""Seeded weights, inputs and rectangle masks for the DETR encoder tests, and the float64 restatement of the encoder
(detr/models/transformer.py:62-83 over the post-norm layer :149-162) they are compared with.  numpy only for the data, as
hoigen_amd/synth.py makes its own; torch float64 on the CPU for the restatement.  No GPU, no library.

Weights: matrices Xavier-uniform, as the reference initialises them (transformer.py:41-45 `_reset_parameters`: xavier_uniform_ on every
parameter with more than one dimension, in_proj_weight as one [3D, D] matrix); biases 0.1 randn; LayerNorm weights 1 + 0.2 randn and
biases 0.1 randn.  Real DETR-R50 weights are not available to the tests: parity is shown on these.
"""
import numpy as np
import torch

from hoigen_amd import synth

FULL = dict(d_model=256, heads=8, d_ff=2048, layers=6)          # the detector's encoder
SMALL = dict(d_model=128, heads=4, d_ff=256, layers=2)


def wide(d_model):
    """one layer at a width beyond the detector's: 384 (12 heads), 512 (16), 640 (20; the encoder alone), d_ff 256"""
    return dict(d_model=d_model, heads=d_model // 32, d_ff=256, layers=1)


# the fixture's case (tests/golden/make_golden_detr_encoder.py): B = 3 on a 13 x 17 grid; image 0 unpadded, 1 visible on 10 x 12, 2 on 4 x 5
G18 = dict(B=3, gh=13, gw=17, visible=((13, 17), (10, 12), (4, 5)), wseed=18, xseed=180)

LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def _uniform(shape, seed):
    """U(-1, 1) float64, a pure function of (shape, seed): the 53 high bits of splitmix64"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        h = synth._splitmix64(np.arange(n, dtype=np.uint64) + (np.uint64(seed & 0xFFFFFF) << np.uint64(40)))
    return ((h >> np.uint64(11)).astype(np.float64) / float(1 << 53) * 2.0 - 1.0).reshape(shape)


def weights(cfg=FULL, seed=18):
    """state dict of the reference's TransformerEncoder: `layers.N.<LAYER_KEYS>` -> float32 numpy arrays"""
    D, F = cfg["d_model"], cfg["d_ff"]
    shapes = {"self_attn.in_proj_weight": (3 * D, D), "self_attn.in_proj_bias": (3 * D,), "self_attn.out_proj.weight": (D, D),
              "self_attn.out_proj.bias": (D,), "linear1.weight": (F, D), "linear1.bias": (F,), "linear2.weight": (D, F), "linear2.bias": (D,),
              "norm1.weight": (D,), "norm1.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,)}
    sd = {}
    for l in range(cfg["layers"]):
        for key in LAYER_KEYS:
            name, shape = f"layers.{l}.{key}", shapes[key]
            s = synth._seed_of(seed, name)
            if len(shape) == 2:
                a = np.sqrt(6.0 / (shape[0] + shape[1]))
                sd[name] = (a * _uniform(shape, s)).astype(np.float32)
            elif key.startswith("norm") and key.endswith("weight"):
                sd[name] = synth.hg_normal(shape, s, 0.2, 1.0)
            else:
                sd[name] = synth.hg_normal(shape, s, 0.1)
    return sd


def inputs(B, gh, gw, D, seed):
    """src, pos float32 [S, B, D] (the reference's layout), S = gh * gw"""
    S = gh * gw
    return synth.hg_normal((S, B, D), synth._seed_of(seed, "src")), synth.hg_normal((S, B, D), synth._seed_of(seed, "pos"))


def rect_mask(gh, gw, visible):
    """uint8 [B, gh * gw], 1 = padding: image b is visible on the top-left visible[b] = (vh, vw) cells (right and bottom padding)"""
    m = np.ones((len(visible), gh, gw), np.uint8)
    for b, (vh, vw) in enumerate(visible):
        m[b, :vh, :vw] = 0
    return m.reshape(len(visible), gh * gw)


MASK_KINDS = ("none", "rect", "one", "head64", "midrun", "perimage")


def mask_of(kind, B, gh, gw):
    """the masks of tests/detr_attn_bound.py on a grid: uint8 [B, gh * gw] or None"""
    S = gh * gw
    if kind == "none":
        return None
    if kind == "rect":
        return rect_mask(gh, gw, [(max(1, gh - (b + 1) * gh // 4), max(1, gw - (b + 2) * gw // 5)) for b in range(B)])
    m = np.zeros((B, S), np.uint8)
    if kind == "one":
        m[:] = 1
        for b in range(B):
            m[b, (0, S // 2, S - 1)[b % 3]] = 0
    elif kind == "head64":
        m[:, :min(64, S - 1)] = 1
    elif kind == "midrun":
        a = max(0, (S // 3) // 32 * 32 - 5) if S >= 160 else S // 3
        m[:, a:max(a + 1, min(S - 1, a + 72 if S >= 160 else 2 * S // 3))] = 1
    else:
        assert kind == "perimage", kind
        for b in range(B):
            k = ("rect", "head64", "none", "midrun")[b % 4]
            if k != "none":
                m[b] = mask_of(k, B, gh, gw)[b]
    return m


def encoder_fp64(sd, cfg, src, pos, mask, layers=None):
    """The encoder in float64 on the CPU: the stream after every layer, a list of [B * S, D] tensors (batch-major rows, as the device's
    trace).  src, pos [S, B, D]; mask uint8 / bool [B, S] or None.  Every step is the reference's: q = k = src + pos, v = src, the
    in_proj split of nn.MultiheadAttention, softmax(q k^T / sqrt(head dim) + key padding mask) v, out_proj, residual, norm1, linear1,
    ReLU, linear2, residual, norm2 (LayerNorm eps 1e-5, biased variance)."""
    D, H = cfg["d_model"], cfg["heads"]
    hd = D // H
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    x = t(src).transpose(0, 1).contiguous()          # [B, S, D]
    p = t(pos).transpose(0, 1).contiguous() if pos is not None else torch.zeros_like(x)
    B, S, _ = x.shape
    vis = torch.ones(B, S, dtype=torch.bool) if mask is None else ~torch.as_tensor(np.asarray(mask)).bool()

    def ln(v, w, b):
        mu = v.mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        return (v - mu) / torch.sqrt(var + 1e-5) * w + b

    out = []
    for l in range(cfg["layers"] if layers is None else layers):
        g = lambda key: t(sd[f"layers.{l}.{key}"])
        w_in, b_in = g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias")
        qk_in = x + p
        q = qk_in @ w_in[:D].T + b_in[:D]
        k = qk_in @ w_in[D:2 * D].T + b_in[D:2 * D]
        v = x @ w_in[2 * D:].T + b_in[2 * D:]
        heads = lambda a: a.view(B, S, H, hd).permute(0, 2, 1, 3)
        s = heads(q) @ heads(k).transpose(-1, -2) / np.sqrt(hd)
        s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
        att = (torch.softmax(s, -1) @ heads(v)).permute(0, 2, 1, 3).reshape(B, S, D)
        x = ln(x + att @ g("self_attn.out_proj.weight").T + g("self_attn.out_proj.bias"), g("norm1.weight"), g("norm1.bias"))
        ff = torch.relu(x @ g("linear1.weight").T + g("linear1.bias")) @ g("linear2.weight").T + g("linear2.bias")
        x = ln(x + ff, g("norm2.weight"), g("norm2.bias"))
        out.append(x.reshape(B * S, D).clone())
    return out


def rel_l2(got, want):
    """(relative L2 of the whole tensor, of the worst row) over the rows where `want` is finite"""
    g, w = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(want)).double()
    ok = torch.isfinite(w).all(-1)
    g, w = g[ok], w[ok]
    return float((g - w).norm() / w.norm()), float(((g - w).norm(dim=-1) / w.norm(dim=-1)).max())
