"""What the stem kernel (hoigen_amd/csrc/hg_resnet_stem.hip) is held to: the float64 statement from the UNROUNDED operands, a restatement
of the kernel's arithmetic in torch on the CPU (`model`), and a bound PER OUTPUT ELEMENT.  A plain module beside the tests: no GPU, no
library.

    pre  = conv7x7/2,pad3(x, w) s + b                  float64, s and b the fp32 scale and bias the launch is given
    want = maxpool3x3/2,pad1(relu(pre))                torch's: the window's positions outside the conv map take no part, a NaN propagates
    Epre                                                tests/resnet_bound.py's stage() at K = 147 with e_in = |x - fp16(x)|: the operand's
                                                        and the weight's actual rounding, fp32 accumulation in any order, one fmaf
    b32  = max of Epre over the window's valid positions          since |max a - max b| <= max |a - b|, and ReLU does not grow an error
    b16  = b32 + f16_term(|want| + b32)                           the RNE rounding of the fp16 copy (tests/gemm_bound.py)

Rule: every element has |got - want| <= bound.  The exact families (tests/stem_cases.py EXACT) are expected bit for bit against `model`
(+0 and -0 equal); the non-finite outputs are exactly the reference's.

`model` restates the kernel: image and weight rounded once to fp16, the products accumulated in fp32 (torch's order - the exact families
do not depend on it, the bound holds for any), fmaf(acc, scale, bias), relu(v) = v < 0 ? 0 : v, the max over the valid positions that
keeps a NaN, RNE to fp16.  `mutant`: one of MUTANTS, a wrong kernel."""
import torch
import torch.nn.functional as F

from gemm_bound import f16_term
from resnet_bound import _fmaf, _to_f16, scale_bias, scale_bias64, stage, worst
from stem_cases import conv_size, pool_size

MUTANTS = ("drop_tap", "drop_channel", "swap_rs", "flip", "pad_clamp", "pad_wrap", "conv_pad2", "stride_one_axis", "conv_odd", "hc_ceil",
           "pool_start_2p", "pool_2x2", "hp_ceil", "pool_pad_relu_bias", "max_before_norm", "no_eps", "f16_truncate", "nan_dropped", "nan_leak",
           "tile_runs_on")
NEG_INF = float("-inf")


def reference(c, exact_norm=False):
    """dict(want, b32, b16), float64 [B, 64, Hp, Wp].  scale and bias are the fp32 values the launch is given; `exact_norm`: their exact
    float64 values, with the launch's rounding of them inside the bound (for a comparison with another implementation of the norm)."""
    s, b = scale_bias64(c["norm"]) if exact_norm else (t.double() for t in scale_bias(c["norm"]))
    x = c["x"].double()
    _, pre, E = stage(x, (x - c["x"].half().double()).abs(), c["w"], s, b, 2, exact_norm)
    want = F.max_pool2d(torch.relu(pre), 3, 2, 1)
    b32 = F.max_pool2d(E, 3, 2, 1)
    return dict(want=want, b32=b32, b16=b32 + f16_term(want.abs() + b32))


def reference_fp32(x, w, norm_forward):
    """the fixture's statement: F.conv2d -> the norm -> ReLU -> F.max_pool2d, in x's precision"""
    return F.max_pool2d(torch.relu(norm_forward(F.conv2d(x, w, None, 2, 3))), 3, 2, 1)


def _pool(r, Hp, Wp, offs, outside, drop_nan):
    """max over the window offsets `offs` (conv coordinate 2 p + o) of r [B, C, Hc, Wc]; a position outside r is `outside` ([C] or -inf)"""
    B, C, Hc, Wc = r.shape
    big = torch.full((B, C, 2 * Hp + 4, 2 * Wp + 4), NEG_INF)
    if outside is not None:
        big[:] = outside.reshape(1, -1, 1, 1)
    big[:, :, 2:2 + Hc, 2:2 + Wc] = r
    if drop_nan:
        big = torch.where(torch.isnan(big), torch.full_like(big, NEG_INF), big)
    cands = [big[:, :, 2 + dy:2 + dy + 2 * Hp:2, 2 + dx:2 + dx + 2 * Wp:2] for dy in offs for dx in offs]
    return torch.stack(cands).max(0).values      # torch's max keeps a NaN


def model(c, mutant=None):
    """dict(out32, out16), fp32 [B, 64, Hp, Wp]"""
    x, w = c["x"], c["w"]
    B, _, Hi, Wi = x.shape
    Hc, Wc = conv_size(Hi), conv_size(Wi)
    Hp, Wp = pool_size(Hc), pool_size(Wc)
    trunc = mutant == "f16_truncate"
    x16, w16 = _to_f16(x, trunc), _to_f16(w, trunc)
    if mutant == "drop_tap":
        w16 = w16.clone()
        w16[:, :, 6, 6] = 0
    elif mutant == "drop_channel":
        w16 = w16.clone()
        w16[:, 2] = 0
    elif mutant == "swap_rs":
        w16 = w16.transpose(2, 3)
    elif mutant == "flip":
        w16 = w16.flip(2, 3)
    P = 5                      # zeros around the image; the kernel's own pad is 3
    xp = F.pad(x16, (3, 3, 3, 3), mode="replicate") if mutant == "pad_clamp" else F.pad(x16, (3, 3, 3, 3))
    if mutant == "pad_wrap":   # a pad column is the flattened neighbour: column -k of row h is column Wi - k of row h - 1
        flat = F.pad(x16.reshape(B, 3, Hi * Wi), (3, 3))
        for k in (1, 2, 3):
            idx = torch.arange(Hi) * Wi
            xp[:, :, 3:3 + Hi, 3 - k] = flat[:, :, 3 + idx - k]
            xp[:, :, 3:3 + Hi, 2 + Wi + k] = flat[:, :, 3 + idx + Wi - 1 + k]
    if mutant == "tile_runs_on":      # the rows behind an image's last are the next image's first, and the other way round
        for k in range(min(3, Hi)):
            xp[:-1, :, 3 + Hi + k, 3:3 + Wi] = x16[1:, :, k, :]
            xp[1:, :, 2 - k, 3:3 + Wi] = x16[:-1, :, Hi - 1 - k, :]
    xp = F.pad(xp, (P - 3, 16, P - 3, 16))
    off = 1 if mutant == "conv_pad2" else -1 if mutant == "conv_odd" else 0
    sw = 1 if mutant == "stride_one_axis" else 2
    Hc2, Wc2 = (Hc, Wc) if mutant != "hc_ceil" else (-(-(Hi - 1) // 2) + 1, -(-(Wi - 1) // 2) + 1)
    o = P - 3 + off
    if mutant == "nan_leak":   # the eighth column of a lane's operand under a zero weight: 0 * NaN
        w16 = F.pad(w16, (0, 1))
    acc = F.conv2d(xp[:, :, o:, o:], w16, None, (2, sw))[:, :, :Hc2, :Wc2]
    scale, bias = scale_bias(c["norm"], eps_off=mutant == "no_eps")
    s4, b4 = scale.reshape(1, -1, 1, 1), bias.reshape(1, -1, 1, 1)
    relu = lambda t: torch.where(t < 0, torch.zeros_like(t), t)      # noqa: E731
    offs = (0, 1, 2) if mutant == "pool_start_2p" else (-1, 0) if mutant == "pool_2x2" else (-1, 0, 1)
    Hp2, Wp2 = (Hp, Wp) if mutant != "hp_ceil" else (-(-(Hc - 1) // 2) + 1, -(-(Wc - 1) // 2) + 1)
    outside = relu(bias) if mutant == "pool_pad_relu_bias" else None
    if mutant == "max_before_norm":
        v = relu(_fmaf(_pool(acc, Hp2, Wp2, offs, None, False), s4, b4))
    else:
        v = _pool(relu(_fmaf(acc, s4, b4)), Hp2, Wp2, offs, outside, mutant == "nan_dropped")
    if mutant == "hp_ceil":    # B Hp2 Wp2 rows of the wider map, read as the [B, Hp, Wp] the caller allocated
        v = v.permute(0, 2, 3, 1).reshape(-1, 64)[:B * Hp * Wp].reshape(B, Hp, Wp, 64).permute(0, 3, 1, 2)
    return dict(out32=v, out16=_to_f16(v, trunc))


def check(c, got, ref=None):
    """(failure messages, worst |err| / bound per output) of a launch's outputs (dict out32 / out16 as torch fp32 [B, 64, Hp, Wp]) on case
    c: every element inside the bound; the exact families bit for bit against `model`; the non-finite set equal to the reference's."""
    ref = ref or reference(c)
    fails, ratios = [], {}
    exact = model(c) if c["family"] in ("ints", "pow2") else None
    for k, b in (("out32", "b32"), ("out16", "b16")):
        g = got[k]
        if tuple(g.shape) != tuple(ref["want"].shape):
            fails.append(f"{k}: shape {tuple(g.shape)}, expected {tuple(ref['want'].shape)}")
            continue
        nf_want, nf_got = ~torch.isfinite(ref["want"]), ~torch.isfinite(g)
        if not torch.equal(nf_want, nf_got):
            fails.append(f"{k}: {int(nf_got.sum())} non-finite outputs, the reference has {int(nf_want.sum())} (or elsewhere)")
        bound = torch.where(nf_want, torch.ones_like(ref[b]), ref[b])
        r, bad = worst(torch.where(nf_want, torch.zeros_like(g), g), torch.where(nf_want, torch.zeros_like(ref["want"]), ref["want"]), bound)
        ratios[k] = r
        if bad:
            fails.append(f"{k}: {bad} elements outside the bound, worst |err| / bound {r:.3f}")
        if exact is not None and not torch.equal(g, exact[k]):
            fails.append(f"{k}: {int((g != exact[k]).sum())} elements differ from the exact expectation")
    return fails, ratios
