"""What the bottleneck convolution and the stages built on it (hoigen_amd/csrc/hg_resnet_conv.hip, hg_resnet.hip) are held to: the float64
statement from the UNROUNDED operands, a restatement of the kernel's arithmetic in torch on the CPU (`model`), and a bound PER OUTPUT
ELEMENT that is the sum of the worst case of each rounding the kernel performs.  A plain module beside the tests: no GPU, no library.

One convolution stage, all float64, u = 2^-24.  v is the stage's exact input, e_in a bound on |kernel's fp16 operand - v| per element
(for a stage fed by a launch's returned fp32 tensor: the ACTUAL |v - fp16(v)|), w the unrounded weight, w16 its fp16 rounding:

    acc  = conv(v, w)                                                      the reference accumulates the unrounded operands
    E    = conv(e_in, |w|)                                                 the operand's error through |w|
         + conv(|v| + e_in, |w - w16|)                                     the weight's actual rounding error through |x|
         + K 2^-23 conv(|v| + e_in, |w16|)                                 fp32 accumulation of K = R R Cin exact products in ANY order
                                                                           (2^-23, so that it holds whether the matrix unit's adds
                                                                           round or truncate: tests/gemm_bound.py)
    pre  = acc s + b                                                       s, b: the norm's scale and bias
    Epre = E |s| + u |pre|                                                 the fmaf rounds once
         + u |acc s| + u |b|            only where s and b are the exact float64 values and the kernel's are their fp32 roundings
    epilogue 1   want = relu(pre)                 ReLU does not grow an error;       fp16 output: + f16_term(|want| + Epre)
    epilogue 2   want = pre
    epilogue 3   want = relu(pre + id)            + u |pre + id| for the add (id is read as fp32, exact);  the fp16 copy: + f16_term
f16_term is tests/gemm_bound.py's: 2^-11 t for a normal result, 2^-25 where t < 2^-14 (the subnormal floor).

A block (`block_reference`) chains the stages from the block input the launch RETURNED: conv1 -> conv2 -> conv3 with each stage's
output bound as the next stage's e_in, the downsample beside them; errors of earlier blocks do not enter.

Rule: every element has |got - want| <= bound.  The exact families (tests/resnet_cases.py EXACT) hold numbers whose products and partial
sums fp32 represents, so any summation order gives the same accumulator and `model` is expected bit for bit."""
import math

import torch
import torch.nn.functional as F

from gemm_bound import U, f16_term

MUTANTS = ("drop_tap", "drop_cblock", "swap_rs", "flip", "pad_clamp", "pad_wrap", "stride_one_axis", "down_odd", "ho_ceil", "f16_truncate",
           "relu_before_add", "identity_f16", "no_eps", "scale_after_relu", "tile_runs_on")


def out_size(H, R, stride):
    return (H + 2 * ((R - 1) // 2) - R) // stride + 1


def scale_bias64(norm, eps_off=False):
    """backbone.py:45-55 in float64: scale = w / sqrt(rv + eps), bias = b - rm * scale"""
    w, b, rm, rv, eps = norm
    s = w.double() / torch.sqrt(rv.double() + (0.0 if eps_off else eps))
    return s, b.double() - rm.double() * s


def scale_bias(norm, eps_off=False):
    """what the loader makes: the float64 values rounded to fp32"""
    s, b = scale_bias64(norm, eps_off)
    return s.float(), b.float()


def conv64(x, w, stride):
    """float64 convolution, pad (R - 1) / 2, as unfold + matmul (zeros are real zeros: a NaN reaches exactly the windows that hold it)"""
    B, C, H, W = x.shape
    R = w.shape[2]
    Ho, Wo = out_size(H, R, stride), out_size(W, R, stride)
    cols = F.unfold(x.double(), R, padding=(R - 1) // 2, stride=stride)
    return (w.double().reshape(w.shape[0], -1) @ cols).reshape(B, w.shape[0], Ho, Wo)


def stage(v, e_in, w, s64, b64, stride, sb_rounded):
    """(acc, pre, Epre) of one convolution stage (module docstring)"""
    w16 = w.half().double()
    K = w.shape[1] * w.shape[2] * w.shape[3]
    mag = v.abs() + e_in
    acc = conv64(v, w, stride)
    E = conv64(e_in, w.double().abs(), stride) + conv64(mag, (w.double() - w16).abs(), stride) + K * 2.0 ** -23 * conv64(mag, w16.abs(), stride)
    s, b = s64.reshape(1, -1, 1, 1), b64.reshape(1, -1, 1, 1)
    pre = acc * s + b
    Epre = E * s.abs() + U * pre.abs()
    if sb_rounded:
        Epre = Epre + U * (acc * s).abs() + U * b.abs()
    return acc, pre, Epre


def reference(c):
    """One convolution launch on a case of tests/resnet_cases.py: dict(want, b32, b16), float64 [B, Cout, Ho, Wo]; b32 bounds the fp32
    output (epilogues 2, 3), b16 the fp16 one (1, 3).  scale and bias are the fp32 values the launch is given."""
    s, b = scale_bias(c["norm"])
    x = c["x"].double()
    _, pre, E = stage(x, (x - c["x"].half().double()).abs(), c["w"], s.double(), b.double(), c["stride"], False)
    if c["epi"] == 3:
        pre = pre + c["identity"].double()
        E = E + U * pre.abs()
    want = pre if c["epi"] == 2 else torch.relu(pre)
    want = torch.where(torch.isnan(pre), pre, want)      # torch.relu keeps a NaN; spelled out
    return dict(want=want, b32=E, b16=E + f16_term(want.abs() + E))


def _norm_of(n):
    return (n.weight, n.bias, n.running_mean, n.running_var, float(getattr(n, "eps", 1e-5)))


def block_reference(blk, x, e_x=None):
    """A bottleneck block (conv1, bn1, .. downsample with torchvision's names; norms with or without an eps attribute): dict(want, b32,
    b16) of the block's output, float64.  e_x None: x is the fp32 block input the launch returned (its fp16 copy's error is the actual
    one, the identity is exact).  Otherwise x is the exact input and e_x bounds the launch's fp32 stream against it, per element."""
    def sb(n):
        return scale_bias64(_norm_of(n))

    x64 = x.double()
    if e_x is None:
        e0, e32 = (x64 - x.half().double()).abs(), 0.0
    else:
        e0, e32 = e_x + f16_term(x64.abs() + e_x), e_x
    v, e = x64, e0
    for cn, bn in (("conv1", "bn1"), ("conv2", "bn2")):
        conv = getattr(blk, cn)
        _, pre, E = stage(v, e, conv.weight.detach(), *sb(getattr(blk, bn)), conv.stride[0], True)
        v = torch.relu(pre)
        e = E + f16_term(v.abs() + E)
    _, pre, E = stage(v, e, blk.conv3.weight.detach(), *sb(blk.bn3), blk.conv3.stride[0], True)
    if blk.downsample is not None:
        _, idn, Ed = stage(x64, e0, blk.downsample[0].weight.detach(), *sb(blk.downsample[1]), blk.downsample[0].stride[0], True)
    else:
        idn, Ed = x64, e32
    pre = pre + idn
    E = E + Ed + U * pre.abs()
    want = torch.relu(pre)
    return dict(want=want, b32=E, b16=E + f16_term(want.abs() + E))


def block_model(blk, x):
    """the block restated with `model`: (out32, out16) from the fp32 block input x"""
    def case(conv, norm, inp, epi, identity=None):
        return dict(x=inp, w=conv.weight.detach(), R=conv.kernel_size[0], stride=conv.stride[0], epi=epi, norm=_norm_of(norm), identity=identity)

    t = model(case(blk.conv1, blk.bn1, x, 1))["out16"]
    t = model(case(blk.conv2, blk.bn2, t, 1))["out16"]
    idn = x if blk.downsample is None else model(case(blk.downsample[0], blk.downsample[1], x, 2))["out32"]
    o = model(case(blk.conv3, blk.bn3, t, 3, idn))
    return o["out32"], o["out16"]


def worst(got, want, bound):
    """max |got - want| / bound over the finite expectations, and the number of elements outside"""
    ok = torch.isfinite(want)
    r = ((got.double() - want).abs() / bound.clamp_min(1e-300))[ok]
    bad = int((r > 1.0).sum()) + int((~torch.isfinite(got.double()[ok])).sum())
    return (float(r[torch.isfinite(r)].max()) if r.numel() and torch.isfinite(r).any() else 0.0), bad


# ---- the kernel's arithmetic restated -------------------------------------------------------------------------------------------------
def _to_f16(v, truncate):
    if not truncate:
        return v.half().float()
    h = v.half().float()      # toward zero: step back where rounding went away from zero
    away = h.abs() > v.abs()
    bits = h.half().view(torch.int16)
    return torch.where(away, (bits - 1).view(torch.float16).float(), h)


def _fmaf(a, s, b):
    """fmaf in fp32 through float64: the product of two fp32 numbers is exact there"""
    return (a.double() * s.double() + b.double()).float()


def model(c, mutant=None):
    """The launch restated: operands rounded to fp16, fp32 accumulation over taps (r, s) ascending then 64-channel blocks ascending (torch's
    fp32 sum inside a block), fmaf(acc, scale, bias), the fp32 identity, ReLU, RNE to fp16.  Returns dict(out32, out16) (None where the
    epilogue has none), fp32 [B, Cout, Ho, Wo].  `mutant`: one of MUTANTS, a wrong kernel."""
    x, w, R, st, epi = c["x"], c["w"], c["R"], c["stride"], c["epi"]
    B, Cin, H, W = x.shape
    p = (R - 1) // 2
    Ho, Wo = out_size(H, R, st), out_size(W, R, st)
    x16, w16 = x.half().float(), w.half().float()
    Ho2, Wo2 = Ho, Wo
    if mutant == "ho_ceil":
        Ho2, Wo2 = math.ceil((H + 2 * p - R) / st) + 1, math.ceil((W + 2 * p - R) / st) + 1
    xp = F.pad(x16, (p, p, p, p), mode="replicate" if mutant == "pad_clamp" and p else "constant")
    if mutant == "pad_wrap" and p:       # column -1 of row h is the flattened neighbour: column W - 1 of row h - 1; column W is column 0 of row h + 1
        xp[:, :, p + 1:p + H, 0] = x16[:, :, :H - 1, W - 1]
        xp[:, :, p:p + H - 1, p + W] = x16[:, :, 1:, 0]
    if mutant == "tile_runs_on" and p:   # the row behind an image's last is the next image's first
        xp[:-1, :, p + H, p:p + W] = x16[1:, :, 0, :]
        xp[1:, :, 0, p:p + W] = x16[:-1, :, H - 1, :]
    xp = F.pad(xp, (0, 2 * st + 2, 0, 2 * st + 2))      # room for the mutants that read further; zeros
    off = 1 if mutant == "down_odd" and st == 2 else 0
    sw = 1 if mutant == "stride_one_axis" else st
    acc = torch.zeros(B, w.shape[0], Ho2, Wo2)
    ncb = Cin // 64
    for r in range(R):
        for s in range(R):
            if mutant == "drop_tap" and (r, s) == (R - 1, R - 1):
                continue
            wt = w16[:, :, s, r] if mutant == "swap_rs" else w16[:, :, R - 1 - r, R - 1 - s] if mutant == "flip" else w16[:, :, r, s]
            patch = xp[:, :, r + off:r + off + (Ho2 - 1) * st + 1:st, s + off:s + off + (Wo2 - 1) * sw + 1:sw]
            for cb in range(ncb):
                if mutant == "drop_cblock" and cb == ncb - 1:
                    continue
                acc = acc + torch.einsum("bchw,oc->bohw", patch[:, cb * 64:(cb + 1) * 64], wt[:, cb * 64:(cb + 1) * 64])
    if mutant == "ho_ceil":              # M rows of the wider map, read as the [B, Ho, Wo] the caller allocated
        acc = acc.permute(0, 2, 3, 1).reshape(-1, w.shape[0])[:B * Ho * Wo].reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2)
    scale, bias = scale_bias(c["norm"], eps_off=mutant == "no_eps")
    scale, bias = scale.reshape(1, -1, 1, 1), bias.reshape(1, -1, 1, 1)
    relu = lambda t: torch.where(t < 0, torch.zeros_like(t), t)
    if mutant == "scale_after_relu":
        v = _fmaf(relu(acc), scale, bias)
    else:
        v = _fmaf(acc, scale, bias)
    if epi == 3:
        idn = c["identity"].half().float() if mutant == "identity_f16" else c["identity"]
        v = relu(v) + idn if mutant == "relu_before_add" else v + idn
    if epi != 2 and mutant != "scale_after_relu":
        v = relu(v)
    return dict(out32=None if epi == 1 else v, out16=None if epi == 2 else _to_f16(v, mutant == "f16_truncate"))


def check(c, got, ref=None):
    """(failure messages, worst |err| / bound per output) of a launch's outputs (dict out32 / out16 as torch fp32 [B, Cout, Ho, Wo]) on
    case c: every element inside the bound; the exact families bit for bit against `model`; the NaN family's non-finite set equal to the
    reference's."""
    ref = ref or reference(c)
    fails, ratios = [], {}
    exact = model(c) if c["family"] in ("ints", "pow2") else None
    for k, b in (("out32", "b32"), ("out16", "b16")):
        g = got.get(k)
        if g is None:
            continue
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
