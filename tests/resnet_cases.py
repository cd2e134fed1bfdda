"""Seeded inputs for the ResNet bottleneck stages (hoigen_amd/csrc/hg_resnet_conv.hip, hoigen_amd/resnet.py): stand-in modules written from
the architecture with torchvision's attribute names (torchvision itself is not installed), the seeded recipe of their parameters, and the
input families of the single-convolution tests.  torch on the CPU only.  No GPU, no library.

The recipe: convolution weights N(0, 2 / fan_in); bn1 / bn2 weight U(0.5, 1.5), bn3 weight U(0.1, 0.3), downsample norm weight
U(0.5, 1.5); norm bias and running_mean N(0, 0.1), running_var U(0.5, 1.5); the input relu(N(0, 1)).  With it a full ResNet-50 neither
dies nor blows up: 49 to 78 % of its outputs stay positive at every depth, with rms 0.9 to 1.7."""
import math
import zlib

import torch
from torch import nn

SEED = 20


class FrozenBN(nn.Module):
    """The reference's FrozenBatchNorm2d by its structure: four buffers, eps fixed at 1e-5 inside forward (no eps attribute)."""

    def __init__(self, n):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def forward(self, x):
        scale = self.weight.reshape(1, -1, 1, 1) * (self.running_var.reshape(1, -1, 1, 1) + 1e-5).rsqrt()
        return x * scale + (self.bias.reshape(1, -1, 1, 1) - self.running_mean.reshape(1, -1, 1, 1) * scale)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, stride_on_conv1=False, norm=FrozenBN):
        super().__init__()
        s1, s2 = (stride, 1) if stride_on_conv1 else (1, stride)
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride=s1, bias=False)
        self.bn1 = norm(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=s2, padding=1, bias=False)
        self.bn2 = norm(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = norm(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class BasicBlock(nn.Module):
    """resnet18 / 34's block: what ResNetStages refuses."""

    def __init__(self, planes=64):
        super().__init__()
        self.conv1 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn1 = FrozenBN(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = FrozenBN(planes)
        self.downsample = None


class ResNet(nn.Module):
    """conv1 7 x 7 / 2, bn1, relu, maxpool 3 x 3 / 2, layer1 .. layer4 of bottleneck blocks; no avgpool / fc (the body never runs them)."""

    def __init__(self, blocks=(3, 4, 6, 3), planes=(64, 128, 256, 512), strides=(1, 2, 2, 2), stem=64, stride_on_conv1=False, norm=FrozenBN):
        super().__init__()
        self.conv1 = nn.Conv2d(3, stem, 7, stride=2, padding=3, bias=False)
        self.bn1 = norm(stem)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        cin = stem
        for i, (nb, p, st) in enumerate(zip(blocks, planes, strides)):
            layer = []
            for j in range(nb):
                s = st if j == 0 else 1
                down = None
                if j == 0 and (s != 1 or cin != 4 * p):
                    down = nn.Sequential(nn.Conv2d(cin, 4 * p, 1, stride=s, bias=False), norm(4 * p))
                layer.append(Bottleneck(cin, p, s, down, stride_on_conv1, norm))
                cin = 4 * p
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
        self.num_channels = cin

    def stages(self, x):
        for i in range(1, 5):
            x = getattr(self, f"layer{i}")(x)
        return x

    def forward(self, x):
        return self.stages(self.maxpool(self.relu(self.bn1(self.conv1(x)))))


def _fill_norm(n, lo, hi, g):
    n.weight.data = torch.empty(n.weight.shape).uniform_(lo, hi, generator=g)
    n.bias.data = torch.randn(n.bias.shape, generator=g) * 0.1
    n.running_mean.data = torch.randn(n.running_mean.shape, generator=g) * 0.1
    n.running_var.data = torch.empty(n.running_var.shape).uniform_(0.5, 1.5, generator=g)


def _fill_conv(c, g):
    fan_in = c.weight.shape[1] * c.weight.shape[2] * c.weight.shape[3]
    c.weight.data = torch.randn(c.weight.shape, generator=g) * math.sqrt(2.0 / fan_in)


def seed_blocks(blocks, g):
    for blk in blocks:
        for cn, bn, lo, hi in (("conv1", "bn1", 0.5, 1.5), ("conv2", "bn2", 0.5, 1.5), ("conv3", "bn3", 0.1, 0.3)):
            _fill_conv(getattr(blk, cn), g)
            _fill_norm(getattr(blk, bn), lo, hi, g)
        if blk.downsample is not None:
            _fill_conv(blk.downsample[0], g)
            _fill_norm(blk.downsample[1], 0.5, 1.5, g)


def seed_resnet(net, seed=SEED):
    """the seeded recipe on every block of layer1 .. layer4 (and the stem)"""
    g = torch.Generator().manual_seed(seed)
    _fill_conv(net.conv1, g)
    _fill_norm(net.bn1, 0.5, 1.5, g)
    for i in range(1, 5):
        seed_blocks(getattr(net, f"layer{i}"), g)
    return net.eval()


class Stage(nn.Module):
    """one level on its own, under the name ResNetStages.from_module(levels=(1, 1)) reads"""

    def __init__(self, blocks):
        super().__init__()
        self.layer1 = nn.Sequential(*blocks)


G22_SHAPE = (2, 64, 9, 7)


def g22_stage(norm=FrozenBN, seed=22):
    """the fixture's case (tests/golden/make_golden_resnet.py): one two-block stage with stride 2 and a downsample, 64 -> 256 channels, on
    2 x 64 x 9 x 7; `norm`: the norm class (the generator passes the reference's own)"""
    down = nn.Sequential(nn.Conv2d(64, 256, 1, stride=2, bias=False), norm(256))
    stage = Stage([Bottleneck(64, 64, 2, down, norm=norm), Bottleneck(256, 64, norm=norm)])
    seed_blocks(stage.layer1, torch.Generator().manual_seed(seed))
    return stage.eval(), stage_input(*G22_SHAPE, seed=seed)


def make_resnet(blocks=(3, 4, 6, 3), planes=(64, 128, 256, 512), strides=(1, 2, 2, 2), seed=SEED, **kw):
    return seed_resnet(ResNet(blocks, planes, strides, **kw), seed)


def small_resnet(stride_on_conv1=False, seed=SEED):
    """the stand-in of the stage tests: blocks (2, 2, 1, 2), planes (64, 128, 64, 128), strides (1, 2, 2, 2)"""
    return make_resnet((2, 2, 1, 2), (64, 128, 64, 128), (1, 2, 2, 2), seed, stride_on_conv1=stride_on_conv1)


def stage_input(B, C, H, W, seed=SEED):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.relu(torch.randn(B, C, H, W, generator=g))


def all_blocks(net):
    return [b for i in range(1, 5) for b in getattr(net, f"layer{i}")]


# ---- single-convolution cases --------------------------------------------------------------------------------------------------------
FAMILIES = ("relu", "outlier", "cancel", "ints", "pow2", "nan")
# every product and partial sum is a number fp32 holds, so any summation order gives the same accumulator; scale, bias and the identity
# stay arbitrary fp32 numbers - the fmaf and the add round once each, the same in any order
EXACT = ("ints", "pow2")
SMALL = ((1, 1, 1), (1, 2, 3), (2, 5, 7), (3, 13, 9), (1, 8, 8))


def out_size(H, R, stride):
    return (H + 2 * ((R - 1) // 2) - R) // stride + 1


def nan_pixels(B, H, W):
    """one interior and one corner pixel (the same pixel where the image has one)"""
    return [(B - 1, H // 2, W // 2), (0, H - 1, W - 1)]


def make_conv_case(family, B, H, W, Cin, Cout, R, stride, epi, seed=SEED):
    """x fp32 [B, Cin, H, W], w [Cout, Cin, R, R], the norm's four vectors with eps (scale / bias follow in resnet_bound.scale_bias), the
    fp32 identity [B, Cout, Ho, Wo] of epilogue 3."""
    g = torch.Generator().manual_seed(seed * 7919 + zlib.crc32(repr((family, B, H, W, Cin, Cout, R, stride, epi)).encode()) % 100003)
    Ho, Wo = out_size(H, R, stride), out_size(W, R, stride)
    fan_in = Cin * R * R
    if family in ("relu", "nan"):
        x = torch.relu(torch.randn(B, Cin, H, W, generator=g))
        w = torch.randn(Cout, Cin, R, R, generator=g) * math.sqrt(2.0 / fan_in)
    elif family == "outlier":      # a sixteenth of the channels carries 60 times the rest
        x = torch.relu(torch.randn(B, Cin, H, W, generator=g))
        x[:, torch.randperm(Cin, generator=g)[: max(1, Cin // 16)]] *= 60.0
        w = torch.randn(Cout, Cin, R, R, generator=g) * math.sqrt(2.0 / fan_in)
    elif family == "cancel":       # channel pairs with equal x and opposite w: the products cancel to a remainder 1e-3 of their size
        h = torch.relu(torch.randn(B, Cin // 2, H, W, generator=g)) + 0.5
        x = torch.cat([h, h * (1 + 1e-3 * torch.randn(h.shape, generator=g))], 1)
        v = torch.randn(Cout, Cin // 2, R, R, generator=g) * math.sqrt(2.0 / fan_in)
        w = torch.cat([v, -v * (1 + 1e-3 * torch.randn(v.shape, generator=g))], 1)
    elif family == "ints":         # |sum| <= 4608 x 16 < 2^24
        x = torch.randint(0, 5, (B, Cin, H, W), generator=g).float()
        w = torch.randint(-4, 5, (Cout, Cin, R, R), generator=g).float()
    elif family == "pow2":         # products 2^-4 .. 2^4: sums are multiples of 2^-4 below 4608 x 16, 21 bits
        x = torch.exp2(torch.randint(-2, 3, (B, Cin, H, W), generator=g).float())
        w = torch.exp2(torch.randint(-2, 3, (Cout, Cin, R, R), generator=g).float()) * (torch.randint(0, 2, (Cout, Cin, R, R), generator=g).float() * 2 - 1)
    else:
        raise ValueError(family)
    if family == "nan":
        for b, y, xx in nan_pixels(B, H, W):
            x[b, (7 * b + y) % Cin, y, xx] = float("nan")
    c = dict(family=family, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, stride=stride, epi=epi, Ho=Ho, Wo=Wo, x=x, w=w)
    lo, hi = (0.1, 0.3) if epi == 3 else (0.5, 1.5)
    c["norm"] = (torch.empty(Cout).uniform_(lo, hi, generator=g), torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1,
                 torch.empty(Cout).uniform_(0.5, 1.5, generator=g), 1e-5)
    c["identity"] = torch.relu(torch.randn(B, Cout, Ho, Wo, generator=g)) if epi == 3 else None
    return c


def without_nan(c):
    """the same case with the NaN pixels' values put back to 0.5"""
    d = dict(c)
    d["x"] = torch.where(torch.isnan(c["x"]), torch.full_like(c["x"], 0.5), c["x"])
    d["family"] = "relu"
    return d
