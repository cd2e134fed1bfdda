"""Seeded inputs for the ResNet stem (hoigen_amd/csrc/hg_resnet_stem.hip, hoigen_amd/resnet.py ResNetStem): the input families of the
one-launch tests and the shapes they run at.  torch on the CPU only.  No GPU, no library.

A case is dict(family, B, Hi, Wi, x fp32 [B, 3, Hi, Wi], w fp32 [64, 3, 7, 7], norm = (weight, bias, running_mean, running_var, eps)).
The recipe of the parameters is tests/resnet_cases.py's: weights N(0, 2 / fan_in), norm weight U(0.5, 1.5), bias and running_mean
N(0, 0.1), running_var U(0.5, 1.5)."""
import math
import zlib

import torch

SEED = 21
FAMILIES = ("image", "outlier", "cancel", "negnorm", "ints", "pow2", "nan")
# every product and partial sum is a number fp32 holds (147 x 16 < 2^24), so any summation order gives the same accumulator; scale and
# bias stay arbitrary fp32 numbers - the fmaf rounds once, the same in any order
EXACT = ("ints", "pow2")
# (B, Hi, Wi): Hc and Wc even and odd, a pooled last row with one and with two valid conv rows, one pixel
SHAPES = ((1, 1, 1), (1, 2, 3), (1, 3, 2), (2, 7, 9), (3, 13, 18), (1, 37, 45))
G23_SHAPE = (2, 3, 37, 45)


def conv_size(Hi):
    return (Hi - 1) // 2 + 1


def pool_size(Hc):
    return (Hc - 1) // 2 + 1


def out_hw(Hi, Wi):
    return pool_size(conv_size(Hi)), pool_size(conv_size(Wi))


def nan_pixels(B, Hi, Wi):
    """one interior and one corner pixel (the same pixel where the image has one): (image, channel, row, column)"""
    return [(B - 1, 1, Hi // 2, Wi // 2), (0, 2, Hi - 1, Wi - 1)]


def make_stem_case(family, B, Hi, Wi, seed=SEED):
    g = torch.Generator().manual_seed(seed * 7919 + zlib.crc32(repr((family, B, Hi, Wi)).encode()) % 100003)
    std = math.sqrt(2.0 / 147)
    if family in ("image", "negnorm", "nan"):      # a normalised image: N(0, 1.2)
        x = torch.randn(B, 3, Hi, Wi, generator=g) * 1.2
        w = torch.randn(64, 3, 7, 7, generator=g) * std
    elif family == "outlier":                      # one channel carries 60 times the rest
        x = torch.randn(B, 3, Hi, Wi, generator=g) * 1.2
        x[:, int(torch.randint(0, 3, (1,), generator=g))] *= 60.0
        w = torch.randn(64, 3, 7, 7, generator=g) * std
    elif family == "cancel":                       # a nearly flat image under tap pairs (s, s + 1) of opposite weights: the products cancel to 1e-3
        x = 1.0 + 1e-3 * torch.randn(B, 3, Hi, Wi, generator=g)
        w = torch.randn(64, 3, 7, 7, generator=g) * std
        w[..., 1:6:2] = -w[..., 0:6:2] * (1 + 1e-3 * torch.randn(64, 3, 7, 3, generator=g))
    elif family == "ints":                         # |sum| <= 147 x 16 < 2^24
        x = torch.randint(-4, 5, (B, 3, Hi, Wi), generator=g).float()
        w = torch.randint(-4, 5, (64, 3, 7, 7), generator=g).float()
    elif family == "pow2":                         # products 2^-4 .. 2^4: sums are multiples of 2^-4 below 147 x 16
        sign = lambda shape: torch.randint(0, 2, shape, generator=g).float() * 2 - 1      # noqa: E731
        x = torch.exp2(torch.randint(-2, 3, (B, 3, Hi, Wi), generator=g).float()) * sign((B, 3, Hi, Wi))
        w = torch.exp2(torch.randint(-2, 3, (64, 3, 7, 7), generator=g).float()) * sign((64, 3, 7, 7))
    else:
        raise ValueError(family)
    if family == "nan":
        for b, c, y, xx in nan_pixels(B, Hi, Wi):
            x[b, c, y, xx] = float("nan")
    weight = torch.empty(64).uniform_(0.5, 1.5, generator=g)
    if family == "negnorm":                        # every other channel's norm weight is negative: the norm does not commute with the max
        weight[1::2] *= -1.0
    norm = (weight, torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1, torch.empty(64).uniform_(0.5, 1.5, generator=g), 1e-5)
    return dict(family=family, B=B, Hi=Hi, Wi=Wi, x=x, w=w, norm=norm)


def without_nan(c):
    """the same case with the NaN pixels' values put back to 0.5"""
    d = dict(c)
    d["x"] = torch.where(torch.isnan(c["x"]), torch.full_like(c["x"], 0.5), c["x"])
    d["family"] = "image"
    return d


def case_of_module(net, x, family="image"):
    """the case of a module with conv1 / bn1 (tests/resnet_cases.py's ResNet) on the images x"""
    n = net.bn1
    return dict(family=family, B=x.shape[0], Hi=x.shape[2], Wi=x.shape[3], x=x, w=net.conv1.weight.detach(),
                norm=(n.weight, n.bias, n.running_mean, n.running_var, float(getattr(n, "eps", 1e-5))))


def g23_input(seed=23):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(*G23_SHAPE, generator=g) * 1.2
