"""hg_test_resnet_conv (hoigen_amd/csrc/hg_resnet_conv.hip: one launch of the bottleneck convolution, the loader's weight packing
included) on the device: every output element of every input family inside the per-element bound of tests/resnet_bound.py, the exact
families bit for bit, the NaN family's non-finite outputs exactly the reference's; both kernel sizes and strides, all three epilogues,
both tile heights with M one below, at and one above them, K = 4 608; NaN canary rows around every output; an image of a three-image
call equal to the same image alone."""
import ctypes as C

import pytest
import torch

import resnet_bound as rb
import resnet_cases as rc
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

HG_ERR_INVALID = -1
CINS, COUTS = (64, 128, 512), (64, 256)
SOFT = ("relu", "outlier", "cancel", "nan")


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def run(ctx, c, tile=0, expect=0):
    """one launch on case c -> dict(out32, out16) as CPU fp32 [B, Cout, Ho, Wo] (None where the epilogue has none); a canary row of NaN in
    front of and behind every output is checked"""
    lib = _lib.lib()
    B, Cout, Ho, Wo, epi = c["B"], c["Cout"], c["Ho"], c["Wo"], c["epi"]
    n = B * Ho * Wo * Cout
    s, b = rb.scale_bias(c["norm"])
    dev = [nhwc(c["x"]).cuda(), c["w"].contiguous().cuda(), s.cuda(), b.cuda()]
    idn = nhwc(c["identity"]).cuda() if epi == 3 else None
    buf = {k: torch.full((n + 2 * Cout,), float("nan"), device="cuda") for k in ("out32", "out16")}
    a = _lib.hg_test_resnet_conv_args()
    a.x, a.w, a.scale, a.bias = (t.data_ptr() for t in dev)
    a.identity = idn.data_ptr() if idn is not None else None
    a.out32 = buf["out32"][Cout:].data_ptr() if epi != 1 else None
    a.out16 = buf["out16"][Cout:].data_ptr() if epi != 2 else None
    a.B, a.H, a.W, a.cin, a.cout, a.k, a.stride, a.epi, a.tile = B, c["H"], c["W"], c["Cin"], Cout, c["R"], c["stride"], epi, tile
    rcode = lib.hg_test_resnet_conv(ctx, C.byref(a), None)
    assert rcode == expect, (rcode, lib.hg_last_error(ctx))
    torch.cuda.synchronize()
    out = {}
    for k, written in (("out32", epi != 1), ("out16", epi != 2)):
        h = buf[k].cpu()
        assert torch.isnan(h[:Cout]).all() and torch.isnan(h[Cout + n:]).all(), f"the canary rows around {k} were written"
        if not written or expect:
            assert torch.isnan(h).all(), f"{k} was written"
            out[k] = None
        else:
            out[k] = h[Cout:Cout + n].reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2).contiguous()
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def judge(ctx, c, tile, fails, top, tag):
    got = run(ctx, c, tile)
    f, ratios = rb.check(c, got)
    fails += [f"{tag} tile {tile}: {m}" for m in f]
    top.update({k: max(top.get(k, 0.0), v) for k, v in ratios.items()})
    if c["family"] == "nan":      # no bit outside the NaN's windows changes
        clean = run(ctx, rc.without_nan(c), tile)
        for k, g in got.items():
            if g is not None and not torch.equal(g[torch.isfinite(g)], clean[k][torch.isfinite(g)]):
                fails.append(f"{tag} tile {tile}: {k}: a NaN changed an output outside its windows")
    return got


@pytest.mark.parametrize("R,stride", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_every_family_at_the_small_shapes_inside_the_bound(ctx, R, stride):
    fails, top, n = [], {}, 0
    combos = [(f, e) for f in rc.FAMILIES for e in (1, 2, 3)]
    for si, (B, H, W) in enumerate(rc.SMALL):
        for ci, Cin in enumerate(CINS):
            for oi, Cout in enumerate(COUTS):
                # every family x epilogue at Cin 64, Cout 64; elsewhere one pair per (shape, Cin, Cout), walking through all of them
                picks = combos if (Cin, Cout) == (64, 64) else [combos[(5 * si + 7 * ci + 11 * oi + 3 * R + stride) % len(combos)]]
                for pi, (fam, epi) in enumerate(picks):
                    c = rc.make_conv_case(fam, B, H, W, Cin, Cout, R, stride, epi)
                    judge(ctx, c, (0, 32, 128)[(pi + si) % 3], fails, top, f"{fam} epi {epi} {(B, H, W)} Cin {Cin} Cout {Cout}")
                    n += 1
    print(f"RESNET_CONV_RATIO R {R} stride {stride}: {n} launches, worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("tile", [32, 128])
def test_pixel_counts_around_a_tile_height(ctx, tile):
    """M = tile - 1, tile, tile + 1 (and two tiles + 1), with the tile height forced: the ragged last tile and the row that starts a new one"""
    fails, top = [], {}
    shapes = {32: ((1, 1, 31), (1, 4, 8), (1, 3, 11), (1, 5, 13)), 128: ((1, 1, 127), (1, 8, 16), (1, 3, 43), (1, 1, 257))}[tile]
    for B, H, W in shapes:
        for R, fam, epi in ((1, "relu", 3), (3, "ints", 1), (3, "relu", 2), (1, "pow2", 3)):
            c = rc.make_conv_case(fam, B, H, W, 64, 64, R, 1, epi)
            judge(ctx, c, tile, fails, top, f"{fam} R {R} epi {epi} {(B, H, W)}")
    print(f"RESNET_CONV_RATIO tile {tile} edges: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])


def test_a_launch_the_rule_gives_128_pixel_tiles(ctx):
    """2 x 64 x 65 pixels x 256 channels: 65 tiles of 128 x 4 column tiles >= 256 work items, the last tile ragged; both tile heights give
    the same bits"""
    fails, top = [], {}
    c = rc.make_conv_case("relu", 2, 64, 65, 64, 256, 3, 1, 3)
    got = judge(ctx, c, 0, fails, top, "relu 3 x 3 epi 3 (2, 64, 65)")
    small = run(ctx, c, 32)
    print("RESNET_CONV_RATIO rule's 128-pixel tiles: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])
    assert same_bits(got["out32"], small["out32"]) and same_bits(got["out16"], small["out16"])


def test_an_image_of_a_batch_equals_the_image_alone(ctx):
    for R, stride, epi in ((3, 1, 3), (3, 2, 1), (1, 2, 2)):
        c = rc.make_conv_case("relu", 3, 13, 9, 128, 64, R, stride, epi)
        full = run(ctx, c)
        for b in range(3):
            d = dict(c, B=1, x=c["x"][b:b + 1], identity=None if c["identity"] is None else c["identity"][b:b + 1])
            alone = run(ctx, d)
            for k, g in full.items():
                if g is not None:
                    assert same_bits(g[b:b + 1], alone[k]), (R, stride, epi, b, k)


def test_refusals_launch_nothing(ctx):
    c = rc.make_conv_case("relu", 1, 2, 3, 64, 64, 1, 1, 2)
    for bad in (dict(Cin=96), dict(Cout=32), dict(R=5), dict(stride=3), dict(epi=4)):
        d = dict(c, **bad)
        d["x"] = torch.zeros(1, max(d["Cin"], 64), 2, 3)
        d["w"] = torch.zeros(max(d["Cout"], 64), max(d["Cin"], 64), 5, 5)
        d["norm"] = tuple(torch.ones(max(d["Cout"], 64)) for _ in range(4)) + (1e-5,)
        d["identity"] = torch.zeros(1, 64, 2, 3)
        run(ctx, d, expect=HG_ERR_INVALID)
    run(ctx, c, tile=64, expect=HG_ERR_INVALID)
