"""hg_test_resnet_stem (hoigen_amd/csrc/hg_resnet_stem.hip: one launch of conv1 -> norm -> ReLU -> max-pool, the loader's weight packing
included) on the device: every output element of every input family inside the per-element bound of tests/stem_bound.py, the exact
families bit for bit, the NaN family's non-finite outputs exactly the reference's and no other bit changed; pooled heights and widths one
below, at, one above and two tiles + 1 of the 4 x 8 tile; NaN canary rows around both outputs; an image of a three-image call equal to the
image alone; an input at an odd float offset that ends where its buffer ends; every refusal launches nothing."""
import ctypes as C

import pytest
import torch

import stem_bound as sb
import stem_cases as sc
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

HG_ERR_INVALID = -1
TH, TW = _lib.HG_RESNET_STEM_TILE


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def run(ctx, c, expect=0, x_dev=None, shape=None, null=None, x_byte_offset=0):
    """one launch on case c -> dict(out32, out16) as CPU fp32 [B, 64, Hp, Wp]; a canary row of NaN in front of and behind both outputs is
    checked.  x_dev: the device tensor to read instead of a fresh copy of c["x"]; shape: (B, Hi, Wi) to claim instead of the case's."""
    lib = _lib.lib()
    B, Hi, Wi = shape or (c["B"], c["Hi"], c["Wi"])
    Hp, Wp = sc.out_hw(max(Hi, 1), max(Wi, 1))
    n = max(B, 1) * Hp * Wp * 64 if expect == 0 else 64
    s, b = sb.scale_bias(c["norm"])
    x = c["x"].contiguous().cuda() if x_dev is None else x_dev
    dev = dict(x=x, w=c["w"].contiguous().cuda(), scale=s.cuda(), bias=b.cuda())
    buf = {k: torch.full((n + 2 * 64,), float("nan"), device="cuda") for k in ("out32", "out16")}
    a = _lib.hg_test_resnet_stem_args()
    for k, t in dev.items():
        setattr(a, k, None if k == null else t.data_ptr() + (x_byte_offset if k == "x" else 0))
    a.out32, a.out16 = (None if k == null else buf[k][64:].data_ptr() for k in ("out32", "out16"))
    a.B, a.Hi, a.Wi = B, Hi, Wi
    rcode = lib.hg_test_resnet_stem(ctx, C.byref(a), None)
    assert rcode == expect, (rcode, lib.hg_last_error(ctx))
    torch.cuda.synchronize()
    out = {}
    for k in ("out32", "out16"):
        h = buf[k].cpu()
        assert torch.isnan(h[:64]).all() and torch.isnan(h[64 + n:]).all(), f"the canary rows around {k} were written"
        if expect:
            assert torch.isnan(h).all(), f"{k} was written"
            out[k] = None
        else:
            out[k] = h[64:64 + n].reshape(B, Hp, Wp, 64).permute(0, 3, 1, 2).contiguous()
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def judge(ctx, c, fails, top, tag):
    got = run(ctx, c)
    f, ratios = sb.check(c, got)
    fails += [f"{tag}: {m}" for m in f]
    top.update({k: max(top.get(k, 0.0), v) for k, v in ratios.items()})
    if c["family"] == "nan":      # no bit outside the NaN's windows changes
        clean = run(ctx, sc.without_nan(c))
        for k, g in got.items():
            if not torch.equal(g[torch.isfinite(g)].view(torch.int32), clean[k][torch.isfinite(g)].view(torch.int32)):
                fails.append(f"{tag}: {k}: a NaN changed an output outside its windows")
    return got


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_family_inside_the_bound(ctx, shape):
    fails, top = [], {}
    for fam in sc.FAMILIES:
        judge(ctx, sc.make_stem_case(fam, *shape), fails, top, f"{fam} {shape}")
    print(f"RESNET_STEM_RATIO {shape}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])


def test_pooled_sizes_around_the_tile_sides(ctx):
    """Hp in {TH - 1, TH, TH + 1, 2 TH + 1} x Wp in {TW - 1, TW, TW + 1, 2 TW + 1} (there is one tile shape, so nothing to force): the
    ragged last tile and the row / column that starts a new one, with Hc and Wc even and odd"""
    fails, top, n = [], {}, 0
    for i, Hp in enumerate((TH - 1, TH, TH + 1, 2 * TH + 1)):
        for j, Wp in enumerate((TW - 1, TW, TW + 1, 2 * TW + 1)):
            Hi, Wi = 4 * (Hp - 1) + 1 + (i + j) % 4, 4 * (Wp - 1) + 1 + (2 * i + j + 1) % 4
            assert sc.out_hw(Hi, Wi) == (Hp, Wp)
            fam = sc.FAMILIES[(4 * i + j) % len(sc.FAMILIES)]
            judge(ctx, sc.make_stem_case(fam, 1 + (i + j) % 2, Hi, Wi), fails, top, f"{fam} Hp {Hp} Wp {Wp} ({Hi} x {Wi})")
            n += 1
    print(f"RESNET_STEM_RATIO tile edges: {n} launches, worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])


def test_an_image_of_a_batch_equals_the_image_alone(ctx):
    c = sc.make_stem_case("image", 3, 13, 18)
    full = run(ctx, c)
    for b in range(3):
        alone = run(ctx, dict(c, B=1, x=c["x"][b:b + 1]))
        for k, g in full.items():
            assert same_bits(g[b:b + 1], alone[k]), (b, k)


def test_an_odd_width_at_an_odd_float_offset_that_ends_with_its_buffer(ctx):
    """x one float into its buffer (a base that is 4-byte but not 8-byte aligned, rows of an odd width); once ending where the buffer
    ends, once with NaN behind it: a read beyond the last element that reached the arithmetic would show"""
    c = sc.make_stem_case("image", 2, 13, 17)
    want = run(ctx, c)
    n = c["x"].numel()
    for tail in (0, 64):
        flat = torch.full((1 + n + tail,), float("nan"), device="cuda")
        flat[1:1 + n] = c["x"].reshape(-1).cuda()
        view = flat[1:1 + n]
        assert view.data_ptr() % 8 == 4
        got = run(ctx, c, x_dev=view)
        assert same_bits(got["out32"], want["out32"]) and same_bits(got["out16"], want["out16"]), tail


def test_refusals_launch_nothing(ctx):
    c = sc.make_stem_case("image", 1, 2, 3)
    m = _lib.HG_RESNET_STEM_MAX_SIDE
    for shape in ((0, 2, 3), (_lib.HG_RESNET_MAX_B + 1, 2, 3), (1, 0, 3), (1, 2, 0), (1, m + 1, 3), (1, 2, m + 1), (-1, 2, 3)):
        run(ctx, c, expect=HG_ERR_INVALID, shape=shape)
    for null in ("x", "w", "scale", "bias", "out32", "out16"):
        run(ctx, c, expect=HG_ERR_INVALID, null=null)
    run(ctx, c, expect=HG_ERR_INVALID, x_byte_offset=2)
    got = run(ctx, c)      # and the context still works
    assert not sb.check(c, got)[0]
