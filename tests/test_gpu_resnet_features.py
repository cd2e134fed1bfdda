"""The pool + normalise kernel (hoigen_amd/csrc/hg_resnet_pool.hip) alone through hg_test_resnet_pool, and hg_resnet_features through
hoigen_amd.resnet.ResNetFeatures, held to tests/dino_bound.py:

  pooled            the fp32 restatement bit for bit in every family; within B_pool of the float64 mean; the exact family == float64
  features          within elem_bound's l2_normalize bound of the pooled rows the same call returned; NaN for an all-zero image; a NaN
                    image non-finite in its own rows and nowhere else
  canary rows       in front of and behind both outputs
  facade            pooled == the restatement on the map THE SAME CALL returned; map == NativeBody(native_stem=True)'s; every output
                    may be absent; ResNet-50 at 224 x 224 within the 1e-3 relative-L2 contract of the torch fp32 CPU modules
  history           a NaN image leaves the other rows' bits alone; the next clean call == a fresh object's

Lines DINO_RATIO carry the worst |err| / bound."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import dino_bound as db
import resnet_cases as rc
from hoigen_amd import _lib
from hoigen_amd.resnet import NativeBody, ResNetFeatures

pytestmark = pytest.mark.gpu
HG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run_pool(ctx, x, want_pooled=True, want_features=True, expect=0, shape=None):
    """one launch on x [B, HW, C] numpy -> (pooled, features) numpy or None; a NaN canary row around each output is checked"""
    B, HW, Cc = shape or x.shape
    n = max(B, 1) * max(Cc, 1) if expect == 0 else 64
    pad = max(Cc, 64)
    xd = torch.from_numpy(x).cuda()
    buf = [torch.full((n + 2 * pad,), float("nan"), device="cuda") for _ in range(2)]
    ptr = [b[pad:].data_ptr() if w else None for b, w in zip(buf, (want_pooled, want_features))]
    rcode = _lib.lib().hg_test_resnet_pool(ctx, xd.data_ptr(), B, HW, Cc, ptr[0], ptr[1], None)
    assert rcode == expect, (rcode, _lib.lib().hg_last_error(ctx))
    torch.cuda.synchronize()
    out = []
    for b, w in zip(buf, (want_pooled, want_features)):
        h = b.cpu().numpy()
        assert np.isnan(h[:pad]).all() and np.isnan(h[pad + n:]).all(), "a canary row around an output was written"
        if expect or not w:
            assert np.isnan(h).all(), "an output that was not asked for was written"
            out.append(None)
        else:
            out.append(h[pad:pad + n].reshape(B, Cc).copy())
    return out


@pytest.mark.parametrize("shape", db.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_alone_every_family(ctx, shape):
    B, HW, Cc = shape
    fails, top = [], {"pooled": 0.0, "features": 0.0}
    for fam in db.FAMILIES:
        x = db.make_map(fam, B, HW, Cc)
        pooled, feats = run_pool(ctx, x)
        want = db.pool_model(x)
        sp = db.special_image(fam, B)
        if not np.array_equal(bits(pooled)[~np.isnan(want)], bits(want)[~np.isnan(want)]) or not np.array_equal(np.isnan(pooled), np.isnan(want)):
            fails.append(f"{fam}: pooled is not the restatement's bits")
        ok_rows = [b for b in range(B) if not (fam == "nan_image" and b == sp)]
        if ok_rows:
            top["pooled"] = max(top["pooled"], db.worst_pool(pooled[ok_rows], x[ok_rows]))
        if db.is_exact(fam, HW) and not np.array_equal(pooled.astype(np.float64), x.astype(np.float64).mean(1)):
            fails.append(f"{fam}: the exact family is not the float64 mean")
        norm_rows = [b for b in range(B) if b != sp or fam not in ("zero_image", "nan_image")]
        if norm_rows:
            top["features"] = max(top["features"], db.worst_norm(feats, pooled, norm_rows))
        if fam == "zero_image" and not np.isnan(feats[sp]).all():
            fails.append("zero_image: the all-zero image's features are not NaN")
        if fam == "nan_image":
            if np.isfinite(feats[sp]).any() or not np.isnan(pooled[sp, Cc // 2 + 1]):
                fails.append("nan_image: the NaN image's features are finite somewhere")
            if not (np.isfinite(pooled[ok_rows]).all() and np.isfinite(feats[ok_rows]).all()):
                fails.append("nan_image: a NaN reached another image")
    print(f"DINO_RATIO pool {shape}: worst |err| / bound pooled {top['pooled']:.3f}, features {top['features']:.3f}")
    if top["pooled"] > 1.0 or top["features"] > 1.0:
        fails.append(f"outside the bound: {top}")
    assert not fails, "\n".join(fails)


def test_kernel_outputs_may_be_absent_and_refusals_launch_nothing(ctx):
    x = db.make_map("relu", 2, 50, 320)
    both = run_pool(ctx, x)
    p_only = run_pool(ctx, x, want_features=False)
    f_only = run_pool(ctx, x, want_pooled=False)
    assert np.array_equal(bits(p_only[0]), bits(both[0])) and np.array_equal(bits(f_only[1]), bits(both[1]))
    run_pool(ctx, x, want_pooled=False, want_features=False, expect=HG_ERR_INVALID)
    for shape in ((0, 50, 320), (_lib.HG_RESNET_MAX_B + 1, 50, 320), (2, 0, 320), (2, 50, 0), (2, 50, 96), (2, 50, _lib.HG_RESNET_MAX_C + 64),
                  (2, _lib.HG_RESNET_MAX_SIDE ** 2 + 1, 64)):
        run_pool(ctx, x, expect=HG_ERR_INVALID, shape=shape)


# ---- the facade ---------------------------------------------------------------------------------------------------------------------
def with_pool(net):
    """torchvision's last two attributes on the stand-in (resnet_cases has no avgpool / fc: the body never runs them)"""
    net.avgpool = nn.AdaptiveAvgPool2d((1, 1))
    net.fc = nn.Identity()
    return net


def images(B, H, W, seed):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 1.2


def nhwc(fmap):
    B, Cc, H, W = fmap.shape
    return np.ascontiguousarray(fmap.cpu().numpy().reshape(B, Cc, H * W).transpose(0, 2, 1))


@pytest.mark.parametrize("shape", ((2, 3, 64, 64), (3, 3, 33, 47)), ids=lambda s: "x".join(map(str, s)))
def test_facade_small_resnet(shape):
    net = with_pool(rc.small_resnet())
    m = ResNetFeatures.from_module(net).cuda()
    x = images(shape[0], shape[2], shape[3], 7).cuda()
    pooled, feats, fmap = m.forward_all(x)
    assert tuple(pooled.shape) == tuple(feats.shape) == (shape[0], 512) and fmap.shape[:2] == (shape[0], 512)
    want = db.pool_model(nhwc(fmap))
    assert np.array_equal(bits(pooled.cpu().numpy()), bits(want)), "pooled is not the restatement on the map the same call returned"
    r = db.worst_norm(feats.cpu().numpy(), pooled.cpu().numpy())
    print(f"DINO_RATIO facade {shape}: features {r:.3f}")
    assert r <= 1.0
    body = NativeBody.from_module(net, native_stem=True).cuda()
    assert torch.equal(fmap.view(torch.int32), body(x)["0"].view(torch.int32)), "map differs from NativeBody's"
    # each output may be absent, and what stays keeps its bits
    assert torch.equal(m(x).view(torch.int32), pooled.view(torch.int32))
    assert torch.equal(m.normalized(x).view(torch.int32), feats.view(torch.int32))
    p2, f2, m2 = m.forward_all(x, pooled=False, features=False)
    assert p2 is None and f2 is None and torch.equal(m2.view(torch.int32), fmap.view(torch.int32))
    p3, f3, m3 = m.forward_all(x, map=False)
    assert m3 is None and torch.equal(p3.view(torch.int32), pooled.view(torch.int32)) and torch.equal(f3.view(torch.int32), feats.view(torch.int32))
    with pytest.raises(RuntimeError, match="at least one"):
        m.forward_all(x, pooled=False, features=False, map=False)


def test_full_depth_resnet50_at_224():
    net = with_pool(rc.make_resnet())
    x = images(2, 224, 224, 11)
    with torch.no_grad():
        want = net.avgpool(net(x)).flatten(1).double()
    want = want / want.norm(dim=-1, keepdim=True)
    got = ResNetFeatures.from_module(net).cuda().normalized(x.cuda()).cpu().double()
    rel = ((got - want).norm(dim=1) / want.norm(dim=1)).tolist()
    print("DINO_RATIO resnet50 2 x 3 x 224 x 224: relative L2 of the normalised rows against torch fp32 on the CPU " + ", ".join(f"{v:.2e}" for v in rel))
    assert tuple(got.shape) == (2, 2048) and max(rel) < 1e-3


def test_history_nan_image_then_clean():
    net = with_pool(rc.small_resnet())
    m = ResNetFeatures.from_module(net).cuda()
    x = images(3, 40, 40, 13).cuda()
    clean = [t.clone() for t in m.forward_all(x)]
    bad = x.clone()
    bad[1, 2, 17, 23] = float("nan")
    got = m.forward_all(bad)
    for g, c in zip(got, clean):
        assert torch.equal(g[[0, 2]].view(torch.int32), c[[0, 2]].view(torch.int32)), "a NaN image changed another image's rows"
    assert not torch.isfinite(got[1][1]).any() and torch.isnan(got[0][1]).any()
    again = m.forward_all(x)
    fresh = ResNetFeatures.from_module(net).cuda().forward_all(x)
    for a, f, c in zip(again, fresh, clean):
        assert torch.equal(a.view(torch.int32), f.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
