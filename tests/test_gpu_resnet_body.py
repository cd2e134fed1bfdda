"""hg_load_resnet_stem / hg_resnet_stem / hg_resnet_body through hoigen_amd.resnet.ResNetStem and NativeBody(native_stem=True) on the
device, on the stand-in of tests/resnet_cases.py at 2 x 3 x 52 x 70 (stem map 2 x 64 x 13 x 18): the stem inside the per-element bound
of tests/stem_bound.py; the body equal bit for bit to the stem followed by the stages, for the map and every block of the trace; strided,
fp64 and channels_last images; history independence; Detector(native_stages=True, native_stem=True) against the pieces by hand; the
fixture g23 (the reference's own FrozenBatchNorm2d); a full-depth ResNet-50 against torch fp32 inside the 1e-3 contract."""
import os

import numpy as np
import pytest
import torch

import resnet_cases as rc
import stem_bound as sb
import stem_cases as sc
from hoigen_amd.resnet import NativeBody, ResNetStages, ResNetStem

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 52, 70)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_resnet_stem.npz")


def images(*shape, seed=31):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 1.2


@pytest.fixture(scope="module")
def setup():
    """(the torch stand-in, the native stem, stages and body, the images on the device, the stem's map, the body's map and trace) -
    computed once, never changed"""
    net = rc.small_resnet()
    stem, stages, body = ResNetStem.from_module(net).cuda(), ResNetStages.from_module(net).cuda(), NativeBody.from_module(net, native_stem=True).cuda()
    x = images(*SHAPE).cuda()
    smap = stem(x)
    out, trace = body._run_body(x, want_trace=True)
    torch.cuda.synchronize()
    return net, stem, stages, body, x, smap, out, trace


@pytest.fixture(scope="module")
def resnet50():
    return rc.make_resnet()


def test_the_stem_inside_the_bound(setup):
    net, stem, stages, body, x, smap, out, trace = setup
    assert tuple(smap.shape) == (2, 64, 13, 18) == (2,) + stem.out_shape(52, 70)
    ref = sb.reference(sc.case_of_module(net, x.cpu()))
    r, bad = sb.worst(smap.cpu(), ref["want"], ref["b32"])
    print(f"RESNET_STEM facade at {SHAPE}: worst |err| / bound {r:.3f}")
    assert bad == 0 and r <= 1.0


def test_the_body_equals_the_stem_followed_by_the_stages(setup):
    net, stem, stages, body, x, smap, out, trace = setup
    o2, tr2 = stages.forward_trace(smap)
    assert tuple(out.shape) == (2, 512, 2, 3) and len(trace) == len(tr2) == 7
    assert torch.equal(out, o2) and torch.equal(out, trace[-1])
    for i, (a, b) in enumerate(zip(trace, tr2)):
        assert torch.equal(a, b), f"block {i}"
    assert torch.equal(body(x)["0"], out)
    short, _ = body._run_body(x, last_block=3)
    assert torch.equal(short, trace[3])


def test_strided_fp64_and_channels_last_images_give_the_same_bits(setup):
    net, stem, stages, body, x, smap, out, trace = setup
    wide = torch.full((3, 3, 60, 83), 7.0, device="cuda")      # the padded batch a larger view is sliced from
    wide[:2, :, 5:57, 10:80] = x
    xv = wide[:2, :, 5:57, 10:80]
    assert not xv.is_contiguous() and xv.stride(3) == 1 and xv.data_ptr() % 16 != 0
    for variant in (xv, x.double(), x.contiguous(memory_format=torch.channels_last)):
        assert torch.equal(stem(variant), smap) and torch.equal(body(variant)["0"], out)
    big = torch.full((3, 70, 13, 18), float("nan"), device="cuda")
    view = big[:2, 3:67]
    stem(x, out=view)
    assert torch.equal(view, smap) and torch.isnan(big[2]).all() and torch.isnan(big[:, :3]).all() and torch.isnan(big[:, 67:]).all()


def test_history_independence(setup):
    net, stem, stages, body, x, smap, out, trace = setup
    assert torch.equal(stem(x), smap) and torch.equal(body(x)["0"], out)
    other = images(3, 3, 75, 41, seed=5).cuda()
    assert tuple(stem(other).shape) == (3, 64, 19, 11) and torch.isfinite(body(other)["0"]).all()
    assert torch.equal(stem(x), smap) and torch.equal(body(x)["0"], out)
    assert torch.equal(stem(x[1:2]), smap[1:2]) and torch.equal(body(x[1:2])["0"], out[1:2]), "an image of the batch differs from the image alone"


def test_the_detector_with_both_keywords_equals_the_pieces_by_hand():
    from hoigen_amd import detr as hd
    from test_resnet_facade import stand_in_detector
    net = rc.small_resnet()
    detr = stand_in_detector(net)
    gen = torch.Generator().manual_seed(5)
    for p in list(detr.input_proj.parameters()) + list(detr.transformer.parameters()) + list(detr.class_embed.parameters()) + \
            list(detr.bbox_embed.parameters()) + list(detr.query_embed.parameters()):
        p.data = torch.randn(p.shape, generator=gen) * (0.1 if p.dim() == 1 else float(np.prod(p.shape[1:])) ** -0.5)
    detr = detr.cuda().eval()
    det = hd.Detector.from_module(detr, None, native_stages=True, native_stem=True)
    assert isinstance(det.body, NativeBody) and isinstance(det.body.native_stem, ResNetStem)
    imgs = images(2, 3, 52, 72, seed=11).cuda()
    im = torch.zeros(2, 52, 72, dtype=torch.bool, device="cuda")
    im[1, 40:], im[1, :, 60:] = True, True
    sizes = [(52.0, 72.0), (40.0, 60.0)]
    results, hs, memory = det(imgs, im, sizes)
    feats = ResNetStages.from_module(net)(ResNetStem.from_module(net)(imgs))
    assert tuple(feats.shape) == (2, 512, 2, 3) and torch.equal(det.body(imgs)["0"], feats)
    neck = hd.DetectorNeck.from_modules(detr.input_proj, detr.backbone[1])
    tr = hd.Transformer.from_module(detr.transformer)
    heads = hd.DetectionHeads.from_modules(detr.class_embed, detr.bbox_embed)
    src, pos, mask, hw = neck(feats, im)
    hs2, mem2 = tr.forward_tokens(src, mask, detr.query_embed.weight, pos, hw)
    res2 = heads.detect(hs2, sizes)
    assert torch.equal(hs, hs2) and torch.equal(memory, mem2) and not torch.isnan(hs).any()
    for a, b in zip(results, res2):
        assert all(torch.equal(a[k], b[k]) for k in ("scores", "labels", "boxes"))
    # and against the torch body inside the contract on the body's map
    want = net(imgs)
    assert float((feats - want).norm() / want.norm()) < 1e-3


def test_the_native_stem_against_the_fixture(resnet50):
    g = np.load(GOLDEN)
    x, want = torch.from_numpy(g["x"]), torch.from_numpy(g["out"]).double()
    assert torch.equal(torch.from_numpy(g["conv1.weight"]), resnet50.conv1.weight.detach())
    ref = sb.reference(sc.case_of_module(resnet50, x), exact_norm=True)
    got = ResNetStem.from_module(resnet50).cuda()(x.cuda()).cpu().double()
    slack = 4 * float(g["out_fp32_vs_fp64_max_abs"])
    worst = float(((got - want).abs() / (ref["b32"] + slack)).max())
    rel = float((got - want).norm() / want.norm())
    print(f"RESNET g23 native: rel L2 {rel:.2e}, worst |err| / bound {worst:.3f} (bound + 4 x {slack / 4:.1e})")
    assert rel < 1e-3 and worst <= 1.0


def test_full_depth_from_the_image_against_the_fp32_torch_statement(resnet50):
    x = images(2, 3, 32, 32, seed=7)
    with torch.no_grad():
        want = resnet50(x)
    got = NativeBody.from_module(resnet50, native_stem=True).cuda()(x.cuda())["0"].cpu()
    assert tuple(got.shape) == tuple(want.shape) == (2, 2048, 1, 1)
    rel = float((got - want).norm() / want.norm())
    pix = float(((got - want).norm(dim=1) / want.norm(dim=1)).max())
    print(f"RESNET_BODY full-depth ResNet-50 from a 2 x 3 x 32 x 32 image against torch fp32 on the CPU: rel L2 {rel:.2e}, worst pixel {pix:.2e}")
    assert rel < 1e-3
