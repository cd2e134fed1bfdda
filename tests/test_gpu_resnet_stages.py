"""hg_load_resnet_stages / hg_resnet_stages through hoigen_amd.resnet.ResNetStages on the device, on the stand-in of
tests/resnet_cases.py (blocks (2, 2, 1, 2), planes (64, 128, 64, 128), strides (1, 2, 2, 2)) at 2 x 64 x 13 x 18 with the stride on conv2
and on conv1: every block of the trace inside the per-element bound of tests/resnet_bound.py from the block input the launch returned,
and equal bit for bit to its four convolutions launched one by one through hg_test_resnet_conv (which tests/test_gpu_resnet_conv.py holds
to the per-convolution bound); block ranges, strided outputs and inputs, history independence; a full-depth ResNet-50 at 2 x 64 x 8 x 8
against the fp32 torch statement inside the 1e-3 contract; NativeBody inside Detector(native_stages=True) against the modules by hand."""
import numpy as np
import pytest
import torch
from torch import nn

import resnet_bound as rb
import resnet_cases as rc
from hoigen_amd import _lib
from hoigen_amd.resnet import NativeBody, ResNetStages
from test_gpu_resnet_conv import run as run_conv

pytestmark = pytest.mark.gpu

SHAPE = (2, 64, 13, 18)


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


@pytest.fixture(scope="module", params=[False, True], ids=["stride_on_conv2", "stride_on_conv1"])
def setup(request):
    """(the torch stand-in, the native stages, x on the device, the full run's map and trace) - computed once, never changed"""
    net = rc.small_resnet(stride_on_conv1=request.param)
    m = ResNetStages.from_module(net).cuda()
    x = rc.stage_input(*SHAPE).cuda()
    out, trace = m.forward_trace(x)
    torch.cuda.synchronize()
    return net, m, x, out, trace


def conv_case(conv, norm, x, epi, identity=None):
    B, Cin, H, W = x.shape
    R, st = conv.kernel_size[0], conv.stride[0]
    return dict(family="relu", B=B, H=H, W=W, Cin=Cin, Cout=conv.out_channels, R=R, stride=st, epi=epi, Ho=rc.out_size(H, R, st),
                Wo=rc.out_size(W, R, st), x=x, w=conv.weight.detach(), norm=rb._norm_of(norm), identity=identity)


def test_every_block_inside_the_bound_from_its_returned_input(ctx, setup):
    net, m, x, out, trace = setup
    assert torch.equal(out, trace[-1]) and tuple(out.shape) == (2, 512, 2, 3)
    assert [tuple(t.shape[1:]) for t in trace] == [(256, 13, 18)] * 2 + [(512, 7, 9)] * 2 + [(256, 4, 5)] + [(512, 2, 3)] * 2
    t, top = x.cpu(), 0.0
    for i, blk in enumerate(rc.all_blocks(net)):
        got = trace[i].cpu()
        ref = rb.block_reference(blk, t)
        r, bad = rb.worst(got, ref["want"], ref["b32"])
        top = max(top, r)
        assert bad == 0, f"block {i}: {bad} elements outside the bound, worst |err| / bound {r:.3f}"
        # the same block as four launches of the one kernel, each from what the launch before returned
        t1 = run_conv(ctx, conv_case(blk.conv1, blk.bn1, t, 1))["out16"]
        t2 = run_conv(ctx, conv_case(blk.conv2, blk.bn2, t1, 1))["out16"]
        idn = t if blk.downsample is None else run_conv(ctx, conv_case(blk.downsample[0], blk.downsample[1], t, 2))["out32"]
        o = run_conv(ctx, conv_case(blk.conv3, blk.bn3, t2, 3, idn))
        assert torch.equal(o["out32"], got), f"block {i} differs from its convolutions launched one by one"
        t = got
    print(f"RESNET_STAGES_RATIO worst |err| / bound over the blocks, each from its returned input: {top:.3f}")


def test_block_ranges_equal_the_slices_of_the_full_run(setup):
    net, m, x, out, trace = setup
    for first, last in ((0, 0), (0, 3), (2, 4), (4, 6), (6, 6), (1, 1)):
        got = m.forward_blocks(x if first == 0 else trace[first - 1], first, last)
        assert torch.equal(got, trace[last]), (first, last)
    o2, tr2 = m.forward_trace(trace[1], 2, 5)
    assert all(torch.equal(a, b) for a, b in zip(tr2, trace[2:6])) and torch.equal(o2, trace[5])
    layer4 = ResNetStages.from_module(net, levels=(4, 4)).cuda()
    assert torch.equal(layer4(trace[4]), out)
    with pytest.raises(RuntimeError, match=r"x must be \[B, 256, H, W\]"):
        m.forward_blocks(x, 2, 3)


def test_strided_outputs_and_inputs_give_the_same_bits(setup):
    net, m, x, out, trace = setup
    big = torch.full((3, 520, 2, 3), float("nan"), device="cuda")
    view = big[:2, 4:516]
    m(x, out=view)
    assert torch.equal(view, out) and torch.isnan(big[2]).all() and torch.isnan(big[:, :4]).all() and torch.isnan(big[:, 516:]).all()
    wide = torch.zeros(2, 70, 15, 24, device="cuda")
    wide[:, 3:67, 1:14, 2:20] = x
    xv = wide[:, 3:67, 1:14, 2:20]
    assert not xv.is_contiguous() and torch.equal(m(xv), out)
    assert torch.equal(m(x.double()), out) and torch.equal(m(x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)), out)


def test_history_independence(setup):
    net, m, x, out, trace = setup
    assert torch.equal(m(x), out)
    other = m(rc.stage_input(3, 64, 20, 11, seed=5).cuda())
    assert tuple(other.shape) == (3, 512, 3, 2) and torch.isfinite(other).all()
    assert torch.equal(m(x), out)
    alone = m(x[1:2])
    assert torch.equal(alone, out[1:2]), "an image of the batch differs from the image alone"


def test_full_depth_against_the_fp32_torch_statement():
    net = rc.make_resnet()
    x = rc.stage_input(2, 64, 8, 8)
    with torch.no_grad():
        want = net.stages(x)
    m = ResNetStages.from_module(net).cuda()
    got = m(x.cuda()).cpu()
    assert tuple(got.shape) == tuple(want.shape) == (2, 2048, 1, 1)
    rel = float((got - want).norm() / want.norm())
    pix = float(((got - want).norm(dim=1) / want.norm(dim=1)).max())
    print(f"RESNET_STAGES full-depth ResNet-50 at 2 x 64 x 8 x 8 against torch fp32 on the CPU: rel L2 {rel:.2e}, worst pixel {pix:.2e}")
    assert rel < 1e-3 and pix < 1e-3


def test_native_body_inside_the_detector_equals_the_modules_by_hand():
    from hoigen_amd import detr as hd
    from test_resnet_facade import stand_in_detector
    net = rc.small_resnet()
    detr = stand_in_detector(net)
    gen = torch.Generator().manual_seed(5)
    for p in list(detr.input_proj.parameters()) + list(detr.transformer.parameters()) + list(detr.class_embed.parameters()) + \
            list(detr.bbox_embed.parameters()) + list(detr.query_embed.parameters()):
        p.data = torch.randn(p.shape, generator=gen) * (0.1 if p.dim() == 1 else float(np.prod(p.shape[1:])) ** -0.5)
    detr = detr.cuda().eval()
    det = hd.Detector.from_module(detr, None, native_stages=True)
    assert isinstance(det.body, NativeBody)
    imgs = torch.randn(2, 3, 52, 72, generator=torch.Generator().manual_seed(11)).cuda()
    im = torch.zeros(2, 52, 72, dtype=torch.bool, device="cuda")
    im[1, 40:], im[1, :, 60:] = True, True
    sizes = [(52.0, 72.0), (40.0, 60.0)]
    results, hs, memory = det(imgs, im, sizes)
    stem = net.maxpool(net.relu(net.bn1(net.conv1(imgs))))
    assert tuple(stem.shape) == (2, 64, 13, 18)
    feats = ResNetStages.from_module(net)(stem)
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
    # and against the torch body: the same detector without the keyword, inside the contract on the body's map
    want = net.stages(stem)
    assert float((feats - want).norm() / want.norm()) < 1e-3
