"""Host-side behaviour of hoigen_amd.resnet.ResNetStages / NativeBody and of Detector's native_stages keyword that needs no device:
every refusal of from_module with its message, hg_resnet_out_shape against the output shapes of torch's own convolutions, the exported symbols, and
Detector.from_module without the keyword building exactly what it built before."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import resnet_cases as rc
from hoigen_amd import _lib
from hoigen_amd.detr import Detector, NativeBody, ResNetStages
from hoigen_amd import resnet as hr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small(**kw):
    return rc.small_resnet(**kw)


def test_from_module_reads_the_levels_and_both_stride_placements():
    for on1 in (False, True):
        net = small(stride_on_conv1=on1)
        m = ResNetStages.from_module(net)
        assert m.level_names == ["layer1", "layer2", "layer3", "layer4"] and m.level_ends == [1, 3, 4, 6] and m.in_channels == 64
        blocks = m.blocks()
        assert len(blocks) == 7 and m.training is False
        b = blocks[2]      # layer2.0: the stride sits where the module has it
        assert (b.conv1.desc.stride[0], b.conv2.desc.stride[0]) == ((2, 1) if on1 else (1, 2))
        assert b.downsample is not None and b.downsample[0].desc.stride == (2, 2) and blocks[1].downsample is None
        assert torch.equal(b.conv2.weight, net.layer2[0].conv2.weight) and b.conv2.weight is not net.layer2[0].conv2.weight
        assert b.bn3.eps == 1e-5 and torch.equal(b.bn3.running_var, net.layer2[0].bn3.running_var)
    # the IntermediateLayerGetter around it: a ModuleDict of the children up to layer4
    getter = nn.ModuleDict({k: v for k, v in net.named_children()})
    assert len(ResNetStages.from_module(getter).blocks()) == 7
    # a range of levels; nn.BatchNorm2d in eval() with its own eps
    assert ResNetStages.from_module(net, levels=(4, 4)).in_channels == 256
    bn = rc.make_resnet((1, 1, 1, 1), (64, 64, 64, 64), norm=lambda n: nn.BatchNorm2d(n, eps=1e-3))
    assert ResNetStages.from_module(bn).blocks()[0].bn1.eps == 1e-3


def refused(net, pattern, **kw):
    with pytest.raises(RuntimeError, match=pattern):
        ResNetStages.from_module(net, **kw)


def test_from_module_refuses_what_the_loader_would():
    net = small()
    net.layer1[1] = rc.BasicBlock(256)
    refused(net, r"layer1\.1 \(BasicBlock\) has no conv3: BasicBlock \(resnet18 / resnet34\) is not implemented")
    bn = rc.make_resnet((1, 1, 1, 1), (64, 64, 64, 64), norm=nn.BatchNorm2d)
    bn.train()
    refused(bn, r"layer1\.0\.bn1 \(BatchNorm2d\) is in training mode and would normalise with batch statistics")
    net = small(); net.layer2[0].bn2 = nn.GroupNorm(1, 128)
    refused(net, r"layer2\.0\.bn2 \(GroupNorm\) has no \['running_mean', 'running_var'\]")
    net = small(); del net.layer3
    refused(net, r"the body \(ResNet\) has no layer3")
    refused(small(), r"levels = \(3, 2\)", levels=(3, 2))

    def conv(net, path, new):
        blk = net.layer2[0]
        setattr(blk, path, new) if path != "downsample" else blk.downsample.__setitem__(0, new)
        return net

    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 3, stride=2, padding=2, dilation=2, bias=False)),
            r"layer2\.0\.conv2: dilation \(2, 2\); only dilation 1 is implemented \(the reference's --dilation, DC5, is off by default\)")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 3, stride=2, padding=1, groups=2, bias=False)), r"layer2\.0\.conv2: groups = 2")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 3, stride=2, padding=1, bias=True)), r"layer2\.0\.conv2: the convolution has a bias")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 5, stride=2, padding=2, bias=False)), r"layer2\.0\.conv2: a 5 x 5 kernel; only 1 x 1 and 3 x 3")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, (1, 3), stride=2, padding=(0, 1), bias=False)), r"layer2\.0\.conv2: a 1 x 3 kernel")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 3, stride=2, padding=0, bias=False)), r"layer2\.0\.conv2: padding \(0, 0\) under a 3 x 3 kernel")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 3, stride=3, padding=1, bias=False)), r"layer2\.0\.conv2: stride \(3, 3\); only 1 and 2")
    refused(conv(small(), "conv2", nn.Conv2d(128, 128, 3, stride=(2, 1), padding=1, bias=False)), r"layer2\.0\.conv2: stride \(2, 1\)")
    refused(conv(small(), "conv1", nn.Conv2d(256, 96, 1, bias=False)), r"layer2\.0\.conv1: 256 -> 96 channels; both must be multiples of 64 up to 2048")
    refused(conv(small(), "conv3", nn.Conv2d(128, 4096, 1, bias=False)), r"layer2\.0\.conv3: 128 -> 4096 channels")
    refused(conv(small(), "conv1", nn.Conv2d(256, 192, 1, bias=False)), r"layer2\.0\.bn1 has 128 channels, its convolution gives 192")
    net = conv(small(), "conv1", nn.Conv2d(256, 192, 1, bias=False)); net.layer2[0].bn1 = rc.FrozenBN(192)
    refused(net, r"layer2\.0: the channels do not chain \(conv1 256 -> 192, conv2 128 -> 128, conv3 128 -> 512\)")
    net = small(); net.layer3[0].conv1 = nn.Conv2d(128, 64, 1, bias=False); net.layer3[0].downsample[0] = nn.Conv2d(128, 256, 1, stride=2, bias=False)
    refused(net, r"layer3\.0 takes 128 channels, its predecessor gives 512")
    refused(conv(small(), "conv1", nn.Linear(256, 128)), r"layer2\.0\.conv1 has no \[Cout, Cin, k, k\] weight")
    refused(conv(small(), "downsample", nn.Conv2d(256, 512, 1, stride=1, bias=False)),
            r"layer2\.0\.downsample\.0 is 1 x 1, 256 -> 512 at stride 1; the block needs 1 x 1, 256 -> 512 at stride 2")
    wide = rc.make_resnet((1, 1, 1, 1), (64, 128, 256, 1024), seed=3)      # a 3 x 3 over 1 024 channels
    wide.layer4[0].conv3 = nn.Conv2d(1024, 2048, 1, bias=False); wide.layer4[0].bn3 = rc.FrozenBN(2048)
    wide.layer4[0].downsample = nn.Sequential(nn.Conv2d(1024, 2048, 1, stride=2, bias=False), rc.FrozenBN(2048))
    refused(wide, r"layer4\.0\.conv2: a 3 x 3 kernel over 1024 input channels, at most 512")
    net = small(); net.layer2[0].downsample = None
    refused(net, r"layer2\.0 has no downsample, and maps 256 channels to 512 at stride 2: the identity does not fit")
    net = small(); net.layer2[0].downsample = nn.Sequential(net.layer2[0].downsample[0])
    refused(net, r"layer2\.0\.downsample has 1 children")
    many = rc.ResNet((17, 16, 16, 16), (64, 64, 64, 64), (1, 1, 1, 1))
    refused(many, r"65 blocks, at most 64")


def test_forward_refuses_host_tensors_and_gradient_callers():
    m = ResNetStages.from_module(small())
    with pytest.raises(RuntimeError, match="must be on a HIP device"):
        m(torch.zeros(1, 64, 4, 4))
    body = NativeBody.from_module(small())
    assert isinstance(body.stem[0], nn.Conv2d) and isinstance(body.stem[3], nn.MaxPool2d) and body.training is False
    with pytest.raises(RuntimeError, match=r"NativeBody.from_module: the body \(Sequential\) has no"):
        NativeBody.from_module(nn.Sequential())
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference-only"):
            m(torch.zeros(1, 64, 4, 4, requires_grad=True))


@pytest.mark.parametrize("on1", [False, True])
def test_out_shape_is_conv2ds(on1):
    net = small(stride_on_conv1=on1)
    m = ResNetStages.from_module(net)
    blocks = rc.all_blocks(net)
    probes = [nn.Sequential(*[nn.Conv2d(1, 1, c.kernel_size, c.stride, c.padding) for c in (b.conv1, b.conv2, b.conv3)]) for b in blocks]
    for H in range(1, 71):
        W = 71 - H
        t = torch.zeros(1, 1, H, W)
        for i, p in enumerate(probes):
            t = p(t)
            assert m.out_shape(H, W, 0, i) == (blocks[i].conv3.out_channels, t.shape[2], t.shape[3]), (H, W, i)
        assert m.out_shape(H, W) == m.out_shape(H, W, 0, 6)
    assert m.out_shape(13, 18, 2, 4) == (256, 4, 5) and m.out_shape(13, 18) == (512, 2, 3)
    for bad in ((0, 7), (3, 2), (-1, 2)):
        with pytest.raises(RuntimeError, match="hg_resnet_out_shape"):
            m.out_shape(8, 8, *bad)
    with pytest.raises(RuntimeError, match="hg_resnet_out_shape"):
        m.out_shape(0, 8)


def test_the_abi_is_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hg_load_resnet_stages", "hg_resnet_stages", "hg_resnet_out_shape", "hg_test_resnet_conv"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"int {name}\(", hdr), name
    assert re.search(r"#define HG_PROF_RESNET_CONV (\d+)", hdr).group(1) == str(_lib.HG_PROF_RESNET_CONV)
    kinds = [int(v) for v in re.findall(r"#define HG_PROF_[A-Z_0-9]+ \(?(-?\d+)\)?", hdr)]
    assert len(kinds) == len(set(kinds)), "profiler ids are unique"
    # struct layouts: field counts and sizes as the header spells them (LP64)
    assert ctypes.sizeof(_lib.hg_resnet_conv) == 8 + 12 * 4 and ctypes.sizeof(_lib.hg_resnet_norm) == 5 * 8
    assert ctypes.sizeof(_lib.hg_resnet_block) == 4 * 56 + 4 * 40 + 8 and ctypes.sizeof(_lib.hg_resnet_args) == 8 + 24 + 12 + 8 + 4 + 8 + 16 + 8
    assert ctypes.sizeof(_lib.hg_test_resnet_conv_args) == 7 * 8 + 9 * 4 + 4
    assert (_lib.HG_RESNET_MAX_C, _lib.HG_RESNET_MAX_C3, _lib.HG_RESNET_MAX_SIDE, _lib.HG_RESNET_MAX_B, _lib.HG_RESNET_MAX_BLOCKS) == \
        tuple(int(v) for v in re.search(r"RESNET_MAX_C = (\d+), RESNET_MAX_C3 = (\d+), RESNET_MAX_SIDE = (\d+), RESNET_MAX_B = (\d+), RESNET_MAX_BLOCKS = (\d+)",
                                         open(os.path.join(REPO, "hoigen_amd", "csrc", "hg_kernels.h")).read()).groups())
    assert hr.LEVELS == ("layer1", "layer2", "layer3", "layer4")


class _Sine(nn.Module):
    num_pos_feats, temperature, normalize, scale = 64, 10000.0, True, 6.283185307179586


class _Joiner(nn.Sequential):
    pass


class _Backbone(nn.Module):
    def __init__(self, body):
        super().__init__()
        self.body = body


def stand_in_detector(net, d_model=128):
    """a detector by the reference's attribute names around a stand-in ResNet"""
    from hoigen_amd.detr import BoxMLP, Transformer
    det = nn.Module()
    det.backbone = _Joiner(_Backbone(net), _Sine())
    det.input_proj = nn.Conv2d(net.num_channels, d_model, 1)
    det.transformer = Transformer(d_model, 4, 1, 1, 128)
    det.class_embed = nn.Linear(d_model, 12)
    det.bbox_embed = BoxMLP(d_model)
    det.query_embed = nn.Embedding(5, d_model)
    return det.eval()


def test_detector_keyword_defaults_to_the_torch_body():
    net = small()
    det = stand_in_detector(net)
    d = Detector.from_module(det)
    assert d.body is net and not isinstance(d.body, NativeBody)
    n = Detector.from_module(det, None, native_stages=True)
    assert isinstance(n.body, NativeBody) and n.body.stem[0] is net.conv1 and n.body.stages._ctx is n.neck._ctx is n.transformer.encoder._ctx
    assert [k for k, _ in d.named_children()] == [k for k, _ in n.named_children()] == ["body", "neck", "transformer", "heads", "query_embed"]
    assert list(Detector.from_module.__func__.__defaults__) == [None, False]
