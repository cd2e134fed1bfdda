"""Host-side behaviour of hoigen_amd.resnet.ResNetStem, of NativeBody's and Detector's native_stem keyword, and of the stem's ABI, that
needs no device: every refusal of ResNetStem.from_module in the loader's words, the keyword's defaults, the exported symbols and their
ctypes signatures, and hg_resnet_stem_out_shape against torch's own shapes."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import resnet_cases as rc
from hoigen_amd import _lib
from hoigen_amd.detr import Detector
from hoigen_amd.resnet import NativeBody, ResNetStem
from test_resnet_facade import stand_in_detector

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOADER = open(os.path.join(REPO, "hoigen_amd", "csrc", "hg_resnet.hip")).read()


def small():
    return rc.small_resnet()


def refused(net, pattern, in_loader=None):
    with pytest.raises(RuntimeError, match=pattern):
        ResNetStem.from_module(net)
    if in_loader:      # the loader's own words
        assert in_loader in LOADER, in_loader


def test_from_module_reads_the_stem():
    net = small()
    m = ResNetStem.from_module(net)
    assert torch.equal(m.conv1.weight, net.conv1.weight) and torch.equal(m.bn1.running_var, net.bn1.running_var) and m.bn1.eps == 1e-5
    assert m.pool == (3, 2, 1, 1, 0) and m.training is False and m.get_option("detr_ffn") is None
    assert m.out_shape(52, 70) == (64, 13, 18) and m.out_shape(800, 1333) == (64, 200, 334)
    w, _ = m._weights(False)
    assert (w.conv1.kh, w.conv1.stride_h, w.conv1.pad_w, w.conv1.cin, w.conv1.cout, w.pool_kernel, w.pool_ceil_mode) == (7, 2, 3, 3, 64, 3, 0)
    with pytest.raises(RuntimeError, match="must be on a HIP device"):
        m(torch.zeros(1, 3, 8, 8))


def test_every_refusal_in_the_loaders_words():
    refused(nn.Sequential(), r"ResNetStem.from_module: the body \(Sequential\) has no \['conv1', 'bn1', 'relu', 'maxpool'\]")
    net = small(); net.conv1 = nn.Conv2d(3, 64, 5, 2, 3, bias=False)
    refused(net, r"conv1: a 5 x 5 kernel; only 7 x 7 is implemented", "a %d x %d kernel; only 7 x 7 is implemented")
    net = small(); net.conv1 = nn.Conv2d(3, 64, 7, 2, 3, dilation=2, bias=False)
    refused(net, r"conv1: dilation \(2, 2\); only dilation 1 is implemented", "dilation (%d, %d); only dilation 1 is implemented")
    net = small(); net.conv1 = nn.Conv2d(3, 63, 7, 2, 3, groups=3, bias=False)
    refused(net, r"conv1: groups = 3; only groups = 1 is implemented", "groups = %d; only groups = 1 is implemented")
    net = small(); net.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=True)
    refused(net, r"conv1: the convolution has a bias; a ResNet's convolutions have none", "the convolution has a bias; a ResNet's convolutions have none")
    net = small(); net.conv1 = nn.Conv2d(3, 64, 7, (2, 1), 3, bias=False)
    refused(net, r"conv1: stride \(2, 1\); only \(2, 2\) is implemented", "stride (%d, %d); only (2, 2) is implemented")
    net = small(); net.conv1 = nn.Conv2d(3, 64, 7, 2, 2, bias=False)
    refused(net, r"conv1: padding \(2, 2\); only \(3, 3\) is implemented", "padding (%d, %d); only (3, 3) is implemented")
    net = small(); net.conv1 = nn.Conv2d(4, 64, 7, 2, 3, bias=False)
    refused(net, r"conv1: 4 -> 64 channels; only 3 -> 64 is implemented", "%d -> %d channels; only 3 -> 64 is implemented")
    net = small(); net.conv1 = nn.Conv2d(3, 128, 7, 2, 3, bias=False); net.bn1 = rc.FrozenBN(128)
    refused(net, r"conv1: 3 -> 128 channels; only 3 -> 64 is implemented")
    pool_words = "only 3 / 2 / 1 with dilation 1 and ceil_mode off is implemented"
    for pool, said in ((nn.MaxPool2d(2, 2, 1), "kernel 2, stride 2, padding 1, dilation 1, ceil_mode 0"),
                       (nn.MaxPool2d(3, 1, 1), "kernel 3, stride 1, padding 1, dilation 1, ceil_mode 0"),
                       (nn.MaxPool2d(3, 2, 0), "kernel 3, stride 2, padding 0, dilation 1, ceil_mode 0"),
                       (nn.MaxPool2d(3, 2, 1, dilation=2), "kernel 3, stride 2, padding 1, dilation 2, ceil_mode 0"),
                       (nn.MaxPool2d(3, 2, 1, ceil_mode=True), "kernel 3, stride 2, padding 1, dilation 1, ceil_mode 1")):
        net = small(); net.maxpool = pool
        refused(net, "maxpool: " + said + "; " + pool_words, pool_words)
    assert "maxpool: kernel %d, stride %d, padding %d, dilation %d, ceil_mode %d; " in LOADER
    net = small(); net.maxpool = nn.Identity()
    refused(net, r"maxpool \(Identity\) has no kernel_size")
    words = "conv1.weight holds a value that is not finite or rounds beyond fp16's range (65504)"
    for bad in (float("nan"), float("inf"), 65520.0, -1e6):
        net = small(); net.conv1.weight.data[5, 1, 2, 3] = bad
        refused(net, re.escape(words), words)
    net = small(); net.conv1.weight.data[5, 1, 2, 3] = 65519.0      # rounds to 65504
    ResNetStem.from_module(net)
    for eps in (-1e-5, 1.5, float("nan")):
        net = small(); net.bn1.eps = eps
        refused(net, r"ResNetStem.from_module: bn1: eps = ", "hg_load_resnet_stem: bn1: eps = %g")
    net = small(); net.bn1.running_var = None
    refused(net, r"ResNetStem.from_module: bn1 \(FrozenBN\) has no \['running_var'\]")
    net = small(); net.bn1 = rc.FrozenBN(32)
    refused(net, r"bn1 has 32 channels, its convolution gives 64")
    net = rc.make_resnet((1, 1, 1, 1), (64, 64, 64, 64), (1, 1, 1, 1), norm=nn.BatchNorm2d).train()
    refused(net, r"ResNetStem.from_module: bn1 \(BatchNorm2d\) is in training mode")
    ResNetStem.from_module(net.eval())


def test_native_stem_needs_native_stages_and_the_defaults_are_todays():
    net = small()
    det = stand_in_detector(net)
    with pytest.raises(RuntimeError, match="native_stem=True needs native_stages=True"):
        Detector.from_module(det, None, native_stem=True)
    d = Detector.from_module(det)
    assert d.body is net
    n = Detector.from_module(det, None, native_stages=True)
    assert isinstance(n.body, NativeBody) and n.body.native_stem is None and n.body.stem[0] is net.conv1 and len(n.body.stem) == 4
    b = NativeBody.from_module(net)
    assert b.native_stem is None and b.stem[0] is net.conv1 and b.stem[3] is net.maxpool
    assert NativeBody.from_module.__func__.__defaults__ == (False,) and Detector.from_module.__func__.__kwdefaults__ == {"native_stem": False}
    s = Detector.from_module(det, None, native_stages=True, native_stem=True)
    assert isinstance(s.body.native_stem, ResNetStem) and len(s.body.stem) == 0
    assert s.body.native_stem._ctx is s.body.stages._ctx is s.neck._ctx is s.transformer.encoder._ctx
    alone = NativeBody.from_module(net, native_stem=True)
    assert alone.native_stem._ctx is alone.stages._ctx and alone.training is False


def test_the_abi_is_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hg_load_resnet_stem", "hg_resnet_stem_out_shape", "hg_resnet_stem", "hg_resnet_body", "hg_test_resnet_stem"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"int {name}\(", hdr), name
    assert re.search(r"#define HG_PROF_RESNET_STEM (\d+)", hdr).group(1) == str(_lib.HG_PROF_RESNET_STEM) == "108"
    kinds = [int(v) for v in re.findall(r"#define HG_PROF_[A-Z_0-9]+ \(?(-?\d+)\)?", hdr)]
    assert len(kinds) == len(set(kinds)), "profiler ids are unique"
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["hg_load_resnet_stem"] == (I, [P, ctypes.POINTER(_lib.hg_resnet_stem_weights)])
    assert _lib.SIGNATURES["hg_resnet_stem"] == (I, [P, ctypes.POINTER(_lib.hg_resnet_stem_args), P])
    assert _lib.SIGNATURES["hg_resnet_body"] == (I, [P, ctypes.POINTER(_lib.hg_resnet_body_args), P])
    assert _lib.SIGNATURES["hg_test_resnet_stem"] == (I, [P, ctypes.POINTER(_lib.hg_test_resnet_stem_args), P])
    # struct layouts: field counts and sizes as the header spells them (LP64)
    assert ctypes.sizeof(_lib.hg_resnet_stem_weights) == 56 + 40 + 5 * 4 + 4
    assert ctypes.sizeof(_lib.hg_resnet_stem_args) == 8 + 24 + 12 + 4 + 8 + 16
    assert ctypes.sizeof(_lib.hg_resnet_body_args) == 8 + 24 + 16 + 8 + 16 + 8
    assert ctypes.sizeof(_lib.hg_test_resnet_stem_args) == 6 * 8 + 3 * 4 + 4
    kern = open(os.path.join(REPO, "hoigen_amd", "csrc", "hg_kernels.h")).read()
    assert _lib.HG_RESNET_STEM_TILE == tuple(int(v) for v in re.search(r"RESNET_STEM_TILE_H = (\d+), RESNET_STEM_TILE_W = (\d+)", kern).groups())
    assert _lib.HG_RESNET_STEM_MAX_SIDE == 4 * _lib.HG_RESNET_MAX_SIDE


def test_out_shape_is_torchs():
    lib = _lib.lib()
    probe = nn.Sequential(nn.Conv2d(1, 1, 7, 2, 3), nn.MaxPool2d(3, 2, 1))
    h, w = ctypes.c_int32(), ctypes.c_int32()
    for Hi in range(1, 41):
        for Wi in range(1, 41):
            assert lib.hg_resnet_stem_out_shape(Hi, Wi, ctypes.byref(h), ctypes.byref(w)) == 0
            t = probe(torch.zeros(1, 1, Hi, Wi))
            assert (h.value, w.value) == (t.shape[2], t.shape[3]), (Hi, Wi)
    for bad in ((0, 5), (5, 0), (-1, 3)):
        assert lib.hg_resnet_stem_out_shape(bad[0], bad[1], ctypes.byref(h), ctypes.byref(w)) != 0
