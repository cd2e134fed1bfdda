"""ResNet bottleneck stages façade: ``layer1`` .. ``layer4`` of the detector's body - torchvision's ResNet-50 under the reference's
``FrozenBatchNorm2d`` (detr/models/backbone.py:19-55, :83-93; chosen at inference.py:950 and main_tip_finetune.py:1057), which also runs
as the DINO backbone on the 224-pixel crops (upt_tip_cache_model_free_finetune_distill3.py:1617) - on one implicit-GEMM convolution
(hoigen_amd/csrc/hg_resnet_conv.hip: hg_load_resnet_stages, hg_resnet_stages).

    stages = ResNetStages.from_module(self.detector.backbone[0].body)
    body = NativeBody.from_module(self.detector.backbone[0].body)          # torch stem + the native stages, returns {'0': map}

The stem (``conv1`` 7 x 7, ``bn1``, ReLU, max-pool) stays torch by default; ``ResNetStem.from_module(body)`` is its one native launch
(hoigen_amd/csrc/hg_resnet_stem.hip) and ``NativeBody.from_module(body, native_stem=True)`` runs stem and stages as one call
(hg_resnet_body).  ``ResNetFeatures.from_module(net)`` is the whole network as the reference's DINO backbone runs it - stem, stages,
global average pool, ``fc = Identity`` - with the L2 normalisation of :1618 behind it, in one call (hg_resnet_features; the pool and the
norm are one launch, hoigen_amd/csrc/hg_resnet_pool.hip).  torchvision is not imported: the source module is read by its attribute
names.  Inference only; tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from .model import _inference_only, _NativeModule, _require_cuda, _stream_ptr

LEVELS = ("layer1", "layer2", "layer3", "layer4")
_CONVS = (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"))


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class _ConvDesc:
    """The integers of one convolution, as hg_resnet_conv takes them."""

    def __init__(self, name: str, conv: nn.Module):
        w = getattr(conv, "weight", None)
        if w is None or w.dim() != 4:
            raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {name} has no [Cout, Cin, k, k] weight "
                               f"(got {type(conv).__name__}, weight {None if w is None else tuple(w.shape)})")
        self.name = name
        self.cout, cin_g, self.kh, self.kw = (int(v) for v in w.shape)
        self.groups = int(getattr(conv, "groups", 1))
        self.cin = cin_g * self.groups
        self.stride, self.padding, self.dilation = _pair(getattr(conv, "stride", 1)), _pair(getattr(conv, "padding", 0)), _pair(getattr(conv, "dilation", 1))
        self.has_bias = getattr(conv, "bias", None) is not None

    def check(self) -> None:
        """What hg_load_resnet_stages refuses, refused here with the same words (no device needed)."""
        head = f"hoigen_amd: ResNetStages.from_module: {self.name}: "
        k = self.kh
        if self.kh != self.kw or k not in (1, 3):
            raise RuntimeError(head + f"a {self.kh} x {self.kw} kernel; only 1 x 1 and 3 x 3 are implemented")
        if self.dilation != (1, 1):
            raise RuntimeError(head + f"dilation {self.dilation}; only dilation 1 is implemented (the reference's --dilation, DC5, is off by default)")
        if self.groups != 1:
            raise RuntimeError(head + f"groups = {self.groups}; only groups = 1 is implemented")
        if self.has_bias:
            raise RuntimeError(head + "the convolution has a bias; a ResNet's convolutions have none")
        if self.stride[0] != self.stride[1] or self.stride[0] not in (1, 2):
            raise RuntimeError(head + f"stride {self.stride}; only 1 and 2, the same on both axes, are implemented")
        if self.padding != ((k - 1) // 2, (k - 1) // 2):
            raise RuntimeError(head + f"padding {self.padding} under a {k} x {k} kernel; only (k - 1) / 2 is implemented")
        m = _lib.HG_RESNET_MAX_C
        if self.cin < 64 or self.cin % 64 or self.cin > m or self.cout < 64 or self.cout % 64 or self.cout > m:
            raise RuntimeError(head + f"{self.cin} -> {self.cout} channels; both must be multiples of 64 up to {m}")
        if k == 3 and self.cin > _lib.HG_RESNET_MAX_C3:
            raise RuntimeError(head + f"a 3 x 3 kernel over {self.cin} input channels, at most {_lib.HG_RESNET_MAX_C3}")

    def check_stem(self, head: str) -> None:
        """What hg_load_resnet_stem refuses of conv1, refused here with the same words (no device needed)."""
        if (self.kh, self.kw) != (7, 7):
            raise RuntimeError(head + f"a {self.kh} x {self.kw} kernel; only 7 x 7 is implemented")
        if self.dilation != (1, 1):
            raise RuntimeError(head + f"dilation {self.dilation}; only dilation 1 is implemented")
        if self.groups != 1:
            raise RuntimeError(head + f"groups = {self.groups}; only groups = 1 is implemented")
        if self.has_bias:
            raise RuntimeError(head + "the convolution has a bias; a ResNet's convolutions have none")
        if self.stride != (2, 2):
            raise RuntimeError(head + f"stride {self.stride}; only (2, 2) is implemented")
        if self.padding != (3, 3):
            raise RuntimeError(head + f"padding {self.padding}; only (3, 3) is implemented")
        if (self.cin, self.cout) != (3, 64):
            raise RuntimeError(head + f"{self.cin} -> {self.cout} channels; only 3 -> 64 is implemented")

    def struct(self, ptr: Optional[int]) -> "_lib.hg_resnet_conv":
        return _lib.hg_resnet_conv(ptr, self.cout, self.cin, self.kh, self.kw, self.stride[0], self.stride[1], self.padding[0], self.padding[1],
                                   self.dilation[0], self.dilation[1], self.groups, int(self.has_bias))


class FrozenNorm(nn.Module):
    """Holder of a frozen norm's four vectors under the reference's names (backbone.py:32-36) and its eps (:50)."""

    def __init__(self, n: int, eps: float = 1e-5):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self.eps = float(eps)


class ConvWeight(nn.Module):
    """Holder of a convolution's weight and integers; never called."""

    def __init__(self, d: _ConvDesc):
        super().__init__()
        self.register_buffer("weight", torch.empty(d.cout, d.cin, d.kh, d.kw))
        self.desc = d


class BottleneckParams(nn.Module):
    def __init__(self):
        super().__init__()
        self.downsample = None


def _read_norm(name: str, norm: nn.Module, channels: int, who: str = "ResNetStages") -> FrozenNorm:
    missing = [k for k in ("weight", "bias", "running_mean", "running_var") if getattr(norm, k, None) is None]
    if missing:
        raise RuntimeError(f"hoigen_amd: {who}.from_module: {name} ({type(norm).__name__}) has no {missing}: a frozen norm or an "
                           "nn.BatchNorm2d with running statistics is needed")
    if isinstance(norm, nn.modules.batchnorm._BatchNorm) and norm.training:
        raise RuntimeError(f"hoigen_amd: {who}.from_module: {name} ({type(norm).__name__}) is in training mode and would normalise with "
                           "batch statistics; call eval() on the body first (the reference freezes its norms, backbone.py:19-55)")
    if int(norm.weight.numel()) != channels:
        raise RuntimeError(f"hoigen_amd: {who}.from_module: {name} has {int(norm.weight.numel())} channels, its convolution gives {channels}")
    eps = float(getattr(norm, "eps", 1e-5))      # FrozenBatchNorm2d holds no eps attribute: 1e-5 inside forward (backbone.py:50)
    if not (0.0 <= eps <= 1.0):
        raise RuntimeError(f"hoigen_amd: {who}.from_module: {name}: eps = {eps}")
    m = FrozenNorm(channels, eps)
    for k in ("weight", "bias", "running_mean", "running_var"):
        getattr(m, k).data = getattr(norm, k).detach().to(torch.float32).clone()
    return m


class ResNetStages(_NativeModule):
    """``layer1`` .. ``layer4`` (or a range of them) of a bottleneck ResNet in one native call.  ``forward(x)`` takes the stem's
    ``[B, 64, H, W]`` map and returns the last level's map - ``[B, 2048, H / 8, W / 8]`` for ResNet-50's four levels (each stride-2 level
    gives ``(H - 1) // 2 + 1``) - as fp32 NCHW; ``forward_trace`` also returns every block's output.  Arithmetic: fp16 operands, fp32
    accumulation in a fixed order, the norm as one ``fmaf`` on fp32 scale / bias made in double, the identity chain in fp32 (DESIGN.md
    section 20)."""

    def __init__(self):
        super().__init__()
        self.level_names: List[str] = []
        self.level_ends: List[int] = []      # index of each level's last block

    @classmethod
    def from_module(cls, body: nn.Module, levels: Tuple[int, int] = (1, 4)) -> "ResNetStages":
        """From a torchvision-style ResNet or the ``IntermediateLayerGetter`` around it: attributes ``layer1`` .. ``layer4``, every block
        with ``conv1, bn1, conv2, bn2, conv3, bn3`` and an optional ``downsample`` of two children.  ``levels = (first, last)``, 1-based
        and inclusive, selects a range (``(4, 4)``: ``layer4`` alone, fed with ``layer3``'s map)."""
        first, last = int(levels[0]), int(levels[1])
        if not (1 <= first <= last <= 4):
            raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: levels = {tuple(levels)}; 1 <= first <= last <= 4")
        m = cls()
        n_blocks, prev_cout, device, training = 0, None, None, False
        for name in LEVELS[first - 1:last]:
            level = getattr(body, name, None)
            if level is None:
                raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: the body ({type(body).__name__}) has no {name}")
            blocks = nn.ModuleList()
            for i, blk in enumerate(level):
                where = f"{name}.{i}"
                if not hasattr(blk, "conv3"):
                    raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where} ({type(blk).__name__}) has no conv3: BasicBlock "
                                       "(resnet18 / resnet34) is not implemented, only the bottleneck block of resnet50 / 101 / 152")
                p = BottleneckParams()
                for cn, bn in _CONVS:
                    if not hasattr(blk, cn) or not hasattr(blk, bn):
                        raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where} ({type(blk).__name__}) has no {cn} / {bn}")
                    d = _ConvDesc(f"{where}.{cn}", getattr(blk, cn))
                    d.check()
                    holder = ConvWeight(d)
                    holder.weight.data = getattr(blk, cn).weight.detach().to(torch.float32).clone()
                    setattr(p, cn, holder)
                    setattr(p, bn, _read_norm(f"{where}.{bn}", getattr(blk, bn), d.cout))
                c1, c2, c3 = p.conv1.desc, p.conv2.desc, p.conv3.desc
                if c2.cin != c1.cout or c3.cin != c2.cout:
                    raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where}: the channels do not chain (conv1 {c1.cin} -> {c1.cout}, "
                                       f"conv2 {c2.cin} -> {c2.cout}, conv3 {c3.cin} -> {c3.cout})")
                stride = c1.stride[0] * c2.stride[0] * c3.stride[0]
                down = getattr(blk, "downsample", None)
                if down is None:
                    if c3.cout != c1.cin or stride != 1:
                        raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where} has no downsample, and maps {c1.cin} channels to "
                                           f"{c3.cout} at stride {stride}: the identity does not fit")
                else:
                    kids = list(down.children()) if isinstance(down, nn.Module) else list(down)
                    if len(kids) != 2:
                        raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where}.downsample has {len(kids)} children; a convolution "
                                           "and a norm are needed")
                    d = _ConvDesc(f"{where}.downsample.0", kids[0])
                    d.check()
                    if d.cin != c1.cin or d.cout != c3.cout or d.stride[0] != stride or d.kh != 1:
                        raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where}.downsample.0 is {d.kh} x {d.kw}, {d.cin} -> {d.cout} at "
                                           f"stride {d.stride[0]}; the block needs 1 x 1, {c1.cin} -> {c3.cout} at stride {stride}")
                    holder = ConvWeight(d)
                    holder.weight.data = kids[0].weight.detach().to(torch.float32).clone()
                    p.downsample = nn.Sequential(holder, _read_norm(f"{where}.downsample.1", kids[1], d.cout))
                if prev_cout is not None and c1.cin != prev_cout:
                    raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {where} takes {c1.cin} channels, its predecessor gives {prev_cout}")
                prev_cout = c3.cout
                device = blk.conv1.weight.device
                training = training or bool(getattr(blk, "training", False))
                blocks.append(p)
                n_blocks += 1
            if not len(blocks):
                raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {name} has no blocks")
            setattr(m, name, blocks)
            m.level_names.append(name)
            m.level_ends.append(n_blocks - 1)
        if n_blocks > _lib.HG_RESNET_MAX_BLOCKS:
            raise RuntimeError(f"hoigen_amd: ResNetStages.from_module: {n_blocks} blocks, at most {_lib.HG_RESNET_MAX_BLOCKS}")
        m.to(device)
        m.train(getattr(body, "training", training))
        return m

    # ---- the blocks in order, and their descriptors
    def blocks(self) -> List[BottleneckParams]:
        return [b for name in self.level_names for b in getattr(self, name)]

    @property
    def in_channels(self) -> int:
        return self.blocks()[0].conv1.desc.cin

    def _descriptors(self, with_pointers: bool):
        """(hg_resnet_weights, what must stay alive while it is used)"""
        blocks = self.blocks()
        arr = (_lib.hg_resnet_block * len(blocks))()
        keep = [arr]

        def ptr(t):
            if not with_pointers:
                return None
            _require_cuda(t, "ResNetStages weights")
            t = t.detach().to(torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        def norm(n):
            return _lib.hg_resnet_norm(ptr(n.weight), ptr(n.bias), ptr(n.running_mean), ptr(n.running_var), n.eps)

        ends = set(self.level_ends)
        for i, b in enumerate(blocks):
            a = arr[i]
            a.conv1, a.conv2, a.conv3 = (getattr(b, cn).desc.struct(ptr(getattr(b, cn).weight)) for cn, _ in _CONVS)
            a.bn1, a.bn2, a.bn3 = norm(b.bn1), norm(b.bn2), norm(b.bn3)
            if b.downsample is not None:
                a.down_conv, a.down_bn, a.has_downsample = b.downsample[0].desc.struct(ptr(b.downsample[0].weight)), norm(b.downsample[1]), 1
            a.ends_level = int(i in ends)
        return _lib.hg_resnet_weights(arr, len(blocks)), keep

    def out_shape(self, H: int, W: int, first_block: int = 0, last_block: Optional[int] = None) -> Tuple[int, int, int]:
        """(C, H, W) behind blocks ``first_block .. last_block`` (default: all) for an ``H x W`` input - hg_resnet_out_shape, pure host."""
        w, keep = self._descriptors(False)
        last = len(keep[0]) - 1 if last_block is None else last_block
        c, h, ww = C.c_int32(), C.c_int32(), C.c_int32()
        rc = _lib.lib().hg_resnet_out_shape(C.byref(w), first_block, last, H, W, C.byref(c), C.byref(h), C.byref(ww))
        if rc:
            raise RuntimeError(f"hoigen_amd: hg_resnet_out_shape({first_block}, {last}, {H}, {W}) failed ({rc})")
        return c.value, h.value, ww.value

    def _sig_terms(self) -> tuple:
        return (tuple((t.data_ptr(), t._version) for t in self.buffers()), tuple(b.bn1.eps for b in self.blocks()))

    def _load_native(self, h: int) -> None:
        w, keep = self._descriptors(True)
        self._ctx.check(_lib.lib().hg_load_resnet_stages(h, C.byref(w)), "hg_load_resnet_stages")

    def _run(self, x: torch.Tensor, first_block: int = 0, last_block: Optional[int] = None, out: Optional[torch.Tensor] = None,
             want_trace: bool = False):
        _require_cuda(x, "ResNetStages x")
        blocks = self.blocks()
        last = len(blocks) - 1 if last_block is None else int(last_block)
        first = int(first_block)
        if not (0 <= first <= last < len(blocks)):
            raise RuntimeError(f"hoigen_amd: ResNetStages: blocks {first} .. {last} of {len(blocks)}")
        cin = blocks[first].conv1.desc.cin
        if x.dim() != 4 or x.shape[1] != cin:
            raise RuntimeError(f"hoigen_amd: ResNetStages: x must be [B, {cin}, H, W] (got {tuple(x.shape)})")
        B, _, H, W = (int(v) for v in x.shape)
        if not (1 <= B <= _lib.HG_RESNET_MAX_B) or not (1 <= H <= _lib.HG_RESNET_MAX_SIDE) or not (1 <= W <= _lib.HG_RESNET_MAX_SIDE):
            raise RuntimeError(f"hoigen_amd: ResNetStages: B = {B} (1 .. {_lib.HG_RESNET_MAX_B}), H x W = {H} x {W} (1 .. {_lib.HG_RESNET_MAX_SIDE} each)")
        x = x.detach()
        if x.dtype != torch.float32 or x.stride(3) != 1:
            x = x.to(torch.float32).contiguous()
        h = self._load(x.device)
        Co, Ho, Wo = self.out_shape(H, W, first, last)
        f32 = dict(device=x.device, dtype=torch.float32)
        if out is None:
            out = torch.empty(B, Co, Ho, Wo, **f32)
        elif tuple(out.shape) != (B, Co, Ho, Wo) or out.dtype != torch.float32 or out.device != x.device or out.stride(3) != 1 or \
                (Ho > 1 and out.stride(2) != Wo):
            raise RuntimeError(f"hoigen_amd: ResNetStages: out must be an fp32 [{B}, {Co}, {Ho}, {Wo}] tensor (or view) on x's device whose "
                               "tokens are contiguous within a channel")
        a = _lib.hg_resnet_args()
        a.x, a.B, a.H, a.W, a.first_block, a.last_block, a.out = x.data_ptr(), B, H, W, first, last, out.data_ptr()
        a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
        a.out_stride[:] = [out.stride(0), out.stride(1)]
        trace = None
        if want_trace:
            trace = [torch.empty(B, *self.out_shape(H, W, first, i), **f32) for i in range(first, last + 1)]
            ptrs = (C.c_void_p * len(trace))(*[t.data_ptr() for t in trace])
            a.trace = ptrs
        self._ctx.check(_lib.lib().hg_resnet_stages(h, C.byref(a), _stream_ptr(x.device)), "hg_resnet_stages")
        return out, trace

    @_inference_only
    @torch.no_grad()
    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x [B, Cin, H, W]`` (fp32 with a column stride of 1 is read where it lies through its strides; anything else is converted
        once) -> the last level's map, fp32 ``[B, C, Ho, Wo]``; ``out``: write into this tensor or view instead."""
        return self._run(x, out=out)[0]

    @_inference_only
    @torch.no_grad()
    def forward_blocks(self, x: torch.Tensor, first_block: int, last_block: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Blocks ``first_block .. last_block`` (inclusive, counted over the loaded levels) on the input of ``first_block``."""
        return self._run(x, first_block, last_block, out)[0]

    @_inference_only
    @torch.no_grad()
    def forward_trace(self, x: torch.Tensor, first_block: int = 0, last_block: Optional[int] = None):
        """``(map, [every block's output])``."""
        return self._run(x, first_block, last_block, want_trace=True)


def _images(x: torch.Tensor, what: str) -> torch.Tensor:
    """``[B, 3, Hi, Wi]`` on a HIP device; fp32 with a column stride of 1 is read where it lies, anything else is converted once"""
    _require_cuda(x, what)
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"hoigen_amd: {what} must be [B, 3, Hi, Wi] (got {tuple(x.shape)})")
    B, _, Hi, Wi = (int(v) for v in x.shape)
    m = _lib.HG_RESNET_STEM_MAX_SIDE
    if not (1 <= B <= _lib.HG_RESNET_MAX_B) or not (1 <= Hi <= m) or not (1 <= Wi <= m):
        raise RuntimeError(f"hoigen_amd: {what}: B = {B} (1 .. {_lib.HG_RESNET_MAX_B}), Hi x Wi = {Hi} x {Wi} (1 .. {m} each)")
    x = x.detach()
    if x.dtype != torch.float32 or x.stride(3) != 1:
        x = x.to(torch.float32).contiguous()
    return x


class ResNetStem(_NativeModule):
    """``conv1`` (7 x 7 / 2, 3 -> 64), ``bn1``, ReLU and the 3 x 3 / 2 max-pool of a ResNet in one native launch
    (hoigen_amd/csrc/hg_resnet_stem.hip).  ``forward(images)`` takes ``[B, 3, Hi, Wi]`` and returns the stem's map, fp32
    ``[B, 64, Hp, Wp]``: what ``ResNetStages`` takes.  Arithmetic: image and weight rounded once to fp16, fp32 accumulation in a fixed
    order, the norm as one ``fmaf``, ReLU, a max that keeps a NaN."""

    def __init__(self):
        super().__init__()
        self.pool = (3, 2, 1, 1, 0)      # kernel, stride, padding, dilation, ceil_mode

    @classmethod
    def from_module(cls, body: nn.Module) -> "ResNetStem":
        """From a torchvision-style ResNet or the ``IntermediateLayerGetter`` around it: attributes ``conv1``, ``bn1``, ``relu``,
        ``maxpool``.  Refuses what hg_load_resnet_stem refuses, in its words, without a device."""
        missing = [k for k in ("conv1", "bn1", "relu", "maxpool") if getattr(body, k, None) is None]
        if missing:
            raise RuntimeError(f"hoigen_amd: ResNetStem.from_module: the body ({type(body).__name__}) has no {missing}")
        head = "hoigen_amd: ResNetStem.from_module: "
        d = _ConvDesc("conv1", body.conv1)
        d.check_stem(head + "conv1: ")
        p = body.maxpool
        if getattr(p, "kernel_size", None) is None:
            raise RuntimeError(head + f"maxpool ({type(p).__name__}) has no kernel_size")

        def one(v):      # an int where both axes agree, else the pair
            a, b = _pair(v)
            return a if a == b else (a, b)

        k = one(p.kernel_size)
        stride = getattr(p, "stride", None)
        flat = (k, k if stride is None else one(stride), one(getattr(p, "padding", 0)), one(getattr(p, "dilation", 1)),
                int(bool(getattr(p, "ceil_mode", False))))
        if flat != (3, 2, 1, 1, 0):
            raise RuntimeError(head + f"maxpool: kernel {flat[0]}, stride {flat[1]}, padding {flat[2]}, dilation {flat[3]}, ceil_mode {flat[4]}; "
                               "only 3 / 2 / 1 with dilation 1 and ceil_mode off is implemented")
        w = body.conv1.weight.detach().to(torch.float32)
        if not bool((w.half().float().abs() <= 65504.0).all()):
            raise RuntimeError(head + "conv1.weight holds a value that is not finite or rounds beyond fp16's range (65504)")
        m = cls()
        m.conv1 = ConvWeight(d)
        m.conv1.weight.data = w.clone()
        m.bn1 = _read_norm("bn1", body.bn1, d.cout, who="ResNetStem")
        m.to(body.conv1.weight.device)
        m.train(getattr(body, "training", False))
        return m

    def _weights(self, with_pointers: bool):
        keep = []

        def ptr(t):
            if not with_pointers:
                return None
            _require_cuda(t, "ResNetStem weights")
            t = t.detach().to(torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        n = self.bn1
        w = _lib.hg_resnet_stem_weights(self.conv1.desc.struct(ptr(self.conv1.weight)),
                                        _lib.hg_resnet_norm(ptr(n.weight), ptr(n.bias), ptr(n.running_mean), ptr(n.running_var), n.eps), *self.pool)
        return w, keep

    @staticmethod
    def out_shape(Hi: int, Wi: int) -> Tuple[int, int, int]:
        """(64, Hp, Wp) of an ``Hi x Wi`` image - hg_resnet_stem_out_shape, pure host."""
        h, w = C.c_int32(), C.c_int32()
        rc = _lib.lib().hg_resnet_stem_out_shape(Hi, Wi, C.byref(h), C.byref(w))
        if rc:
            raise RuntimeError(f"hoigen_amd: hg_resnet_stem_out_shape({Hi}, {Wi}) failed ({rc})")
        return 64, h.value, w.value

    def _sig_terms(self) -> tuple:
        return (tuple((t.data_ptr(), t._version) for t in self.buffers()), self.bn1.eps)

    def _load_native(self, h: int) -> None:
        w, keep = self._weights(True)
        self._ctx.check(_lib.lib().hg_load_resnet_stem(h, C.byref(w)), "hg_load_resnet_stem")

    @_inference_only
    @torch.no_grad()
    def forward(self, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``images [B, 3, Hi, Wi]`` (fp32 with a column stride of 1 is read where it lies through its strides; anything else is
        converted once) -> the stem's map, fp32 ``[B, 64, Hp, Wp]``; ``out``: write into this tensor or view instead."""
        x = _images(images, "ResNetStem images")
        B, _, Hi, Wi = (int(v) for v in x.shape)
        h = self._load(x.device)
        Co, Hp, Wp = self.out_shape(Hi, Wi)
        if out is None:
            out = torch.empty(B, Co, Hp, Wp, device=x.device, dtype=torch.float32)
        elif tuple(out.shape) != (B, Co, Hp, Wp) or out.dtype != torch.float32 or out.device != x.device or out.stride(3) != 1 or \
                (Hp > 1 and out.stride(2) != Wp):
            raise RuntimeError(f"hoigen_amd: ResNetStem: out must be an fp32 [{B}, {Co}, {Hp}, {Wp}] tensor (or view) on the images' device whose "
                               "tokens are contiguous within a channel")
        a = _lib.hg_resnet_stem_args()
        a.x, a.B, a.Hi, a.Wi, a.out = x.data_ptr(), B, Hi, Wi, out.data_ptr()
        a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
        a.out_stride[:] = [out.stride(0), out.stride(1)]
        self._ctx.check(_lib.lib().hg_resnet_stem(h, C.byref(a), _stream_ptr(x.device)), "hg_resnet_stem")
        return out


class NativeBody(nn.Module):
    """The body the reference builds at backbone.py:69-73 with the stages native: ``forward(images)`` returns ``{'0': layer4's map}`` as
    ``IntermediateLayerGetter`` does, so it drops into ``Detector``.  The stem is the torch modules (``stem``) by default; with
    ``native_stem=True`` it is ``ResNetStem`` on the stages' context and ``forward`` is one native call (hg_resnet_body)."""

    def __init__(self, stem: Sequence[nn.Module], stages: ResNetStages, native_stem: Optional[ResNetStem] = None):
        super().__init__()
        self.stem = nn.Sequential(*stem)
        self.stages = stages
        self.native_stem = native_stem
        if native_stem is not None:
            native_stem._ctx = stages._ctx

    @classmethod
    def from_module(cls, body: nn.Module, native_stem: bool = False) -> "NativeBody":
        missing = [k for k in ("conv1", "bn1", "relu", "maxpool") if getattr(body, k, None) is None]
        if missing:
            raise RuntimeError(f"hoigen_amd: NativeBody.from_module: the body ({type(body).__name__}) has no {missing}")
        if native_stem:
            m = cls([], ResNetStages.from_module(body), ResNetStem.from_module(body))
        else:
            m = cls([body.conv1, body.bn1, body.relu, body.maxpool], ResNetStages.from_module(body))
        m.train(getattr(body, "training", False))
        return m

    def _run_body(self, images: torch.Tensor, last_block: Optional[int] = None, out: Optional[torch.Tensor] = None, want_trace: bool = False):
        """hg_resnet_body: (map, every block's output or None)"""
        st, sg = self.native_stem, self.stages
        x = _images(images, "NativeBody images")
        B, _, Hi, Wi = (int(v) for v in x.shape)
        n = len(sg.blocks())
        last = n - 1 if last_block is None else int(last_block)
        if not (0 <= last < n):
            raise RuntimeError(f"hoigen_amd: NativeBody: blocks 0 .. {last} of {n}")
        if sg._ctx is not st._ctx:
            raise RuntimeError("hoigen_amd: NativeBody: the stem and the stages must share one native context")
        h = sg._load(x.device)
        st._load(x.device)
        _, Hp, Wp = st.out_shape(Hi, Wi)
        Co, Ho, Wo = sg.out_shape(Hp, Wp, 0, last)
        f32 = dict(device=x.device, dtype=torch.float32)
        if out is None:
            out = torch.empty(B, Co, Ho, Wo, **f32)
        elif tuple(out.shape) != (B, Co, Ho, Wo) or out.dtype != torch.float32 or out.device != x.device or out.stride(3) != 1 or \
                (Ho > 1 and out.stride(2) != Wo):
            raise RuntimeError(f"hoigen_amd: NativeBody: out must be an fp32 [{B}, {Co}, {Ho}, {Wo}] tensor (or view) on the images' device whose "
                               "tokens are contiguous within a channel")
        a = _lib.hg_resnet_body_args()
        a.x, a.B, a.Hi, a.Wi, a.last_block, a.out = x.data_ptr(), B, Hi, Wi, last, out.data_ptr()
        a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
        a.out_stride[:] = [out.stride(0), out.stride(1)]
        trace = None
        if want_trace:
            trace = [torch.empty(B, *sg.out_shape(Hp, Wp, 0, i), **f32) for i in range(last + 1)]
            ptrs = (C.c_void_p * len(trace))(*[t.data_ptr() for t in trace])
            a.trace = ptrs
        st._ctx.check(_lib.lib().hg_resnet_body(h, C.byref(a), _stream_ptr(x.device)), "hg_resnet_body")
        return out, trace

    @_inference_only
    @torch.no_grad()
    def forward(self, images: torch.Tensor):
        if self.native_stem is not None:
            return {"0": self._run_body(images)[0]}
        return {"0": self.stages._run(self.stem(images))[0]}


class ResNetFeatures(nn.Module):
    """A torchvision-style bottleneck ResNet with ``fc = nn.Identity()`` - the reference's ``dino_model`` (main_tip_finetune.py:404-408,
    upt_tip_cache_model_free_finetune_distill3.py:1616-1618) - in one native call (hg_resnet_features): the stem, ``layer1`` ..
    ``layer4``, then ONE launch that pools the last block's NHWC stream where it lies and L2-normalises the rows.

        self.dino_model = ResNetFeatures.from_module(dino_model)      # forward(images) -> [B, 2048], as before
        dino_feat = self.dino_model.normalized(images)                # :1617-1618 in one call

    ``pooled``: per (image, channel) one fp32 accumulator over the positions in ascending order and one division; ``features``: sum of
    squares, ``sqrtf``, one reciprocal, one multiply (a zero row is NaN, as ``0 / 0`` is).  Stem and stages share one native context of
    this object's own, so a detector's ResNet and this one coexist."""

    def __init__(self, stem: ResNetStem, stages: ResNetStages):
        super().__init__()
        self.stem = stem
        self.stages = stages
        stem._ctx = stages._ctx

    @classmethod
    def from_module(cls, net: nn.Module) -> "ResNetFeatures":
        """``net``: attributes ``conv1, bn1, relu, maxpool, layer1 .. layer4`` as ``ResNetStem`` / ``ResNetStages`` read them; ``avgpool``
        an adaptive average pool to 1 x 1 (or absent); ``fc`` an ``nn.Identity`` (or absent).  Anything else is refused here, without a
        device."""
        head = "hoigen_amd: ResNetFeatures.from_module: "
        fc = getattr(net, "fc", None)
        if fc is not None and not isinstance(fc, nn.Identity):
            what = f"a Linear {fc.in_features} -> {fc.out_features}" if isinstance(fc, nn.Linear) else type(fc).__name__
            raise RuntimeError(head + f"fc is {what}; only nn.Identity (or no fc) is implemented: the reference replaces it "
                               "(main_tip_finetune.py:406), and a classifier behind the pool is the caller's")
        pool = getattr(net, "avgpool", None)
        if pool is not None:
            size = getattr(pool, "output_size", None)
            if not isinstance(pool, nn.AdaptiveAvgPool2d) or size not in (1, (1, 1), [1, 1]):
                raise RuntimeError(head + f"avgpool is {pool!r}; only nn.AdaptiveAvgPool2d to 1 x 1 (or no avgpool) is implemented")
        stages = ResNetStages.from_module(net)
        stem = ResNetStem.from_module(net)
        if len(stages.level_names) != 4:
            raise RuntimeError(head + "layer1 .. layer4 are needed")
        m = cls(stem, stages)
        m.train(getattr(net, "training", False))
        return m

    @property
    def num_channels(self) -> int:
        return self.stages.blocks()[-1].conv3.desc.cout

    def _run(self, images: torch.Tensor, want_pooled: bool, want_features: bool, want_map: bool):
        st, sg = self.stem, self.stages
        x = _images(images, "ResNetFeatures images")
        B, _, Hi, Wi = (int(v) for v in x.shape)
        if sg._ctx is not st._ctx:
            raise RuntimeError("hoigen_amd: ResNetFeatures: the stem and the stages must share one native context")
        h = sg._load(x.device)
        st._load(x.device)
        _, Hp, Wp = st.out_shape(Hi, Wi)
        Co, Ho, Wo = sg.out_shape(Hp, Wp)
        f32 = dict(device=x.device, dtype=torch.float32)
        pooled = torch.empty(B, Co, **f32) if want_pooled else None
        features = torch.empty(B, Co, **f32) if want_features else None
        fmap = torch.empty(B, Co, Ho, Wo, **f32) if want_map else None
        a = _lib.hg_resnet_features_args()
        a.x, a.B, a.Hi, a.Wi = x.data_ptr(), B, Hi, Wi
        a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
        a.pooled = pooled.data_ptr() if want_pooled else None
        a.features = features.data_ptr() if want_features else None
        if want_map:
            a.map_out = fmap.data_ptr()
            a.map_stride[:] = [fmap.stride(0), fmap.stride(1)]
        st._ctx.check(_lib.lib().hg_resnet_features(h, C.byref(a), _stream_ptr(x.device)), "hg_resnet_features")
        return pooled, features, fmap

    @_inference_only
    @torch.no_grad()
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """``images [B, 3, Hi, Wi]`` -> ``pooled [B, C]``: what ``dino_model(images)`` returns (:1617)."""
        return self._run(images, True, False, False)[0]

    @_inference_only
    @torch.no_grad()
    def normalized(self, images: torch.Tensor) -> torch.Tensor:
        """``pooled / pooled.norm(dim=-1, keepdim=True)`` (:1617-1618): what ``HOIHead`` takes as ``feat_image``."""
        return self._run(images, False, True, False)[1]

    @_inference_only
    @torch.no_grad()
    def forward_all(self, images: torch.Tensor, pooled: bool = True, features: bool = True, map: bool = True):
        """``(pooled [B, C], features [B, C], map [B, C, Ho, Wo])`` of one call; an output switched off comes back as ``None`` (at least
        one must be on).  ``map`` is ``NativeBody(native_stem=True)``'s, bit for bit."""
        if not (pooled or features or map):
            raise RuntimeError("hoigen_amd: ResNetFeatures.forward_all: at least one of pooled, features and map")
        return self._run(images, bool(pooled), bool(features), bool(map))
