"""DETR transformer façade: the reference's ``Transformer``, ``TransformerEncoder`` and ``TransformerDecoder``
(detr/models/transformer.py:18-124 over the post-norm layers :127-162 and :187-233) with the same state-dict keys and call signatures,
running on the HIP kernels (hoigen_amd/csrc/hg_detr.hip: hg_load_detr_encoder, hg_detr_encoder; hg_detr_dec.hip: hg_load_detr_decoder,
hg_detr_decoder).

    self.detector.transformer = Transformer.from_module(self.detector.transformer)

is the whole integration; the two halves can be swapped on their own as well.  ``DetectionHeads`` is what follows the
transformer in the detector (upt_tip_cache_model_free_finetune_distill3.py:1598-1605): ``class_embed``, ``bbox_embed`` with its sigmoid
and ``PostProcess`` in one launch (the kernel hg_detr_heads.hip under hg_load_detr_heads, hg_detr_heads).  ``DetectorNeck`` is what
precedes it (upt...:1594-1597): ``input_proj``, ``PositionEmbeddingSine`` and the mask on the feature grid in one call (the kernel
hg_detr_neck.hip under hg_load_detr_neck, hg_detr_neck), whose batch-first outputs ``Transformer.forward_tokens`` takes; the host code
of both is hg_detr_ends.hip.  ``Detector`` is lines 1594-1605 as one object.  Inference only; tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib
from .model import LayerNorm, Linear, MultiheadAttention, _inference_only, _NativeModule, _require_cuda, _sig, _stream_ptr
from .resnet import NativeBody, ResNetStages, ResNetStem  # noqa: F401  (the body's native stem and stages: hoigen_amd/resnet.py)

MAX_TOKENS = _lib.HG_DETR_ATTN_MAX_L


class TransformerEncoderLayer(nn.Module):
    """Parameters of detr/models/transformer.py:127-144 (dropout is the identity at inference and holds none)."""

    def __init__(self, d_model: int, nhead: int, dim_feedforward: int = 2048):
        super().__init__()
        self.self_attn = MultiheadAttention(d_model, nhead)
        self.linear1 = Linear(d_model, dim_feedforward)
        self.linear2 = Linear(dim_feedforward, d_model)
        self.norm1 = LayerNorm(d_model)
        self.norm2 = LayerNorm(d_model)


def _is_relu(fn) -> bool:
    return fn is torch.nn.functional.relu or isinstance(fn, nn.ReLU) or getattr(fn, "__name__", "") == "relu"


def _f32_rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 with a channel stride of 1: a permuted view of a batch-first buffer passes as it is, the [S, B, C] view of a [B, C, H, W]
    map (flatten(2).permute(2, 0, 1)) is copied"""
    t = t.detach()
    return t if t.dtype == torch.float32 and t.stride(-1) == 1 else t.to(torch.float32).contiguous()


def _from_stack(cls, stack: nn.Module, what: str, layer_lines: str, *extra):
    """``TransformerEncoder.from_module`` / ``TransformerDecoder.from_module``: the layers of ``stack`` (the reference's ``what``) must be
    post-norm (transformer.py:``layer_lines``) ReLU layers with the state-dict keys of ``cls``; ``extra`` follows the four sizes into ``cls``."""
    who = f"hoigen_amd: {cls.__name__}.from_module:"
    layers = list(stack.layers)
    if not layers:
        raise RuntimeError(f"{who} the {what} has no layers")
    for i, l in enumerate(layers):
        if getattr(l, "normalize_before", False):
            raise RuntimeError(f"{who} layers.{i} is pre-norm (normalize_before); only the post-norm layer (transformer.py:{layer_lines}) "
                               "is implemented")
        act = getattr(l, "activation", torch.nn.functional.relu)
        if not _is_relu(act):
            raise RuntimeError(f"{who} layers.{i} uses activation {act!r}; only ReLU is implemented")
    w = layers[0].self_attn.in_proj_weight
    m = cls(int(w.shape[1]), int(layers[0].self_attn.num_heads), len(layers), int(layers[0].linear1.weight.shape[0]), *extra)
    missing, unexpected = m.load_state_dict(stack.state_dict(), strict=False)
    if missing or unexpected:
        raise RuntimeError(f"{who} state-dict keys differ (missing {missing}, unexpected {unexpected})")
    m.to(device=w.device, dtype=w.dtype)
    m.train(stack.training)
    return m


def _layer_tensors(l: nn.Module) -> list:
    """The twelve tensors an encoder layer and a decoder layer both hold, in the order of hg_detr_layer_weights"""
    t = _lib.tensor
    return [t(l.self_attn.in_proj_weight), t(l.self_attn.in_proj_bias), t(l.self_attn.out_proj.weight), t(l.self_attn.out_proj.bias),
            t(l.linear1.weight), t(l.linear1.bias), t(l.linear2.weight), t(l.linear2.bias), t(l.norm1.weight), t(l.norm1.bias),
            t(l.norm2.weight), t(l.norm2.bias)]


class TransformerEncoder(_NativeModule):
    """detr/models/transformer.py:62-83.  ``forward(src, mask=None, src_key_padding_mask=None, pos=None)`` on ``[S, B, C]`` tensors
    returns ``[S, B, C]`` fp32.  Post-norm ReLU layers without a final norm - what the detector builds (transformer.py:26-29 with
    normalize_before = False); anything else is refused."""

    def __init__(self, d_model: int = 256, nhead: int = 8, num_layers: int = 6, dim_feedforward: int = 2048):
        super().__init__()
        self.d_model, self.nhead, self.num_layers, self.dim_feedforward = d_model, nhead, num_layers, dim_feedforward
        self.layers = nn.ModuleList([TransformerEncoderLayer(d_model, nhead, dim_feedforward) for _ in range(num_layers)])
        self.norm = None

    @classmethod
    def from_module(cls, encoder: nn.Module) -> "TransformerEncoder":
        """From the reference's TransformerEncoder (or any module with its attributes and state-dict keys
        ``layers.N.self_attn.in_proj_weight`` / ``in_proj_bias`` / ``out_proj.*``, ``linear1``, ``linear2``, ``norm1``, ``norm2``)."""
        if getattr(encoder, "norm", None) is not None:
            raise RuntimeError("hoigen_amd: TransformerEncoder.from_module: a final norm (the pre-norm encoder, transformer.py:28) is not "
                               "implemented; the detector's encoder is post-norm and has none")
        return _from_stack(cls, encoder, "encoder", "149-162")

    def _load_native(self, h: int) -> None:
        arr = (_lib.hg_detr_layer_weights * self.num_layers)(*[_lib.hg_detr_layer_weights(*_layer_tensors(l)) for l in self.layers])
        w = _lib.hg_detr_encoder_weights(self.d_model, self.nhead, self.dim_feedforward, self.num_layers, 0, 0, arr)
        self._ctx.check(_lib.lib().hg_load_detr_encoder(h, C.byref(w)), "hg_load_detr_encoder")

    def _run(self, src, mask, src_key_padding_mask, pos, want_trace: bool, out: Optional[torch.Tensor] = None, trace=None):
        if mask is not None:
            raise RuntimeError("hoigen_amd: TransformerEncoder: an attention mask (`mask`) is not implemented; the detector passes None "
                               "(detr/models/transformer.py:55) and masks padding with src_key_padding_mask")
        if self.norm is not None:
            raise RuntimeError("hoigen_amd: TransformerEncoder: a final norm is not implemented (post-norm encoder only)")
        _require_cuda(src, "TransformerEncoder src")
        if src.dim() != 3 or src.shape[2] != self.d_model:
            raise RuntimeError(f"hoigen_amd: TransformerEncoder: src must be [S, B, {self.d_model}] (got {tuple(src.shape)})")
        S, B, D = src.shape
        h = self._load(src.device)
        x = _f32_rows(src)
        p = None
        if pos is not None:
            _require_cuda(pos, "TransformerEncoder pos")
            p = _f32_rows(pos).expand(S, B, D)
        kpm = None
        if src_key_padding_mask is not None:
            _require_cuda(src_key_padding_mask, "TransformerEncoder src_key_padding_mask")
            if tuple(src_key_padding_mask.shape) != (B, S):
                raise RuntimeError(f"hoigen_amd: TransformerEncoder: src_key_padding_mask must be [B, S] = [{B}, {S}] "
                                   f"(got {tuple(src_key_padding_mask.shape)})")
            kpm = src_key_padding_mask.detach().to(torch.uint8).contiguous()
        if out is None:
            out = torch.empty(S, B, D, device=src.device, dtype=torch.float32)
        elif tuple(out.shape) != (S, B, D) or out.dtype != torch.float32 or out.stride(2) != 1 or out.device != src.device:
            raise RuntimeError("hoigen_amd: TransformerEncoder: out must be an fp32 [S, B, C] tensor (or view) on src's device with channel stride 1")
        if trace is not None and (tuple(trace.shape) != (self.num_layers, B * S, D) or trace.dtype != torch.float32 or not trace.is_contiguous()):
            raise RuntimeError("hoigen_amd: TransformerEncoder: trace must be a contiguous fp32 [num_layers, B * S, C] tensor")
        if trace is None and want_trace:
            trace = torch.empty(self.num_layers, B * S, D, device=src.device, dtype=torch.float32)
        a = _lib.hg_detr_encoder_args()
        a.src, a.pos, a.mask = x.data_ptr(), (p.data_ptr() if p is not None else None), (kpm.data_ptr() if kpm is not None else None)
        a.out, a.trace, a.B, a.S = out.data_ptr(), (trace.data_ptr() if trace is not None else None), B, S
        for name, t in (("src_stride", x), ("pos_stride", p), ("out_stride", out)):
            if t is not None:
                getattr(a, name)[:] = [t.stride(1), t.stride(0), t.stride(2)]
        self._ctx.check(_lib.lib().hg_detr_encoder(h, C.byref(a), _stream_ptr(src.device)), "hg_detr_encoder")
        return out, trace

    @_inference_only
    @torch.no_grad()
    def forward(self, src, mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._run(src, mask, src_key_padding_mask, pos, False)[0]

    @_inference_only
    @torch.no_grad()
    def forward_trace(self, src, mask=None, src_key_padding_mask=None, pos=None, out=None, trace=None):
        """(output [S, B, C], trace [num_layers, B * S, C]: the stream after every layer, batch-major) - for the tests.  ``out``: an fp32
        [S, B, C] tensor or view to write into (e.g. the permuted view of a batch-first buffer); ``trace``: a contiguous buffer to write the trace into."""
        return self._run(src, mask, src_key_padding_mask, pos, True, out, trace)


class TransformerDecoderLayer(nn.Module):
    """Parameters of detr/models/transformer.py:187-204 (dropout is the identity at inference and holds none)."""

    def __init__(self, d_model: int, nhead: int, dim_feedforward: int = 2048):
        super().__init__()
        self.self_attn = MultiheadAttention(d_model, nhead)
        self.multihead_attn = MultiheadAttention(d_model, nhead)
        self.linear1 = Linear(d_model, dim_feedforward)
        self.linear2 = Linear(dim_feedforward, d_model)
        self.norm1 = LayerNorm(d_model)
        self.norm2 = LayerNorm(d_model)
        self.norm3 = LayerNorm(d_model)


class TransformerDecoder(_NativeModule):
    """detr/models/transformer.py:86-124.  ``forward(tgt, memory, ..., memory_key_padding_mask, pos, query_pos)`` on ``[Q, B, C]`` /
    ``[S, B, C]`` tensors returns ``[L, Q, B, C]`` fp32 with ``return_intermediate`` and ``[1, Q, B, C]`` without.  Post-norm ReLU layers
    with the final norm - what the detector builds (transformer.py:31-35); anything else is refused."""

    def __init__(self, d_model: int = 256, nhead: int = 8, num_layers: int = 6, dim_feedforward: int = 2048,
                 return_intermediate: bool = False):
        super().__init__()
        self.d_model, self.nhead, self.num_layers, self.dim_feedforward = d_model, nhead, num_layers, dim_feedforward
        self.layers = nn.ModuleList([TransformerDecoderLayer(d_model, nhead, dim_feedforward) for _ in range(num_layers)])
        self.norm = LayerNorm(d_model)
        self.return_intermediate = bool(return_intermediate)

    @classmethod
    def from_module(cls, decoder: nn.Module) -> "TransformerDecoder":
        """From the reference's TransformerDecoder (or any module with its attributes and state-dict keys ``layers.N.self_attn.*``,
        ``multihead_attn.*``, ``linear1``, ``linear2``, ``norm1`` .. ``norm3`` and ``norm``)."""
        if getattr(decoder, "norm", None) is None:
            raise RuntimeError("hoigen_amd: TransformerDecoder.from_module: the decoder has no final norm (norm is None); the detector's "
                               "decoder has one (transformer.py:33) and only that form is implemented")
        return _from_stack(cls, decoder, "decoder", "212-233", bool(getattr(decoder, "return_intermediate", False)))

    def _load_native(self, h: int) -> None:
        t = _lib.tensor
        arr = (_lib.hg_detr_dec_layer_weights * self.num_layers)(*[_lib.hg_detr_dec_layer_weights(
            *_layer_tensors(l), t(l.multihead_attn.in_proj_weight), t(l.multihead_attn.in_proj_bias), t(l.multihead_attn.out_proj.weight),
            t(l.multihead_attn.out_proj.bias), t(l.norm3.weight), t(l.norm3.bias)) for l in self.layers])
        norm = self.norm
        w = _lib.hg_detr_decoder_weights(self.d_model, self.nhead, self.dim_feedforward, self.num_layers, 0, 0,
                                         t(norm.weight if norm is not None else None), t(norm.bias if norm is not None else None), arr)
        self._ctx.check(_lib.lib().hg_load_detr_decoder(h, C.byref(w)), "hg_load_detr_decoder")

    def _run(self, tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask, memory_key_padding_mask, pos, query_pos, want_trace: bool,
             out: Optional[torch.Tensor] = None):
        for name, m in (("tgt_mask", tgt_mask), ("memory_mask", memory_mask), ("tgt_key_padding_mask", tgt_key_padding_mask)):
            if m is not None:
                raise RuntimeError(f"hoigen_amd: TransformerDecoder: `{name}` is not implemented; the detector passes None "
                                   "(detr/models/transformer.py:57-58) and masks padding with memory_key_padding_mask")
        _require_cuda(memory, "TransformerDecoder memory")
        D = self.d_model
        if memory.dim() != 3 or memory.shape[2] != D:
            raise RuntimeError(f"hoigen_amd: TransformerDecoder: memory must be [S, B, {D}] (got {tuple(memory.shape)})")
        S, B, _ = memory.shape
        dev = memory.device
        if query_pos is None:
            if tgt is None:
                raise RuntimeError("hoigen_amd: TransformerDecoder: tgt and query_pos are both None: the number of queries is unknown")
            query_pos = torch.zeros(tgt.shape[0], D, device=dev)
        _require_cuda(query_pos, "TransformerDecoder query_pos")
        qp = _f32_rows(query_pos)
        if qp.dim() not in (2, 3) or qp.shape[-1] != D or (qp.dim() == 3 and qp.shape[1] != B):
            raise RuntimeError(f"hoigen_amd: TransformerDecoder: query_pos must be [Q, {D}] or [Q, B = {B}, {D}] (got {tuple(qp.shape)})")
        Q = int(qp.shape[0])
        h = self._load(dev)
        a = _lib.hg_detr_decoder_args()
        a.query_pos = qp.data_ptr()
        a.query_pos_stride[:] = [qp.stride(1) if qp.dim() == 3 else 0, qp.stride(0), 1]
        tg = None
        if tgt is not None:
            _require_cuda(tgt, "TransformerDecoder tgt")
            if tuple(tgt.shape) != (Q, B, D):
                raise RuntimeError(f"hoigen_amd: TransformerDecoder: tgt must be [Q, B, C] = [{Q}, {B}, {D}] (got {tuple(tgt.shape)})")
            tg = _f32_rows(tgt)
            a.tgt = tg.data_ptr()
            a.tgt_stride[:] = [tg.stride(1), tg.stride(0), 1]
        mem = _f32_rows(memory)
        a.memory = mem.data_ptr()
        a.memory_stride[:] = [mem.stride(1), mem.stride(0), 1]
        p = None
        if pos is not None:
            _require_cuda(pos, "TransformerDecoder pos")
            p = _f32_rows(pos).expand(S, B, D)
            a.pos = p.data_ptr()
            a.pos_stride[:] = [p.stride(1), p.stride(0), 1]
        kpm = None
        if memory_key_padding_mask is not None:
            _require_cuda(memory_key_padding_mask, "TransformerDecoder memory_key_padding_mask")
            if tuple(memory_key_padding_mask.shape) != (B, S):
                raise RuntimeError(f"hoigen_amd: TransformerDecoder: memory_key_padding_mask must be [B, S] = [{B}, {S}] "
                                   f"(got {tuple(memory_key_padding_mask.shape)})")
            kpm = memory_key_padding_mask.detach().to(torch.uint8).contiguous()
            a.memory_mask = kpm.data_ptr()
        L = self.num_layers if self.return_intermediate else 1
        if out is None:
            out = torch.empty(L, Q, B, D, device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (L, Q, B, D) or out.dtype != torch.float32 or out.stride(3) != 1 or out.device != dev:
            raise RuntimeError("hoigen_amd: TransformerDecoder: out must be an fp32 [L, Q, B, C] tensor (or view) on memory's device with channel stride 1")
        trace = torch.empty(self.num_layers, B * Q, D, device=dev, dtype=torch.float32) if want_trace else None
        a.out, a.trace = out.data_ptr(), (trace.data_ptr() if trace is not None else None)
        a.out_stride[:] = [out.stride(0), out.stride(2), out.stride(1), 1]
        a.B, a.S, a.Q, a.return_intermediate = B, S, Q, int(self.return_intermediate)
        self._ctx.check(_lib.lib().hg_detr_decoder(h, C.byref(a), _stream_ptr(dev)), "hg_detr_decoder")
        return out, trace

    @_inference_only
    @torch.no_grad()
    def forward(self, tgt, memory, tgt_mask: Optional[torch.Tensor] = None, memory_mask: Optional[torch.Tensor] = None,
                tgt_key_padding_mask: Optional[torch.Tensor] = None, memory_key_padding_mask: Optional[torch.Tensor] = None,
                pos: Optional[torch.Tensor] = None, query_pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._run(tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask, memory_key_padding_mask, pos, query_pos, False)[0]

    @_inference_only
    @torch.no_grad()
    def forward_trace(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None, pos=None,
                      query_pos=None, out=None):
        """(hs [L, Q, B, C], trace [num_layers, B * Q, C]: the stream after every layer - after norm3, before the final norm -,
        batch-major) - for the tests.  ``tgt`` may be None (zeros, nothing read); ``out``: an fp32 [L, Q, B, C] tensor or view to write into."""
        return self._run(tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask, memory_key_padding_mask, pos, query_pos, True, out)


class Transformer(nn.Module):
    """detr/models/transformer.py:18-59: ``forward(src [B, C, H, W], mask [B, H, W], query_embed [Q, C], pos_embed [B, C, H, W])`` returns
    ``(hs [L, B, Q, C], memory [B, C, H, W])``.  Both halves share one native context.  src and pos_embed are channel-major maps and the
    native calls want a channel stride of 1: each is transposed to [B, S, C] once (pos_embed once for both halves); memory travels from the
    encoder to the decoder as a [B, S, C] buffer through strides, hs is written in [L, B, Q, C] order, and the returned memory is the
    [B, C, H, W] view of that buffer, as the reference's is of its own."""

    def __init__(self, d_model: int = 256, nhead: int = 8, num_encoder_layers: int = 6, num_decoder_layers: int = 6,
                 dim_feedforward: int = 2048, return_intermediate_dec: bool = False):
        super().__init__()
        self.encoder = TransformerEncoder(d_model, nhead, num_encoder_layers, dim_feedforward)
        self.decoder = TransformerDecoder(d_model, nhead, num_decoder_layers, dim_feedforward, return_intermediate_dec)
        self.decoder._ctx = self.encoder._ctx
        self.d_model, self.nhead = d_model, nhead

    @classmethod
    def from_module(cls, transformer: nn.Module) -> "Transformer":
        enc, dec = TransformerEncoder.from_module(transformer.encoder), TransformerDecoder.from_module(transformer.decoder)
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.encoder, m.decoder = enc, dec
        dec._ctx = enc._ctx
        m.d_model, m.nhead = enc.d_model, enc.nhead
        m.train(transformer.training)
        return m

    def set_option(self, key: str, value: int) -> None:
        self.encoder.set_option(key, value)

    def get_option(self, key: str):
        return self.encoder.get_option(key)

    @_inference_only
    @torch.no_grad()
    def forward(self, src, mask, query_embed, pos_embed):
        _require_cuda(src, "Transformer src")
        if src.dim() != 4 or src.shape[1] != self.d_model or pos_embed.shape != src.shape:
            raise RuntimeError(f"hoigen_amd: Transformer: src and pos_embed must be [B, {self.d_model}, H, W] (got {tuple(src.shape)}, "
                               f"{tuple(pos_embed.shape)})")
        H, W = src.shape[2:]
        src_b = src.detach().to(torch.float32).flatten(2).transpose(1, 2).contiguous()      # [B, S, C] buffers
        pos_b = pos_embed.detach().to(torch.float32).flatten(2).transpose(1, 2).contiguous()
        return self._run_tokens(src_b, mask.flatten(1) if mask is not None else None, query_embed, pos_b, H, W)

    def _run_tokens(self, src, kpm, query_embed, pos, H: int, W: int):
        """Encoder and decoder on batch-first ``src`` / ``pos`` ``[B, S, C]`` fp32 with channel stride 1 and ``kpm [B, S]``: both read
        them as [S, B, C] views through strides.  Returns ``(hs [L, B, Q, C], memory [B, C, H, W])``."""
        B, S, Cc = src.shape
        mem = torch.empty(B, S, Cc, device=src.device, dtype=torch.float32)
        pos_s = pos.permute(1, 0, 2)
        self.encoder._run(src.permute(1, 0, 2), None, kpm, pos_s, False, mem.permute(1, 0, 2))
        L = self.decoder.num_layers if self.decoder.return_intermediate else 1
        hs = torch.empty(L, B, query_embed.shape[0], Cc, device=src.device, dtype=torch.float32)
        self.decoder._run(None, mem.permute(1, 0, 2), None, None, None, kpm, pos_s, query_embed, False, hs.permute(0, 2, 1, 3))
        return hs, mem.permute(0, 2, 1).view(B, Cc, H, W)

    @_inference_only
    @torch.no_grad()
    def forward_tokens(self, src, mask, query_embed, pos, hw):
        """``forward`` on what ``DetectorNeck`` returns: ``src`` and ``pos`` batch-first ``[B, S, C]`` fp32 with channel stride 1,
        ``mask [B, S]``, ``hw = (H, W)`` with H W = S.  Encoder and decoder read both through strides, so nothing is transposed or
        copied.  Returns what ``forward`` returns: ``(hs [L, B, Q, C], memory [B, C, H, W])``."""
        _require_cuda(src, "Transformer src")
        H, W = (int(v) for v in hw)
        if src.dim() != 3 or src.shape[2] != self.d_model or pos.shape != src.shape or src.shape[1] != H * W:
            raise RuntimeError(f"hoigen_amd: Transformer.forward_tokens: src and pos must be [B, S = H W = {H * W}, {self.d_model}] "
                               f"(got {tuple(src.shape)}, {tuple(pos.shape)})")
        return self._run_tokens(src, mask.reshape(src.shape[:2]) if mask is not None else None, query_embed, pos, H, W)


class BoxMLP(nn.Module):
    """Parameters of the reference's ``MLP(D, D, 4, 3)`` (detr/models/detr.py:293-305): ``layers.{0,1,2}.weight`` / ``bias``."""

    def __init__(self, d_model: int):
        super().__init__()
        self.num_layers = 3
        self.layers = nn.ModuleList([Linear(d_model, d_model), Linear(d_model, d_model), Linear(d_model, 4)])


class DetectionHeads(_NativeModule):
    """The statements between the detector's transformer and the region proposals
    (upt_tip_cache_model_free_finetune_distill3.py:1598-1605) in one native launch (hoigen_amd/csrc/hg_detr_heads.hip: hg_load_detr_heads,
    hg_detr_heads; the host code is hg_detr_ends.hip): ``class_embed(hs)``, ``bbox_embed(hs).sigmoid()``, the V-COCO column selection ``[..., reserve_indices]`` and
    ``PostProcess`` (detr/models/detr.py:258-290).

        heads = DetectionHeads.from_modules(self.detector.class_embed, self.detector.bbox_embed, reserve_indices)
        results = heads.detect(hs, image_sizes)

    Parameters ``class_embed.weight`` / ``bias`` and ``bbox_embed.layers.{0,1,2}.weight`` / ``bias``, the detector's own keys.  With
    ``reserve_indices`` the logits are those rows of ``class_embed`` in that order; the last of them is the no-object column.
    Inference only; tensors must live on a HIP device."""

    def __init__(self, d_model: int = 256, num_logits: int = 92, reserve_indices=None):
        super().__init__()
        self.d_model, self.num_logits = d_model, num_logits
        self.class_embed = Linear(d_model, num_logits)
        self.bbox_embed = BoxMLP(d_model)
        self.reserve_indices = None if reserve_indices is None else [int(i) for i in reserve_indices]

    @property
    def n_out(self) -> int:
        """C1: the logits a row has (classes + 1)"""
        return self.num_logits if self.reserve_indices is None else len(self.reserve_indices)

    @classmethod
    def from_modules(cls, class_embed: nn.Module, bbox_embed: nn.Module, reserve_indices=None) -> "DetectionHeads":
        """From the reference's ``class_embed`` (an ``nn.Linear``: ``weight``, ``bias``) and ``bbox_embed`` (its ``MLP``:
        ``layers.{0,1,2}.weight`` / ``bias``), or any modules with those state-dict keys."""
        cw = class_embed.state_dict()
        bw = bbox_embed.state_dict()
        if sorted(cw) != ["bias", "weight"] or cw["weight"].dim() != 2:
            raise RuntimeError(f"hoigen_amd: DetectionHeads.from_modules: class_embed must hold a [C1, D] `weight` and a `bias` (got {sorted(cw)})")
        C1, D = (int(v) for v in cw["weight"].shape)
        want = sorted(f"layers.{i}.{k}" for i in range(3) for k in ("weight", "bias"))
        if sorted(bw) != want:
            raise RuntimeError("hoigen_amd: DetectionHeads.from_modules: bbox_embed must be the three-layer MLP(D, D, 4, 3) of "
                               f"detr/models/detr.py:38 with keys {want} (got {sorted(bw)})")
        shapes = [tuple(bw[f"layers.{i}.weight"].shape) for i in range(3)]
        if shapes != [(D, D), (D, D), (4, D)]:
            raise RuntimeError(f"hoigen_amd: DetectionHeads.from_modules: bbox_embed must be of width D -> D -> D -> 4 with D = {D}, the "
                               f"width of class_embed (got weights {shapes})")
        m = cls(D, C1, reserve_indices)
        if m.reserve_indices is not None and any(i < 0 or i >= C1 for i in m.reserve_indices):
            raise RuntimeError(f"hoigen_amd: DetectionHeads.from_modules: reserve_indices must lie in [0, {C1})")
        m.class_embed.load_state_dict(cw)
        m.bbox_embed.load_state_dict(bw)
        w = cw["weight"]
        m.to(device=w.device, dtype=w.dtype)
        m.train(class_embed.training)
        return m

    def _sig_terms(self) -> tuple:
        return (_sig(self.parameters()), tuple(self.reserve_indices or ()))

    def _load_native(self, h: int) -> None:
        t = lambda p: _lib.tensor(p.detach().contiguous())
        ls = self.bbox_embed.layers
        rows = self.reserve_indices
        arr = (C.c_int32 * len(rows))(*rows) if rows is not None else None
        w = _lib.hg_detr_heads_weights(t(self.class_embed.weight), t(self.class_embed.bias), t(ls[0].weight), t(ls[0].bias), t(ls[1].weight),
                                       t(ls[1].bias), t(ls[2].weight), t(ls[2].bias), self.d_model, self.num_logits, arr,
                                       len(rows) if rows is not None else 0)
        self._ctx.check(_lib.lib().hg_load_detr_heads(h, C.byref(w)), "hg_load_detr_heads")

    def _run(self, hs, target_sizes, want_all: bool):
        _require_cuda(hs, "DetectionHeads hs")
        if hs.dim() != 4 or hs.shape[3] != self.d_model:
            raise RuntimeError(f"hoigen_amd: DetectionHeads: hs must be [L, B, Q, {self.d_model}] (got {tuple(hs.shape)})")
        L, B, Q, _ = hs.shape
        x = hs.detach()
        if x.dtype != torch.float32 or x.stride(3) != 1:
            x = x.to(torch.float32).contiguous()
        if target_sizes is None:
            sizes = [(1.0, 1.0)] * B
        elif isinstance(target_sizes, torch.Tensor):
            sizes = target_sizes.detach().to("cpu", torch.float32).reshape(-1, 2).tolist()
        else:
            sizes = [(float(h_), float(w_)) for h_, w_ in target_sizes]
        if len(sizes) != B:
            raise RuntimeError(f"hoigen_amd: DetectionHeads: target_sizes must hold one (h, w) for each of the {B} images (got {len(sizes)})")
        h = self._load(x.device)
        f32 = dict(device=x.device, dtype=torch.float32)
        C1 = self.n_out
        logits = torch.empty(L, B, Q, C1, **f32) if want_all else None
        pboxes = torch.empty(L, B, Q, 4, **f32) if want_all else None
        scores, boxes = torch.empty(B, Q, **f32), torch.empty(B, Q, 4, **f32)
        labels = torch.empty(B, Q, device=x.device, dtype=torch.int32)
        a = _lib.hg_detr_heads_args()
        a.hs, a.L, a.B, a.Q = x.data_ptr(), L, B, Q
        a.hs_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
        a.target_sizes = (C.c_float * (2 * B))(*[v for hw in sizes for v in hw])
        a.pred_logits, a.pred_boxes = (logits.data_ptr(), pboxes.data_ptr()) if want_all else (None, None)
        a.scores, a.labels, a.boxes = scores.data_ptr(), labels.data_ptr(), boxes.data_ptr()
        self._ctx.check(_lib.lib().hg_detr_heads(h, C.byref(a), _stream_ptr(x.device)), "hg_detr_heads")
        return logits, pboxes, scores, labels, boxes

    @_inference_only
    @torch.no_grad()
    def forward(self, hs):
        """``(outputs_class [L, B, Q, C1], outputs_coord [L, B, Q, 4])`` fp32, as upt...:1598-1602 produce them from ``hs [L, B, Q, D]``."""
        logits, pboxes = self._run(hs, None, True)[:2]
        return logits, pboxes

    @_inference_only
    @torch.no_grad()
    def detect(self, hs, target_sizes, with_outputs: bool = False):
        """What ``PostProcess.forward({'pred_logits': outputs_class[-1], 'pred_boxes': outputs_coord[-1]}, target_sizes)`` returns
        (upt...:1604-1605): a list of B dicts ``scores [Q]`` fp32, ``labels [Q]`` int64 (as ``torch.max`` gives them) and ``boxes [Q, 4]``
        fp32 in pixels, per-image views of packed buffers.  Only the last level of ``hs`` is computed unless ``with_outputs``, which also
        returns ``{'pred_logits', 'pred_boxes'}`` of the last level.  ``target_sizes``: a host sequence of (h, w), or a tensor [B, 2];
        the sizes travel in the launch's arguments, so a DEVICE tensor costs one copy to the host (and its wait) - pass the host list
        the caller built it from where there is one."""
        logits, pboxes, scores, labels, boxes = self._run(hs, target_sizes, with_outputs)
        labels = labels.to(torch.int64)
        results = [{"scores": s, "labels": l, "boxes": b} for s, l, b in zip(scores, labels, boxes)]
        if with_outputs:
            return results, {"pred_logits": logits[-1], "pred_boxes": pboxes[-1]}
        return results


class DetectorNeck(_NativeModule):
    """What stands between the detector's ResNet body and its transformer (upt_tip_cache_model_free_finetune_distill3.py:1594-1597) in
    one native call (hoigen_amd/csrc/hg_detr_neck.hip: hg_load_detr_neck, hg_detr_neck): the padding mask on the feature grid
    (detr/models/backbone.py:78), ``PositionEmbeddingSine`` (detr/models/position_encoding.py:28-48), ``input_proj``
    (detr/models/detr.py:40, :65) and the flatten / permute of detr/models/transformer.py:50-51 - the outputs are batch-first, which is
    what ``Transformer.forward_tokens`` takes.

        neck = DetectorNeck.from_modules(self.detector.input_proj, self.detector.backbone[1])
        src, pos, mask, hw = neck(features, image_mask)

    Parameters ``input_proj.weight`` ``[D, Cin, 1, 1]`` / ``bias``, the detector's own keys.  Inference only; tensors must live on a HIP
    device."""

    def __init__(self, in_channels: int = 2048, d_model: int = 256, num_pos_feats: Optional[int] = None, temperature: float = 10000.0,
                 normalize: bool = True, scale: Optional[float] = None):
        super().__init__()
        import math
        self.in_channels, self.d_model = int(in_channels), int(d_model)
        self.num_pos_feats = self.d_model // 2 if num_pos_feats is None else int(num_pos_feats)
        self.temperature, self.normalize = float(temperature), bool(normalize)
        self.scale = 2 * math.pi if scale is None else float(scale)
        self.input_proj = nn.Conv2d(self.in_channels, self.d_model, kernel_size=1)      # a parameter holder: never called

    @classmethod
    def from_modules(cls, input_proj: nn.Module, position_embedding: nn.Module) -> "DetectorNeck":
        """From the reference's ``input_proj`` (an ``nn.Conv2d(Cin, D, kernel_size=1)``) and ``PositionEmbeddingSine`` (or any module
        with its attributes ``num_pos_feats``, ``temperature``, ``normalize``, ``scale``)."""
        missing = [k for k in ("num_pos_feats", "temperature", "normalize", "scale") if not hasattr(position_embedding, k)]
        if missing:
            raise RuntimeError(f"hoigen_amd: DetectorNeck.from_modules: the position embedding ({type(position_embedding).__name__}) has no "
                               f"{missing}: only PositionEmbeddingSine (position_encoding.py:12-48) is implemented, not the learned embedding")
        w = getattr(input_proj, "weight", None)
        if w is None or w.dim() != 4 or tuple(w.shape[2:]) != (1, 1):
            raise RuntimeError("hoigen_amd: DetectorNeck.from_modules: input_proj must be a 1 x 1 convolution with a [D, Cin, 1, 1] weight "
                               f"(got {None if w is None else tuple(w.shape)})")
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        if pair(getattr(input_proj, "stride", 1)) != (1, 1) or getattr(input_proj, "groups", 1) != 1 or \
                pair(getattr(input_proj, "padding", 0)) != (0, 0) or pair(getattr(input_proj, "dilation", 1)) != (1, 1):
            raise RuntimeError("hoigen_amd: DetectorNeck.from_modules: input_proj must have stride 1, groups 1, no padding and no dilation "
                               f"(got stride {input_proj.stride}, groups {input_proj.groups}, padding {input_proj.padding}): only the "
                               "1 x 1 projection of detr/models/detr.py:40 is implemented")
        if getattr(input_proj, "bias", None) is None:
            raise RuntimeError("hoigen_amd: DetectorNeck.from_modules: input_proj has no bias; detr/models/detr.py:40 builds it with one")
        D, Cin = int(w.shape[0]), int(w.shape[1])
        if int(position_embedding.num_pos_feats) != D // 2 or D % 2:
            raise RuntimeError(f"hoigen_amd: DetectorNeck.from_modules: num_pos_feats = {position_embedding.num_pos_feats}, and input_proj "
                               f"has {D} output channels: pos and src are added, so num_pos_feats must be out_channels / 2")
        m = cls(Cin, D, position_embedding.num_pos_feats, position_embedding.temperature, position_embedding.normalize,
                position_embedding.scale)
        m.input_proj.load_state_dict({"weight": w.detach(), "bias": input_proj.bias.detach()})
        m.to(device=w.device, dtype=w.dtype)
        m.train(input_proj.training)
        return m

    def _sig_terms(self) -> tuple:
        return (_sig(self.parameters()), self.num_pos_feats, self.temperature, self.normalize, self.scale)

    def _load_native(self, h: int) -> None:
        t = lambda p: _lib.tensor(p.detach().contiguous())
        w = _lib.hg_detr_neck_weights(t(self.input_proj.weight), t(self.input_proj.bias), self.in_channels, self.d_model,
                                      self.num_pos_feats, self.temperature, int(self.normalize), self.scale)
        self._ctx.check(_lib.lib().hg_load_detr_neck(h, C.byref(w)), "hg_load_detr_neck")

    def _run(self, features, image_mask, want_pos: bool = True, want_mask: bool = True, out=None):
        _require_cuda(features, "DetectorNeck features")
        if features.dim() != 4 or features.shape[1] != self.in_channels:
            raise RuntimeError(f"hoigen_amd: DetectorNeck: features must be [B, {self.in_channels}, H, W] (got {tuple(features.shape)})")
        B, _, H, W = features.shape
        S = H * W
        if S > MAX_TOKENS:
            raise RuntimeError(f"hoigen_amd: DetectorNeck: a {H} x {W} grid is {S} tokens, at most {MAX_TOKENS}")
        x = features.detach()
        if x.dtype != torch.float32 or x.stride(3) != 1 or x.stride(2) != W:      # tokens must be contiguous within a channel: never transposed
            x = x.to(torch.float32).contiguous()
        im = None
        if want_pos or want_mask:
            if image_mask is None or image_mask.dim() != 3 or image_mask.shape[0] != B:
                raise RuntimeError(f"hoigen_amd: DetectorNeck: image_mask must be [B = {B}, Hi, Wi] "
                                   f"(got {None if image_mask is None else tuple(image_mask.shape)})")
            _require_cuda(image_mask, "DetectorNeck image_mask")
            if image_mask.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError(f"hoigen_amd: DetectorNeck: image_mask must be bool or uint8 (got {image_mask.dtype})")
            im = image_mask.detach().contiguous()
        h = self._load(x.device)
        f32 = dict(device=x.device, dtype=torch.float32)
        D = self.d_model
        src, pos, mask = out if out is not None else (None, None, None)
        src = torch.empty(B, S, D, **f32) if src is None else src
        pos = (torch.empty(B, S, D, **f32) if pos is None else pos) if want_pos else None
        mask = (torch.empty(B, S, device=x.device, dtype=torch.bool) if mask is None else mask) if want_mask else None
        for name, t in (("src", src), ("pos", pos)):
            if t is not None and (tuple(t.shape) != (B, S, D) or t.dtype != torch.float32 or t.stride(2) != 1 or t.device != x.device):
                raise RuntimeError(f"hoigen_amd: DetectorNeck: {name} must be an fp32 [B, S, C] tensor (or view) on the features' device with channel stride 1")
        a = _lib.hg_detr_neck_args()
        a.x, a.B, a.H, a.W = x.data_ptr(), B, H, W
        a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(3)]
        if im is not None:
            a.image_mask, a.Hi, a.Wi = im.data_ptr(), im.shape[1], im.shape[2]
        a.src = src.data_ptr()
        a.src_stride[:] = [src.stride(0), src.stride(1)]
        if pos is not None:
            a.pos = pos.data_ptr()
            a.pos_stride[:] = [pos.stride(0), pos.stride(1)]
        if mask is not None:
            if tuple(mask.shape) != (B, S) or mask.dtype not in (torch.bool, torch.uint8) or not mask.is_contiguous():
                raise RuntimeError("hoigen_amd: DetectorNeck: mask must be a contiguous bool or uint8 [B, S] tensor")
            a.mask = mask.data_ptr()
        self._ctx.check(_lib.lib().hg_detr_neck(h, C.byref(a), _stream_ptr(x.device)), "hg_detr_neck")
        return src, pos, mask, (H, W)

    @_inference_only
    @torch.no_grad()
    def forward(self, features, image_mask):
        """``features [B, Cin, H, W]`` (the body's map; fp32 with contiguous tokens is read where it lies, anything else is converted
        once), ``image_mask [B, Hi, Wi]`` bool or uint8 (the NestedTensor's).  Returns ``(src [B, S, D], pos [B, S, D], mask bool [B, S],
        (H, W))``."""
        return self._run(features, image_mask)


class Detector(nn.Module):
    """The detector's forward at upt_tip_cache_model_free_finetune_distill3.py:1594-1605 as one object: the backbone's body stays the
    torch module it is, and ``DetectorNeck``, ``Transformer`` and ``DetectionHeads`` run behind it on one native context.  With
    ``native_stages=True`` the body becomes ``NativeBody``: its stem stays torch, ``layer1`` .. ``layer4`` run on the same context
    (hoigen_amd/resnet.py); with ``native_stem=True`` as well the stem runs there too, and the body is one native call from the images.

        det = Detector.from_module(self.detector, reserve_indices)
        results, hs, memory = det(images.tensors, images.mask, image_sizes)

    ``body``: any module mapping ``[B, 3, Hi, Wi]`` to ``[B, Cin, H, W]`` or to the ``{'0': ...}`` dict ``IntermediateLayerGetter``
    returns.  ``query_embed``: the detector's ``nn.Embedding`` (its ``weight`` is read)."""

    def __init__(self, body: nn.Module, neck: DetectorNeck, transformer: Transformer, heads: DetectionHeads, query_embed: nn.Module):
        super().__init__()
        self.body, self.neck, self.transformer, self.heads, self.query_embed = body, neck, transformer, heads, query_embed
        transformer.decoder._ctx = heads._ctx = neck._ctx = transformer.encoder._ctx
        if isinstance(body, NativeBody):
            body.stages._ctx = transformer.encoder._ctx
            if body.native_stem is not None:
                body.native_stem._ctx = transformer.encoder._ctx

    @classmethod
    def from_module(cls, detr: nn.Module, reserve_indices=None, native_stages: bool = False, *, native_stem: bool = False) -> "Detector":
        if native_stem and not native_stages:
            raise RuntimeError("hoigen_amd: Detector.from_module: native_stem=True needs native_stages=True: the native stem writes the "
                               "stages' operands, and there is no native stem in front of torch stages")
        backbone = detr.backbone
        body = NativeBody.from_module(backbone[0].body, native_stem=native_stem) if native_stages else backbone[0].body
        m = cls(body, DetectorNeck.from_modules(detr.input_proj, backbone[1]), Transformer.from_module(detr.transformer),
                DetectionHeads.from_modules(detr.class_embed, detr.bbox_embed, reserve_indices), detr.query_embed)
        m.train(detr.training)
        return m

    def set_option(self, key: str, value: int) -> None:
        self.neck.set_option(key, value)

    def get_option(self, key: str):
        return self.neck.get_option(key)

    @_inference_only
    @torch.no_grad()
    def forward(self, tensors, mask, image_sizes):
        """``tensors [B, 3, Hi, Wi]`` and ``mask [B, Hi, Wi]`` of the NestedTensor, ``image_sizes``: (h, w) per image as
        ``DetectionHeads.detect`` takes them.  Returns ``(results, hs [L, B, Q, C], memory [B, C, H, W])``."""
        feats = self.body(tensors)
        if isinstance(feats, dict):
            feats = feats[sorted(feats)[-1]]      # the last level: IntermediateLayerGetter's {'0': layer4}
        src, pos, kpm, hw = self.neck._run(feats, mask)
        hs, memory = self.transformer.forward_tokens(src, kpm, self.query_embed.weight, pos, hw)
        return self.heads.detect(hs, image_sizes), hs, memory
