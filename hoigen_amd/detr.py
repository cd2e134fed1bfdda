"""DETR transformer encoder façade: the reference's ``TransformerEncoder`` (detr/models/transformer.py:62-83 over the post-norm
``TransformerEncoderLayer`` :127-162) with the same state-dict keys and call signature, running on the HIP kernels
(hoigen_amd/csrc/hg_detr.hip: hg_load_detr_encoder, hg_detr_encoder).

    self.detector.transformer.encoder = TransformerEncoder.from_module(self.detector.transformer.encoder)

is the whole integration.  Inference only; tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib
from .model import LayerNorm, Linear, MultiheadAttention, _Ctx, _inference_only, _require_cuda, _sig, _stream_ptr

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


class TransformerEncoder(nn.Module):
    """detr/models/transformer.py:62-83.  ``forward(src, mask=None, src_key_padding_mask=None, pos=None)`` on ``[S, B, C]`` tensors
    returns ``[S, B, C]`` fp32.  Post-norm ReLU layers without a final norm - what the detector builds (transformer.py:26-29 with
    normalize_before = False); anything else is refused."""

    def __init__(self, d_model: int = 256, nhead: int = 8, num_layers: int = 6, dim_feedforward: int = 2048):
        super().__init__()
        self.d_model, self.nhead, self.num_layers, self.dim_feedforward = d_model, nhead, num_layers, dim_feedforward
        self.layers = nn.ModuleList([TransformerEncoderLayer(d_model, nhead, dim_feedforward) for _ in range(num_layers)])
        self.norm = None
        self._ctx = _Ctx()
        self._sig = None

    @classmethod
    def from_module(cls, encoder: nn.Module) -> "TransformerEncoder":
        """From the reference's TransformerEncoder (or any module with its attributes and state-dict keys
        ``layers.N.self_attn.in_proj_weight`` / ``in_proj_bias`` / ``out_proj.*``, ``linear1``, ``linear2``, ``norm1``, ``norm2``)."""
        if getattr(encoder, "norm", None) is not None:
            raise RuntimeError("hoigen_amd: TransformerEncoder.from_module: a final norm (the pre-norm encoder, transformer.py:28) is not "
                               "implemented; the detector's encoder is post-norm and has none")
        layers = list(encoder.layers)
        if not layers:
            raise RuntimeError("hoigen_amd: TransformerEncoder.from_module: the encoder has no layers")
        for i, l in enumerate(layers):
            if getattr(l, "normalize_before", False):
                raise RuntimeError(f"hoigen_amd: TransformerEncoder.from_module: layers.{i} is pre-norm (normalize_before); only the post-norm "
                                   "layer (transformer.py:149-162) is implemented")
            act = getattr(l, "activation", torch.nn.functional.relu)
            if not _is_relu(act):
                raise RuntimeError(f"hoigen_amd: TransformerEncoder.from_module: layers.{i} uses activation {act!r}; only ReLU is implemented")
        w = layers[0].self_attn.in_proj_weight
        d_model, nhead, d_ff = int(w.shape[1]), int(layers[0].self_attn.num_heads), int(layers[0].linear1.weight.shape[0])
        m = cls(d_model, nhead, len(layers), d_ff)
        missing, unexpected = m.load_state_dict(encoder.state_dict(), strict=False)
        if missing or unexpected:
            raise RuntimeError(f"hoigen_amd: TransformerEncoder.from_module: state-dict keys differ (missing {missing}, unexpected {unexpected})")
        m.to(device=w.device, dtype=w.dtype)
        m.train(encoder.training)
        return m

    def set_option(self, key: str, value: int) -> None:
        """Behaviour option of this module's native context (include/hoigen_amd.h), e.g. ``detr_attn_chunk``."""
        self._ctx.set_option(key, value)

    def get_option(self, key: str):
        return self._ctx.get_option(key)

    def _load(self, device: torch.device) -> int:
        h = self._ctx.get(device)
        sig = (h, _sig(self.parameters()))
        if sig != self._sig:
            t = _lib.tensor
            arr = (_lib.hg_detr_layer_weights * self.num_layers)()
            for i, l in enumerate(self.layers):
                arr[i] = _lib.hg_detr_layer_weights(
                    t(l.self_attn.in_proj_weight), t(l.self_attn.in_proj_bias), t(l.self_attn.out_proj.weight), t(l.self_attn.out_proj.bias),
                    t(l.linear1.weight), t(l.linear1.bias), t(l.linear2.weight), t(l.linear2.bias), t(l.norm1.weight), t(l.norm1.bias),
                    t(l.norm2.weight), t(l.norm2.bias))
            w = _lib.hg_detr_encoder_weights(self.d_model, self.nhead, self.dim_feedforward, self.num_layers, 0, 0, arr)
            self._ctx.check(_lib.lib().hg_load_detr_encoder(h, C.byref(w)), "hg_load_detr_encoder")
            self._sig = sig
        return h

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

        def f32(t):      # fp32 with a channel stride of 1: the [S, B, C] view of a [B, C, H, W] map (flatten(2).permute(2, 0, 1)) is copied
            t = t.detach()
            return t if t.dtype == torch.float32 and t.stride(2) == 1 else t.to(torch.float32).contiguous()

        x = f32(src)
        p = None
        if pos is not None:
            _require_cuda(pos, "TransformerEncoder pos")
            p = f32(pos).expand(S, B, D)
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
