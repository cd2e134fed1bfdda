"""Host-side behaviour of hoigen_amd.detr.DetectorNeck, Transformer.forward_tokens and Detector that needs no device: from_modules reads
the reference's modules and refuses what the HIP path does not implement, each with a message; CPU tensors, wrong shapes and gradient
callers are refused; the modules of a Detector share one context; the ctypes structs mirror the header field by field; the two symbols
are exported."""
import math
import os
import re

import pytest
import torch
from torch import nn

from hoigen_amd import _lib
from hoigen_amd.detr import BoxMLP, Detector, DetectorNeck, Transformer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sine(nn.Module):      # a stand-in with the attributes of PositionEmbeddingSine (detr/models/position_encoding.py:17-26)
    def __init__(self, num_pos_feats=64, temperature=10000, normalize=True, scale=None):
        super().__init__()
        self.num_pos_feats, self.temperature, self.normalize = num_pos_feats, temperature, normalize
        self.scale = 2 * math.pi if scale is None else scale


class _Learned(nn.Module):      # PositionEmbeddingLearned (position_encoding.py:51-62): embeddings, none of the sine's attributes
    def __init__(self):
        super().__init__()
        self.row_embed, self.col_embed = nn.Embedding(50, 64), nn.Embedding(50, 64)


def test_from_modules_reads_the_reference_modules():
    conv = nn.Conv2d(64, 128, kernel_size=1)
    m = DetectorNeck.from_modules(conv, _Sine(64, 20, False, 3.0))
    assert sorted(m.state_dict()) == ["input_proj.bias", "input_proj.weight"]
    assert torch.equal(m.input_proj.weight, conv.weight) and torch.equal(m.input_proj.bias, conv.bias)
    assert (m.in_channels, m.d_model, m.num_pos_feats, m.temperature, m.normalize, m.scale) == (64, 128, 64, 20.0, False, 3.0)
    assert DetectorNeck.from_modules(conv, _Sine()).scale == 2 * math.pi
    assert DetectorNeck.from_modules(conv.eval(), _Sine()).training is False


def test_from_modules_refuses_what_is_not_the_detector():
    with pytest.raises(RuntimeError, match="learned"):
        DetectorNeck.from_modules(nn.Conv2d(64, 128, 1), _Learned())
    with pytest.raises(RuntimeError, match="1 x 1"):
        DetectorNeck.from_modules(nn.Conv2d(64, 128, 3), _Sine())
    with pytest.raises(RuntimeError, match="1 x 1"):
        DetectorNeck.from_modules(nn.Linear(64, 128), _Sine())
    with pytest.raises(RuntimeError, match="stride"):
        DetectorNeck.from_modules(nn.Conv2d(64, 128, 1, stride=2), _Sine())
    with pytest.raises(RuntimeError, match="groups"):
        DetectorNeck.from_modules(nn.Conv2d(64, 128, 1, groups=2), _Sine())
    with pytest.raises(RuntimeError, match="bias"):
        DetectorNeck.from_modules(nn.Conv2d(64, 128, 1, bias=False), _Sine())
    with pytest.raises(RuntimeError, match="num_pos_feats"):
        DetectorNeck.from_modules(nn.Conv2d(64, 128, 1), _Sine(32))


def test_cpu_tensors_shapes_and_gradient_callers_are_refused():
    m = DetectorNeck.from_modules(nn.Conv2d(64, 128, 1), _Sine()).eval()
    x, im = torch.zeros(1, 64, 3, 5), torch.zeros(1, 90, 150, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(x, im)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference-only"):
            m(x.clone().requires_grad_(), im)
        m.train()
        with pytest.raises(RuntimeError, match="inference-only"):
            m(x, im)
        m.eval()
    t = Transformer(128, 4, 1, 1, 256, True).eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        t.forward_tokens(torch.zeros(1, 15, 128), None, torch.zeros(7, 128), torch.zeros(1, 15, 128), (3, 5))


class _Meta(torch.Tensor):      # shape checks come after the device check: a tensor that claims a HIP device without one
    is_cuda = True


def test_shape_and_dtype_errors():
    m = DetectorNeck.from_modules(nn.Conv2d(64, 128, 1), _Sine()).eval()
    fake = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype).as_subclass(_Meta)
    with pytest.raises(RuntimeError, match=r"\[B, 64, H, W\]"):
        m(fake(1, 32, 3, 5), fake(1, 90, 150, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="tokens, at most"):
        m(fake(1, 64, 43, 42), fake(1, 90, 150, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"image_mask must be \[B = 2"):
        m(fake(2, 64, 3, 5), fake(1, 90, 150, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="bool or uint8"):
        m(fake(1, 64, 3, 5), fake(1, 90, 150))
    t = Transformer(128, 4, 1, 1, 256, True).eval()
    with pytest.raises(RuntimeError, match="forward_tokens"):
        t.forward_tokens(fake(1, 15, 128), None, fake(7, 128), fake(1, 15, 128), (3, 4))
    with pytest.raises(RuntimeError, match="forward_tokens"):
        t.forward_tokens(fake(1, 15, 128), None, fake(7, 128), fake(1, 14, 128), (3, 5))


def test_a_detector_shares_one_context():
    detr = nn.Module()
    detr.backbone = nn.ModuleList([nn.Module(), _Sine(64)])
    detr.backbone[0].body = nn.Sequential(nn.Conv2d(3, 64, 32, stride=32), nn.ReLU())
    detr.input_proj = nn.Conv2d(64, 128, 1)
    detr.transformer = Transformer(128, 4, 1, 1, 256, True)
    detr.class_embed, detr.bbox_embed, detr.query_embed = nn.Linear(128, 17), BoxMLP(128), nn.Embedding(7, 128)
    d = Detector.from_module(detr.eval(), reserve_indices=[0, 3, 16])
    ctx = d.transformer.encoder._ctx
    assert d.neck._ctx is ctx and d.heads._ctx is ctx and d.transformer.decoder._ctx is ctx
    assert d.body is detr.backbone[0].body and d.heads.n_out == 3 and d.training is False
    with pytest.raises(RuntimeError, match="HIP device"):
        d(torch.zeros(1, 3, 64, 96), torch.zeros(1, 64, 96, dtype=torch.bool), [(64.0, 96.0)])


def test_abi_structs_match_the_header_and_the_symbols_are_exported():
    hdr = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^}]*)\} (\w+);", hdr))
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    for name in ("hg_detr_neck_weights", "hg_detr_neck_args"):
        fields = []
        for decl in strip(body[name]).split(";"):
            decl = decl.strip()
            if decl:      # `type a, *b, c[3]` -> a, b, c
                first, *rest = decl.split(",")
                fields += [re.sub(r"\[\d+\]", "", first.split()[-1]).lstrip("*")] + [re.sub(r"\[\d+\]", "", r_).strip().lstrip("*") for r_ in rest]
        assert fields == [f[0] for f in getattr(_lib, name)._fields_], (name, fields)
    assert re.search(r"int hg_load_detr_neck\(hg_ctx\*, const hg_detr_neck_weights\*\);", hdr)
    assert re.search(r"int hg_detr_neck\(hg_ctx\*, const hg_detr_neck_args\* args, void\* stream\);", hdr)
    assert re.search(r"#define HG_PROF_DETR_NECK (\d+)", hdr).group(1) == str(_lib.HG_PROF_DETR_NECK)
    assert '"detr_neck_split" [HG_DETR_NECK_SPLIT]' in hdr
    assert {"hg_load_detr_neck", "hg_detr_neck"} <= set(_lib.SIGNATURES)
    lib = _lib.lib()
    assert hasattr(lib, "hg_load_detr_neck") and hasattr(lib, "hg_detr_neck")
