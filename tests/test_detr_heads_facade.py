"""Host-side behaviour of hoigen_amd.detr.DetectionHeads that needs no device: from_modules reads the reference's state-dict keys
(`weight`, `bias`; `layers.{0,1,2}.weight` / `bias`) and refuses what the HIP path does not implement, each with a message; CPU tensors
and gradient callers are refused; the ctypes structs mirror the header field by field; the two symbols are exported."""
import os
import re

import pytest
import torch
from torch import nn

import detr_heads_cases as hc
from hoigen_amd import _lib
from hoigen_amd.detr import DetectionHeads, Transformer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _MLP(nn.Module):      # a stand-in with the state-dict keys of the reference's MLP (detr/models/detr.py:293-305)
    def __init__(self, i, h, o, n):
        super().__init__()
        self.num_layers = n
        dims = [h] * (n - 1)
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip([i] + dims, dims + [o]))


def test_from_modules_reads_the_reference_keys():
    ce, be = nn.Linear(128, 17), _MLP(128, 128, 4, 3)
    m = DetectionHeads.from_modules(ce, be)
    assert sorted(m.state_dict()) == sorted(hc.weights(128, 17))
    assert all(tuple(m.state_dict()[k].shape) == v.shape for k, v in hc.weights(128, 17).items())
    assert m.d_model == 128 and m.num_logits == 17 and m.n_out == 17 and m.reserve_indices is None
    assert torch.equal(m.class_embed.weight, ce.weight) and torch.equal(m.bbox_embed.layers[2].bias, be.layers[2].bias)
    v = DetectionHeads.from_modules(ce, be, reserve_indices=torch.tensor([0, 3, 5, 16]))
    assert v.reserve_indices == [0, 3, 5, 16] and v.n_out == 4 and v.num_logits == 17
    assert DetectionHeads.from_modules(ce.eval(), be).training is False


def test_from_modules_refuses_what_is_not_the_detector():
    ce = nn.Linear(128, 17)
    with pytest.raises(RuntimeError, match="three-layer"):
        DetectionHeads.from_modules(ce, _MLP(128, 128, 4, 2))
    with pytest.raises(RuntimeError, match="three-layer"):
        DetectionHeads.from_modules(ce, _MLP(128, 128, 4, 4))
    with pytest.raises(RuntimeError, match="width"):
        DetectionHeads.from_modules(ce, _MLP(128, 64, 4, 3))
    with pytest.raises(RuntimeError, match="width"):
        DetectionHeads.from_modules(ce, _MLP(128, 128, 5, 3))
    with pytest.raises(RuntimeError, match="width"):
        DetectionHeads.from_modules(nn.Linear(256, 17), _MLP(128, 128, 4, 3))
    with pytest.raises(RuntimeError, match="class_embed"):
        DetectionHeads.from_modules(nn.LayerNorm(128), _MLP(128, 128, 4, 3))
    with pytest.raises(RuntimeError, match="reserve_indices"):
        DetectionHeads.from_modules(ce, _MLP(128, 128, 4, 3), reserve_indices=[0, 17])


def test_cpu_tensors_and_gradient_callers_are_refused():
    m = DetectionHeads.from_modules(nn.Linear(128, 17), _MLP(128, 128, 4, 3)).eval()
    hs = torch.zeros(1, 1, 3, 128)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(hs)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.detect(hs, [(4.0, 5.0)])
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference-only"):
            m(hs.clone().requires_grad_())
        with pytest.raises(RuntimeError, match="inference-only"):
            m.detect(hs.clone().requires_grad_(), [(4.0, 5.0)])
        m.train()
        with pytest.raises(RuntimeError, match="inference-only"):
            m(hs)
        for p in m.parameters():
            p.requires_grad_(False)
        with pytest.raises(RuntimeError, match="HIP device"):      # train() without trainable parameters passes the guard
            m(hs)


def test_the_heads_can_share_a_transformers_context():
    t = Transformer(128, 4, 1, 1, 256, True)
    m = DetectionHeads(128, 17)
    m._ctx = t.encoder._ctx
    assert m._ctx is t.decoder._ctx


def test_abi_structs_match_the_header_and_the_symbols_are_exported():
    hdr = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^}]*)\} (\w+);", hdr))
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    for name in ("hg_detr_heads_weights", "hg_detr_heads_args"):
        fields = []
        for decl in strip(body[name]).split(";"):
            decl = decl.strip()
            if decl:      # `type a, *b, c[3]` -> a, b, c
                first, *rest = decl.split(",")
                fields += [re.sub(r"\[\d+\]", "", first.split()[-1]).lstrip("*")] + [re.sub(r"\[\d+\]", "", r_).strip().lstrip("*") for r_ in rest]
        assert fields == [f[0] for f in getattr(_lib, name)._fields_], (name, fields)
    assert re.search(r"int hg_load_detr_heads\(hg_ctx\*, const hg_detr_heads_weights\*\);", hdr)
    assert re.search(r"int hg_detr_heads\(hg_ctx\*, const hg_detr_heads_args\* args, void\* stream\);", hdr)
    assert {"hg_load_detr_heads", "hg_detr_heads"} <= set(_lib.SIGNATURES)
    lib = _lib.lib()
    assert hasattr(lib, "hg_load_detr_heads") and hasattr(lib, "hg_detr_heads")
