"""Host-side behaviour of the DETR decoder façade that needs no device: the state-dict keys are the reference's (the names
tests/golden/make_golden_detr_decoder.py loads into the reference's own modules with strict=True), and from_module refuses what the HIP
path does not implement, each with a message that says so."""
import pytest
import torch
from torch import nn

import detr_decoder_cases as dd
import detr_encoder_cases as ec
from hoigen_amd import _lib
from hoigen_amd.detr import Transformer, TransformerDecoder


def test_state_dict_keys_are_the_reference_modules():
    cfg = dd.SMALL
    m = TransformerDecoder(cfg["d_model"], cfg["heads"], cfg["layers"], cfg["d_ff"], True)
    sd = dd.weights(cfg, 1)
    assert sorted(m.state_dict()) == sorted(sd)
    assert all(tuple(m.state_dict()[k].shape) == v.shape for k, v in sd.items())
    t = Transformer(cfg["d_model"], cfg["heads"], cfg["layers"], cfg["layers"], cfg["d_ff"], True)
    want = ["encoder." + k for k in ec.weights(cfg, 1)] + ["decoder." + k for k in sd]
    assert sorted(t.state_dict()) == sorted(want)
    assert t.decoder._ctx is t.encoder._ctx, "both halves run in one native context"


class _Layer(nn.Module):
    def __init__(self, d=128, h=4, f=256, activation=torch.nn.functional.relu, normalize_before=False):
        super().__init__()
        self.self_attn, self.multihead_attn = nn.MultiheadAttention(d, h), nn.MultiheadAttention(d, h)
        self.linear1, self.linear2 = nn.Linear(d, f), nn.Linear(f, d)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)
        self.activation, self.normalize_before = activation, normalize_before


class _Decoder(nn.Module):
    def __init__(self, norm=True, return_intermediate=True, **kw):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(**kw) for _ in range(2)])
        self.norm = nn.LayerNorm(128) if norm else None
        self.return_intermediate = return_intermediate


def test_from_module_copies_and_refuses():
    src = _Decoder(return_intermediate=False)
    m = TransformerDecoder.from_module(src)
    assert m.return_intermediate is False and m.num_layers == 2 and m.d_model == 128 and m.nhead == 4 and m.dim_feedforward == 256
    assert torch.equal(m.layers[1].multihead_attn.in_proj_weight, src.layers[1].multihead_attn.in_proj_weight)
    assert TransformerDecoder.from_module(_Decoder()).return_intermediate is True
    with pytest.raises(RuntimeError, match="pre-norm"):
        TransformerDecoder.from_module(_Decoder(normalize_before=True))
    with pytest.raises(RuntimeError, match="only ReLU"):
        TransformerDecoder.from_module(_Decoder(activation=torch.nn.functional.gelu))
    with pytest.raises(RuntimeError, match="no final norm"):
        TransformerDecoder.from_module(_Decoder(norm=False))


def test_masks_the_detector_leaves_at_none_and_cpu_tensors_are_refused():
    m = TransformerDecoder(128, 4, 2, 256, True).eval()
    mem, qp = torch.zeros(5, 1, 128), torch.zeros(3, 128)
    for name in ("tgt_mask", "memory_mask", "tgt_key_padding_mask"):
        with pytest.raises(RuntimeError, match=name):
            m(None, mem, query_pos=qp, **{name: torch.zeros(1, dtype=torch.bool)})
    with pytest.raises(RuntimeError):      # tensors must live on a HIP device
        m(None, mem, query_pos=qp)
    m.train()
    with torch.enable_grad(), pytest.raises(RuntimeError, match="inference-only"):
        m(None, mem, query_pos=qp)


def test_abi_structs_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hoigen_amd.h")).read()
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^}]*)\} (\w+);", hdr))
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    n_tensors = sum(len(d.split(",")) for d in re.findall(r"hg_tensor\s+([^;]+);", strip(body["hg_detr_dec_layer_weights"])))
    assert n_tensors == 18 == len(_lib.hg_detr_dec_layer_weights._fields_)
    names = re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", strip(body["hg_detr_decoder_args"]))
    assert names == [f[0] for f in _lib.hg_detr_decoder_args._fields_], names
