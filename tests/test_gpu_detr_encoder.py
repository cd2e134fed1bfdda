"""The DETR encoder on the HIP path (hoigen_amd/detr.py -> hg_load_detr_encoder / hg_detr_encoder, hoigen_amd/csrc/hg_detr.hip) against
the float64 restatement of tests/detr_encoder_cases.py, the reference's recorded output (tests/golden/g18_detr_encoder*.npz) and a
torch module with the reference's state-dict keys.  Tolerance: the project's contract, relative L2 < 1e-3, for the whole tensor and for
the worst row.  Parity is shown on seeded Xavier weights: real DETR-R50 weights are not available to the tests."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import detr_encoder_cases as dc
from hoigen_amd import _lib
from hoigen_amd.detr import TransformerEncoder

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3
HG_ERR_INVALID, HG_ERR_NOT_LOADED = -1, -3


def build(cfg, seed):
    sd = dc.weights(cfg, seed)
    m = TransformerEncoder(cfg["d_model"], cfg["heads"], cfg["layers"], cfg["d_ff"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda().eval(), sd


@pytest.fixture(scope="module")
def small():
    return build(dc.SMALL, 3)


@pytest.fixture(scope="module")
def full():
    return build(dc.FULL, dc.G18["wseed"])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_trace(trace, want, what):
    worst = 0.0
    for l, w in enumerate(want):
        got = trace[l].cpu()
        dead = ~torch.isfinite(w).all(-1)
        assert torch.isnan(got[dead]).all(), f"{what} layer {l}: an image without a visible token must be NaN"
        assert torch.isfinite(got[~dead]).all(), f"{what} layer {l}: NaN outside such an image"
        if (~dead).any():
            e, r = dc.rel_l2(got, w)
            worst = max(worst, e, r)
            assert e < TOL and r < TOL, f"{what} layer {l}: rel L2 {e:.2e}, worst row {r:.2e}"
    return worst


@pytest.mark.parametrize("gh,gw", [(1, 1), (1, 33), (5, 7), (13, 17)])
def test_small_model_every_layer_against_fp64(small, gh, gw):
    m, sd = small
    cfg, worst = dc.SMALL, 0.0
    for B in (1, 2, 3):
        src, pos = dc.inputs(B, gh, gw, cfg["d_model"], 100 * B + gh * gw)
        for kind in dc.MASK_KINDS:
            mask = dc.mask_of(kind, B, gh, gw)
            want = dc.encoder_fp64(sd, cfg, src, pos, mask)
            out, trace = m.forward_trace(dev(src), src_key_padding_mask=dev(mask), pos=dev(pos))
            worst = max(worst, check_trace(trace, want, f"B {B} {gh}x{gw} {kind}"))
            flat = out.transpose(0, 1).reshape(-1, cfg["d_model"])      # (NaN rows of an image without a visible token compare equal)
            assert torch.equal(torch.nan_to_num(flat, nan=7e37), torch.nan_to_num(trace[-1], nan=7e37)), "out is the last layer's stream"
    print(f"DETR_ENC small {gh}x{gw}: worst rel L2 (tensor or row, any layer) {worst:.2e}")


@pytest.mark.parametrize("d_model", (384, 512, 640))
def test_wider_models_against_fp64(d_model):
    """d_model 384, 512 and 640 (12, 16 and 20 heads; one layer, d_ff 256): the second and third trips of the post-norm's loops, the GEMMs
    at N = 768 .. 1280 and the attention's head counts, with and without pos.  hg_load_detr_encoder takes every multiple of 128: 640
    stands for the widths beyond the decoder's 512."""
    cfg = dc.wide(d_model)
    m, sd = build(cfg, 30 + d_model // 128)
    B, gh, gw = 2, 5, 7
    src, pos = dc.inputs(B, gh, gw, d_model, 300 + d_model)
    mask = dc.mask_of("rect", B, gh, gw)
    for p in (pos, None):
        want = dc.encoder_fp64(sd, cfg, src, p, mask)
        out, trace = m.forward_trace(dev(src), src_key_padding_mask=dev(mask), pos=dev(p))
        worst = check_trace(trace, want, f"d_model {d_model} pos {p is not None}")
        assert torch.equal(out.transpose(0, 1).reshape(-1, d_model), trace[-1])
        print(f"DETR_ENC d_model {d_model} heads {cfg['heads']} pos {p is not None}: worst rel L2 (tensor or row) {worst:.2e}")


@pytest.mark.parametrize("kind", ("none", "rect", "perimage"))
def test_pos_none_against_fp64(small, kind):
    m, sd = small
    cfg = dc.SMALL
    for B, (gh, gw) in ((1, (5, 7)), (3, (13, 17))):
        src, _ = dc.inputs(B, gh, gw, cfg["d_model"], 40 + B)
        mask = dc.mask_of(kind, B, gh, gw)
        want = dc.encoder_fp64(sd, cfg, src, None, mask)
        _, trace = m.forward_trace(dev(src), src_key_padding_mask=dev(mask), pos=None)
        worst = check_trace(trace, want, f"pos None B {B} {gh}x{gw} {kind}")
        print(f"DETR_ENC small pos None B {B} {gh}x{gw} {kind}: worst rel L2 (tensor or row, any layer) {worst:.2e}")


def test_full_width_against_the_reference_fixture(full):
    m, _ = full
    g, cfg = dc.G18, dc.FULL
    src, pos = dc.inputs(g["B"], g["gh"], g["gw"], cfg["d_model"], g["xseed"])
    mask = dc.rect_mask(g["gh"], g["gw"], g["visible"])
    _, trace = m.forward_trace(dev(src), src_key_padding_mask=dev(mask), pos=dev(pos))
    for name, layer in (("g18_detr_encoder_l1.npz", 0), ("g18_detr_encoder.npz", cfg["layers"] - 1)):
        want = torch.from_numpy(np.load(os.path.join(GOLDEN, name))["out"]).transpose(0, 1).reshape(-1, cfg["d_model"])
        e, r = dc.rel_l2(trace[layer].cpu(), want)
        print(f"DETR_ENC g18 after layer {layer + 1}: rel L2 {e:.2e}, worst row {r:.2e}")
        assert e < TOL and r < TOL, (name, e, r)


def test_layouts_history_and_canaries(small):
    """[S, B, C] and [B, S, C] give the same bits; a call at B = 3, S = 221, one at B = 1, S = 35, then the first again gives the first's
    bits (workspace growth, stale masks); nothing is written around out and trace"""
    m, _ = small
    D, L = dc.SMALL["d_model"], dc.SMALL["layers"]
    src, pos = (dev(a) for a in dc.inputs(3, 13, 17, D, 7))
    mask = dev(dc.mask_of("perimage", 3, 13, 17))
    S, B = src.shape[:2]
    out_buf = torch.full((S + 2, B, D), float("nan"), device="cuda")
    tr_buf = torch.full((L + 2, B * S, D), float("nan"), device="cuda")
    first, _ = m.forward_trace(src, src_key_padding_mask=mask, pos=pos, out=out_buf[1:-1], trace=tr_buf[1:-1])
    first, tr_first = first.clone(), tr_buf[1:-1].clone()
    assert torch.isnan(out_buf[0]).all() and torch.isnan(out_buf[-1]).all() and torch.isnan(tr_buf[0]).all() and torch.isnan(tr_buf[-1]).all()
    assert torch.isfinite(first).all()
    s2, p2 = (dev(a) for a in dc.inputs(1, 5, 7, D, 8))
    m(s2, src_key_padding_mask=dev(dc.mask_of("one", 1, 5, 7)), pos=p2)
    again = m(src, src_key_padding_mask=mask, pos=pos)
    assert torch.equal(again, first), "history"
    # batch-first buffers seen through [S, B, C] views: strides (C, S * C, 1)
    bf = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)
    out_bf = torch.empty(B, S, D, device="cuda")
    assert bf(src).stride() == (D, S * D, 1)
    m.forward_trace(bf(src), src_key_padding_mask=mask, pos=bf(pos), out=out_bf.transpose(0, 1))
    assert torch.equal(out_bf.transpose(0, 1), first), "layouts"
    # pos = None, no mask: runs, and differs
    assert not torch.equal(m(src), first)


def test_error_returns(small):
    m, _ = small
    lib = _lib.lib()
    D = dc.SMALL["d_model"]
    h = lib.hg_create(0)
    try:
        x = torch.zeros(4, 1, D, device="cuda")
        out = torch.full_like(x, float("nan"))

        def call(B, S, cstride=1):
            a = _lib.hg_detr_encoder_args()
            a.src, a.out, a.B, a.S = x.data_ptr(), out.data_ptr(), B, S
            a.src_stride[:] = [D, D, cstride]
            a.out_stride[:] = [D, D, 1]
            return lib.hg_detr_encoder(h, C.byref(a), None)

        assert call(1, 4) == HG_ERR_NOT_LOADED
        t = _lib.tensor
        layers = (_lib.hg_detr_layer_weights * 2)()
        for i, l in enumerate(m.layers):
            layers[i] = _lib.hg_detr_layer_weights(t(l.self_attn.in_proj_weight), t(l.self_attn.in_proj_bias), t(l.self_attn.out_proj.weight),
                                                   t(l.self_attn.out_proj.bias), t(l.linear1.weight), t(l.linear1.bias), t(l.linear2.weight),
                                                   t(l.linear2.bias), t(l.norm1.weight), t(l.norm1.bias), t(l.norm2.weight), t(l.norm2.bias))
        cfg = dc.SMALL
        for bad in (dict(normalize_before=1), dict(activation=1), dict(n_layers=13), dict(n_layers=0), dict(heads=3), dict(d_ff=200)):
            kw = dict(d_model=cfg["d_model"], heads=cfg["heads"], d_ff=cfg["d_ff"], n_layers=2, normalize_before=0, activation=0)
            kw.update(bad)
            w = _lib.hg_detr_encoder_weights(kw["d_model"], kw["heads"], kw["d_ff"], kw["n_layers"], kw["normalize_before"], kw["activation"], layers)
            assert lib.hg_load_detr_encoder(h, C.byref(w)) == HG_ERR_INVALID, bad
            assert lib.hg_last_error(h), bad
        assert call(1, 4) == HG_ERR_NOT_LOADED
        w = _lib.hg_detr_encoder_weights(cfg["d_model"], cfg["heads"], cfg["d_ff"], 2, 0, 0, layers)
        assert lib.hg_load_detr_encoder(h, C.byref(w)) == 0, lib.hg_last_error(h)
        for B, S, cs in ((0, 4, 1), (1, 0, 1), (1, 1793, 1), (1, 4, 2)):
            assert call(B, S, cs) == HG_ERR_INVALID, (B, S, cs)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused call wrote something"
        assert call(1, 4) == 0, lib.hg_last_error(h)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
    finally:
        lib.hg_destroy(h)
    with pytest.raises(RuntimeError, match="attention mask"):
        m(torch.zeros(4, 1, D, device="cuda"), mask=torch.zeros(4, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="grad"):
        with torch.enable_grad():
            m(torch.zeros(4, 1, D, device="cuda", requires_grad=True))


class _RefLayer(nn.Module):
    """a module with the reference layer's attribute names (detr/models/transformer.py:127-162), built from torch's own modules"""

    def __init__(self, d, h, f):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, h, dropout=0.1)
        self.linear1, self.linear2 = nn.Linear(d, f), nn.Linear(f, d)
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.activation, self.normalize_before = torch.nn.functional.relu, False

    def forward(self, src, kpm, pos):
        q = k = src + pos
        src = self.norm1(src + self.self_attn(q, k, value=src, key_padding_mask=kpm)[0])
        return self.norm2(src + self.linear2(self.activation(self.linear1(src))))


class _RefEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_RefLayer(cfg["d_model"], cfg["heads"], cfg["d_ff"]) for _ in range(cfg["layers"])])
        self.norm = None

    def forward(self, src, mask=None, src_key_padding_mask=None, pos=None):
        for l in self.layers:
            src = l(src, src_key_padding_mask, pos)
        return src


def test_drop_in_from_module_on_a_padded_full_size_batch():
    """from_module on a torch module with the reference's key names; B = 2 on a 25 x 38 grid (950 tokens), image 1 padded: against that
    module's own fp32 output on the device.  The only full-size encoder run."""
    cfg = dc.FULL
    ref = _RefEncoder(cfg)
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in dc.weights(cfg, 21).items()})
    ref = ref.cuda().eval()
    enc = TransformerEncoder.from_module(ref)
    assert sorted(enc.state_dict()) == sorted(ref.state_dict())
    src, pos = (dev(a) for a in dc.inputs(2, 25, 38, cfg["d_model"], 22))
    mask = dev(dc.rect_mask(25, 38, ((25, 38), (19, 25)))).bool()
    with torch.no_grad():
        want = ref(src, src_key_padding_mask=mask, pos=pos)
        got = enc(src, src_key_padding_mask=mask, pos=pos)
    e, r = dc.rel_l2(got.reshape(-1, cfg["d_model"]).cpu(), want.reshape(-1, cfg["d_model"]).cpu())
    print(f"DETR_ENC drop-in B 2 25x38: rel L2 {e:.2e}, worst row {r:.2e}")
    assert e < TOL and r < TOL
    with_norm = _RefEncoder(dc.SMALL)
    with_norm.norm = nn.LayerNorm(dc.SMALL["d_model"])
    with pytest.raises(RuntimeError, match="final norm"):
        TransformerEncoder.from_module(with_norm)
    pre = _RefEncoder(dc.SMALL)
    pre.layers[1].normalize_before = True
    with pytest.raises(RuntimeError, match="pre-norm"):
        TransformerEncoder.from_module(pre)
    train = TransformerEncoder.from_module(_RefEncoder(dc.SMALL).cuda().train())
    with pytest.raises(RuntimeError, match="train"):
        with torch.enable_grad():
            train(torch.zeros(4, 1, dc.SMALL["d_model"], device="cuda"))
