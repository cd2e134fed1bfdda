"""The DETR decoder and the whole transformer on the HIP path (hoigen_amd/detr.py -> hg_load_detr_decoder / hg_detr_decoder,
hoigen_amd/csrc/hg_detr_dec.hip) against the float64 restatement of tests/detr_decoder_cases.py, the reference's recorded outputs
(tests/golden/g19_detr_*.npz) and a torch module with the reference's attribute names.  Tolerance: the project's contract, relative L2
< 1e-3, for the whole tensor and for the worst row.  Parity is shown on seeded Xavier weights: real DETR-R50 weights are not available."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import detr_decoder_cases as dd
import detr_encoder_cases as ec
from hoigen_amd import _lib
from hoigen_amd.detr import Transformer, TransformerDecoder, TransformerEncoder

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3
HG_ERR_INVALID, HG_ERR_NOT_LOADED = -1, -3


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(cfg, seed, return_intermediate=True):
    sd = dd.weights(cfg, seed)
    m = TransformerDecoder(cfg["d_model"], cfg["heads"], cfg["layers"], cfg["d_ff"], return_intermediate)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda().eval(), sd


@pytest.fixture(scope="module")
def small():
    return build(dd.SMALL, 4)


@pytest.fixture(scope="module")
def full():
    return build(dd.FULL, dd.G19["wseed"])


def check(got, want, what):
    """got, want [rows, D]: NaN in the same rows, relative L2 below TOL on the rest (whole tensor and worst row)"""
    got, want = got.cpu(), torch.as_tensor(want)
    dead = ~torch.isfinite(want).all(-1)
    assert torch.isnan(got[dead]).all(), f"{what}: an image without a visible memory token must be NaN"
    assert torch.isfinite(got[~dead]).all(), f"{what}: NaN outside such an image"
    if not (~dead).any():
        return 0.0
    e, r = dd.rel_l2(got, want)
    assert e < TOL and r < TOL, f"{what}: rel L2 {e:.2e}, worst row {r:.2e}"
    return max(e, r)


def check_all(hs, trace, want_streams, want_hs, what):
    worst = 0.0
    D = hs.shape[-1]
    for l, w in enumerate(want_streams):
        worst = max(worst, check(trace[l], w, f"{what} stream after layer {l}"))
        worst = max(worst, check(hs[l].transpose(0, 1).reshape(-1, D), want_hs[l].transpose(0, 1).reshape(-1, D), f"{what} hs[{l}]"))
    return worst


# (Q, B, mask kind) per memory grid: every Q, every B, every mask kind of detr_encoder_cases.mask_of at least once per grid
COMBOS = ((1, 1, "none"), (1, 3, "rect"), (33, 2, "one"), (33, 3, "perimage"), (100, 1, "head64"), (100, 2, "midrun"), (100, 3, "rect"),
          (33, 1, "rect"), (1, 2, "perimage"))


@pytest.mark.parametrize("gh,gw", [(1, 1), (5, 7), (13, 17)])
def test_small_model_every_layer_against_fp64(small, gh, gw):
    m, sd = small
    cfg, worst = dd.SMALL, 0.0
    for Q, B, kind in COMBOS:
        qe, mem, pos = dd.inputs(B, gh, gw, Q, cfg["d_model"], 100 * B + gh * gw + Q)
        mask = ec.mask_of(kind, B, gh, gw)
        want_s, want_hs = dd.decoder_fp64(sd, cfg, mem, pos, mask, qe)
        hs, trace = m.forward_trace(None, dev(mem), memory_key_padding_mask=dev(mask), pos=dev(pos), query_pos=dev(qe))
        assert tuple(hs.shape) == (cfg["layers"], Q, B, cfg["d_model"])
        worst = max(worst, check_all(hs, trace, want_s, want_hs, f"Q {Q} B {B} {gh}x{gw} {kind}"))
    print(f"DETR_DEC small {gh}x{gw}: worst rel L2 (tensor or row, any layer) {worst:.2e}")


@pytest.mark.parametrize("d_model", (384, 512))
def test_wider_models_against_fp64(d_model):
    """d_model 384 and 512 (12 and 16 heads; one layer, d_ff 256), the widths hg_load_detr_decoder takes beyond the detector's: the
    tail's second register piece (partly filled at 384), the stacked K / V GEMMs, on the default FFN rule and on the two GEMMs, with
    and without the memory's pos"""
    cfg = ec.wide(d_model)
    m, sd = build(cfg, 50 + d_model // 128)
    B, gh, gw, Q = 2, 5, 7, 33
    qe, mem, pos = dd.inputs(B, gh, gw, Q, d_model, 500 + d_model)
    mask = ec.mask_of("rect", B, gh, gw)
    try:
        for option in (0, 1):
            m.set_option("detr_ffn", option)
            for p in (pos, None):
                want_s, want_hs = dd.decoder_fp64(sd, cfg, mem, p, mask, qe)
                hs, trace = m.forward_trace(None, dev(mem), memory_key_padding_mask=dev(mask), pos=dev(p), query_pos=dev(qe))
                worst = check_all(hs, trace, want_s, want_hs, f"d_model {d_model} detr_ffn {option} pos {p is not None}")
                print(f"DETR_DEC d_model {d_model} heads {cfg['heads']} detr_ffn {option} pos {p is not None}: worst rel L2 {worst:.2e}")
    finally:
        m.set_option("detr_ffn", 0)


@pytest.mark.parametrize("option", [1, 2])
def test_memory_pos_none_against_fp64(small, option):
    m, sd = small
    cfg = dd.SMALL
    m.set_option("detr_ffn", option)
    try:
        for Q, B, kind in ((1, 1, "none"), (33, 3, "rect"), (33, 2, "perimage")):
            qe, mem, _ = dd.inputs(B, 5, 7, Q, cfg["d_model"], 60 + Q + B)
            mask = ec.mask_of(kind, B, 5, 7)
            want_s, want_hs = dd.decoder_fp64(sd, cfg, mem, None, mask, qe)
            hs, trace = m.forward_trace(None, dev(mem), memory_key_padding_mask=dev(mask), pos=None, query_pos=dev(qe))
            worst = check_all(hs, trace, want_s, want_hs, f"memory pos None Q {Q} B {B} {kind} detr_ffn {option}")
            print(f"DETR_DEC small memory pos None Q {Q} B {B} {kind} detr_ffn {option}: worst rel L2 {worst:.2e}")
    finally:
        m.set_option("detr_ffn", 0)


@pytest.mark.parametrize("option", [1, 2])
def test_an_image_without_a_visible_memory_token_is_nan_alone(small, option):
    m, sd = small
    cfg = dd.SMALL
    m.set_option("detr_ffn", option)
    try:
        qe, mem, pos = dd.inputs(3, 5, 7, 33, cfg["d_model"], 77)
        mask = ec.mask_of("rect", 3, 5, 7)
        mask[1] = 1
        want_s, want_hs = dd.decoder_fp64(sd, cfg, mem, pos, mask, qe)
        assert not torch.isfinite(want_hs[:, :, 1]).any() and torch.isfinite(want_hs[:, :, 0]).all() and torch.isfinite(want_hs[:, :, 2]).all()
        hs, trace = m.forward_trace(None, dev(mem), memory_key_padding_mask=dev(mask), pos=dev(pos), query_pos=dev(qe))
        check_all(hs, trace, want_s, want_hs, f"dead image, detr_ffn {option}")
        assert torch.isnan(hs[:, :, 1]).all() and torch.isfinite(hs[:, :, 0]).all() and torch.isfinite(hs[:, :, 2]).all()
    finally:
        m.set_option("detr_ffn", 0)


def g19_inputs():
    g, D = dd.G19, dd.FULL["d_model"]
    qe, mem, pos = dd.inputs(g["B"], g["gh"], g["gw"], g["Q"], D, g["xseed"])
    return qe, mem, pos, ec.rect_mask(g["gh"], g["gw"], g["visible"])


def test_full_width_against_the_reference_fixture(full):
    m, _ = full
    qe, mem, pos, mask = g19_inputs()
    fix = np.load(os.path.join(GOLDEN, "g19_detr_decoder.npz"))
    for option in (2, 1):
        m.set_option("detr_ffn", option)
        hs = m(torch.zeros(100, 3, 256, device="cuda"), dev(mem), memory_key_padding_mask=dev(mask), pos=dev(pos), query_pos=dev(qe))
        for name, layer in (("hs0", 0), ("hs_last", 5)):
            e, r = dd.rel_l2(hs[layer].cpu(), fix[name])
            print(f"DETR_DEC g19 hs[{layer}] detr_ffn {option}: rel L2 {e:.2e}, worst row {r:.2e}")
            assert e < TOL and r < TOL, (name, option, e, r)
    m.set_option("detr_ffn", 0)


def test_transformer_full_width(full):
    g, cfg = dd.G19, dd.FULL
    D = cfg["d_model"]
    t = Transformer(D, cfg["heads"], cfg["layers"], cfg["layers"], cfg["d_ff"], True)
    t.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in ec.weights(cfg, g["enc_wseed"]).items()})
    t.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in dd.weights(cfg, g["wseed"]).items()})
    t = t.cuda().eval()
    src, pos_map = (dev(a) for a in dd.src_map(g["B"], g["gh"], g["gw"], D, g["xseed"]))
    qe = dev(dd.inputs(g["B"], g["gh"], g["gw"], g["Q"], D, g["xseed"])[0])
    mask = dev(ec.rect_mask(g["gh"], g["gw"], g["visible"])).bool().view(g["B"], g["gh"], g["gw"])
    hs, memory = t(src, mask, qe, pos_map)
    assert tuple(hs.shape) == (6, 3, 100, D) and tuple(memory.shape) == (3, D, 13, 17) and hs.is_contiguous()
    # the two halves called separately, in the reference's layouts
    enc, dec = TransformerEncoder.from_module(t.encoder), TransformerDecoder.from_module(t.decoder)
    sbc = lambda a: a.flatten(2).permute(2, 0, 1)
    mem2 = enc(sbc(src), src_key_padding_mask=mask.flatten(1), pos=sbc(pos_map))
    hs2, trace = dec.forward_trace(torch.zeros(100, 3, D, device="cuda"), mem2, memory_key_padding_mask=mask.flatten(1), pos=sbc(pos_map),
                                   query_pos=qe.unsqueeze(1).repeat(1, 3, 1))
    assert torch.equal(memory, mem2.permute(1, 2, 0).reshape(3, D, 13, 17)), "memory is hg_detr_encoder's output"
    assert torch.equal(hs, hs2.transpose(1, 2)), "hs is the decoder's output on that memory"
    want = np.load(os.path.join(GOLDEN, "g19_detr_transformer.npz"))["hs_last"]
    e, r = dd.rel_l2(hs[-1].reshape(-1, D).cpu(), want.reshape(-1, D))
    print(f"DETR_TRANSFORMER g19 hs[-1] after 6 + 6 layers: rel L2 {e:.2e}, worst row {r:.2e}")
    assert e < TOL, e


def test_plumbing_layouts_tgt_history_options(small):
    m, sd = small
    cfg = dd.SMALL
    D, L, Q, B = cfg["d_model"], cfg["layers"], 33, 3
    qe, mem, pos = (dev(a) for a in dd.inputs(B, 13, 17, Q, D, 9))
    mask = dev(ec.mask_of("perimage", B, 13, 17))
    kw = dict(memory_key_padding_mask=mask, pos=pos)
    buf = torch.full((L + 2, Q, B, D), float("nan"), device="cuda")
    first, tr = m.forward_trace(None, mem, query_pos=qe, out=buf[1:-1], **kw)
    first = first.clone()
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all() and torch.isfinite(first).all()
    # [L, B, Q, C] through strides; query_pos [Q, B, C]; an explicit zero tgt; batch-first memory and pos
    lbqc = torch.empty(L, B, Q, D, device="cuda")
    m.forward_trace(None, mem, query_pos=qe, out=lbqc.transpose(1, 2), **kw)
    assert torch.equal(lbqc.transpose(1, 2), first), "[L, B, Q, C] output"
    assert torch.equal(m(None, mem, query_pos=qe.unsqueeze(1).repeat(1, B, 1), **kw), first), "query_pos [Q, B, C]"
    assert torch.equal(m(torch.zeros(Q, B, D, device="cuda"), mem, query_pos=qe, **kw), first), "tgt = zeros"
    bf = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)
    assert torch.equal(m(None, bf(mem), query_pos=qe, memory_key_padding_mask=mask, pos=bf(pos)), first), "batch-first memory"
    # a tgt that is not zero is read
    tgt = 0.5 * torch.randn(Q, B, D, generator=torch.Generator().manual_seed(3))
    hs_t, tr_t = m.forward_trace(tgt.cuda(), mem, query_pos=qe, **kw)
    assert not torch.equal(hs_t, first)
    want_s, want_hs = dd.decoder_fp64(sd, cfg, mem.cpu().numpy(), pos.cpu().numpy(), mask.cpu().numpy(), qe.cpu().numpy(), tgt=tgt.numpy())
    check_all(hs_t, tr_t, want_s, want_hs, "non-zero tgt")
    # history: a small call in between, then the first again
    q2, m2, p2 = (dev(a) for a in dd.inputs(1, 5, 7, 1, D, 10))
    m(None, m2, memory_key_padding_mask=dev(ec.mask_of("one", 1, 5, 7)), pos=p2, query_pos=q2)
    assert torch.equal(m(None, mem, query_pos=qe, **kw), first), "history"
    # the attention kernel's chunk sizes, and both FFN paths' bits are each their own
    for chunk in (32, 96, 1280):
        m.set_option("detr_attn_chunk", chunk)
        assert torch.equal(m(None, mem, query_pos=qe, **kw), first), f"detr_attn_chunk {chunk}"
    m.set_option("detr_attn_chunk", 0)
    m.set_option("detr_ffn", 2)
    assert torch.equal(m(None, mem, query_pos=qe, **kw), first), "99 rows: the default rule runs the split kernel"
    m.set_option("detr_ffn", 0)
    # without return_intermediate: out[0] = hs[-1], nothing else written
    m1, _ = build(cfg, 4, return_intermediate=False)
    buf1 = torch.full((3, Q, B, D), float("nan"), device="cuda")
    m1.forward_trace(None, mem, query_pos=qe, out=buf1[1:2], **kw)
    assert torch.equal(buf1[1], first[-1]) and torch.isnan(buf1[0]).all() and torch.isnan(buf1[2]).all()
    assert tuple(m1(None, mem, query_pos=qe, **kw).shape) == (1, Q, B, D)


def raw_args(out, mem, qp, B, S, Q, D, L):
    a = _lib.hg_detr_decoder_args()
    a.query_pos, a.memory, a.out = qp.data_ptr(), mem.data_ptr(), out.data_ptr()
    a.B, a.S, a.Q, a.return_intermediate = B, S, Q, 1
    a.query_pos_stride[:] = [0, D, 1]
    a.memory_stride[:] = [S * D, D, 1]
    a.out_stride[:] = [B * Q * D, Q * D, D, 1]
    return a


def test_refusals_leave_out_untouched_and_the_slots_are_independent(small):
    lib = _lib.lib()
    cfg = dd.SMALL
    D, L = cfg["d_model"], cfg["layers"]
    h = lib.hg_create(0)
    assert h
    try:
        B, S, Q = 2, 35, 7
        mem, qp = torch.randn(B, S, D, device="cuda"), torch.randn(Q, D, device="cuda")
        out = torch.full((L, B, Q, D), float("nan"), device="cuda")
        a = raw_args(out, mem, qp, B, S, Q, D, L)
        assert lib.hg_detr_decoder(h, C.byref(a), None) == HG_ERR_NOT_LOADED
        # an encoder first, then a decoder beside it: the encoder's output keeps its bits
        enc = TransformerEncoder(D, cfg["heads"], L, cfg["d_ff"]).cuda().eval()
        dec, _ = small
        enc._ctx.handle, enc._ctx.device_index = h, 0
        src = torch.randn(S, B, D, device="cuda")
        try:
            e0 = enc(src)
            ctx_of_dec = dec._ctx
            dec._ctx, dec._sig = enc._ctx, None
            try:
                assert lib.hg_detr_decoder(h, C.byref(a), None) == HG_ERR_NOT_LOADED
                d0 = dec(None, mem.transpose(0, 1), query_pos=qp)
                assert torch.equal(enc(src), e0), "loading a decoder disturbed the encoder"
                enc._sig = None
                assert torch.equal(enc(src), e0)      # the encoder loaded again
                assert torch.equal(dec(None, mem.transpose(0, 1), query_pos=qp), d0), "loading an encoder disturbed the decoder"
            finally:
                dec._ctx, dec._sig = ctx_of_dec, None
        finally:
            enc._ctx.handle = None
        assert lib.hg_detr_decoder(h, C.byref(a), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.transpose(1, 2), d0)
        out.fill_(float("nan"))
        bad = []
        for field, value in (("B", 0), ("S", 0), ("Q", 0), ("S", 1793), ("Q", 1793), ("memory", None), ("query_pos", None), ("out", None)):
            b = raw_args(out, mem, qp, B, S, Q, D, L)
            setattr(b, field, value)
            bad.append((field, value, b))
        for field in ("memory_stride", "query_pos_stride", "out_stride"):
            b = raw_args(out, mem, qp, B, S, Q, D, L)
            getattr(b, field)[-1] = 2
            bad.append((field, 2, b))
        b = raw_args(out, mem, qp, 1025, 1024, Q, D, L)      # B * max(S, Q) > 2^20
        bad.append(("B * S", 1025 * 1024, b))
        b = raw_args(out, mem, qp, B, S, Q, D, L)
        b.tgt = mem.data_ptr()
        b.tgt_stride[:] = [Q * D, D, 3]
        bad.append(("tgt_stride", 3, b))
        for field, value, b in bad:
            assert lib.hg_detr_decoder(h, C.byref(b), None) == HG_ERR_INVALID, (field, value)
            assert lib.hg_last_error(h)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused call wrote into out"
    finally:
        lib.hg_destroy(h)


class _RefLayer(nn.Module):
    def __init__(self, d, h, f, cross):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, h, dropout=0.0)
        if cross:
            self.multihead_attn = nn.MultiheadAttention(d, h, dropout=0.0)
            self.norm3 = nn.LayerNorm(d)
        self.linear1, self.linear2 = nn.Linear(d, f), nn.Linear(f, d)
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.activation, self.normalize_before = torch.nn.functional.relu, False


class _RefStack(nn.Module):
    def __init__(self, layers, norm=None, return_intermediate=False):
        super().__init__()
        self.layers, self.norm, self.return_intermediate = nn.ModuleList(layers), norm, return_intermediate


class _RefTransformer(nn.Module):
    """a torch module with the reference's attribute names (transformer.py:18-59), its forward written out with torch's own ops"""

    def __init__(self, d=256, h=8, n=6, f=2048):
        super().__init__()
        self.encoder = _RefStack([_RefLayer(d, h, f, False) for _ in range(n)])
        self.decoder = _RefStack([_RefLayer(d, h, f, True) for _ in range(n)], nn.LayerNorm(d), True)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
            else:
                nn.init.normal_(p, 1.0 if p.shape[0] == d and p.mean() > 0.5 else 0.0, 0.1)

    def forward(self, src, mask, query_embed, pos_embed):
        bs, c, h, w = src.shape
        x, pos = src.flatten(2).permute(2, 0, 1), pos_embed.flatten(2).permute(2, 0, 1)
        qp, kpm = query_embed.unsqueeze(1).repeat(1, bs, 1), mask.flatten(1)
        for l in self.encoder.layers:
            x = l.norm1(x + l.self_attn(x + pos, x + pos, x, key_padding_mask=kpm)[0])
            x = l.norm2(x + l.linear2(torch.relu(l.linear1(x))))
        t, hs = torch.zeros_like(qp), []
        for l in self.decoder.layers:
            t = l.norm1(t + l.self_attn(t + qp, t + qp, t)[0])
            t = l.norm2(t + l.multihead_attn(t + qp, x + pos, x, key_padding_mask=kpm)[0])
            t = l.norm3(t + l.linear2(torch.relu(l.linear1(t))))
            hs.append(self.decoder.norm(t))
        return torch.stack(hs).transpose(1, 2), x.permute(1, 2, 0).view(bs, c, h, w)


def test_drop_in_for_a_torch_module_at_full_size():
    torch.manual_seed(21)
    ref = _RefTransformer().cuda().eval()
    B, D, gh, gw = 2, 256, 25, 38
    src, pos = torch.randn(B, D, gh, gw, device="cuda"), torch.randn(B, D, gh, gw, device="cuda")
    qe = torch.randn(100, D, device="cuda")
    mask = torch.zeros(B, gh, gw, dtype=torch.bool, device="cuda")
    mask[1, 19:], mask[1, :, 30:] = True, True
    with torch.no_grad():
        want_hs, want_mem = ref(src, mask, qe, pos)
    ours = Transformer.from_module(ref)
    assert sorted(ours.state_dict()) == sorted(ref.state_dict())
    hs, mem = ours(src, mask, qe, pos)
    assert hs.shape == want_hs.shape and mem.shape == want_mem.shape
    e_m, r_m = dd.rel_l2(mem.permute(0, 2, 3, 1).reshape(-1, D).cpu(), want_mem.permute(0, 2, 3, 1).reshape(-1, D).cpu())
    worst = 0.0
    for l in range(6):
        e, r = dd.rel_l2(hs[l].reshape(-1, D).cpu(), want_hs[l].reshape(-1, D).cpu())
        worst = max(worst, e)
        print(f"DETR_DROPIN hs[{l}]: rel L2 {e:.2e}, worst row {r:.2e}")
    print(f"DETR_DROPIN memory: rel L2 {e_m:.2e}, worst row {r_m:.2e}")
    assert e_m < TOL and worst < TOL
