"""The DETR encoder and decoder runners (hoigen_amd/csrc/hg_detr.hip, hg_detr_dec.hip), launch by launch.  Every kernel the runners
launch is held to a float64 bound alone (test_gpu_gemm*.py, test_gpu_detr_attention.py, test_gpu_detr_ffn.py, test_gpu_detr_rows.py);
what the runners add is the choice of which buffer, weight pointer, bias offset, leading dimension and layer offset goes into which
launch.  Here that sequence is rebuilt in Python out of the test hooks alone - one hook call for each launch the runner's source shows,
in its order -

    hg_test_detr_rows           entry, dec_entry, postnorm, dec_tail, exit
    hg_test_gemm_ex, kernel 0   the dispatcher (the launch_gemm the runners call), epilogues 0 (bias -> fp16), 2 (bias + ReLU -> fp16) and
                                3 (bias + residual, fp32 in place), operands and leading dimensions as the runner passes them
    hg_test_detr_attention      layout 0 (q | k of one buffer, v of its own) for the self-attentions, 1 for the cross-attention
    hg_test_detr_ffn            the split kernel's partial sums, fed to the tail (op 4) with b2 - or the two GEMMs and the tail without

and `forward_trace`'s trace after every layer, the encoder's output and the decoder's hs must be torch.equal to it.  A wrong in_proj row
block, `b_in + 2 * D`, `kall + l * D`, a K / V matrix of the wrong layer, norm2's weights in norm1's place, a stale xp16 or a trace
written one layer off changes bits.

One step differs between hook and runner by construction: the cross-attention reads K and V from the stacked [B * S, n_layers * D]
buffers (row stride n_layers * D) in the runner and from dense copies of this layer's columns (row stride D) in the hook.  The kernel
copies the rows it needs into the LDS and its arithmetic does not see the row stride, so the bits are equal and are REQUIRED to be: no
step is held to a bound in place of equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import detr_decoder_cases as dd
import detr_encoder_cases as ec
from hoigen_amd import _lib
from hoigen_amd.detr import TransformerDecoder, TransformerEncoder

pytestmark = pytest.mark.gpu

ENTRY, POSTNORM, EXIT, DEC_ENTRY, DEC_TAIL = range(5)
EPI_F16, EPI_RELU_F16, EPI_RESID = 0, 2, 3
GH, GW = 5, 7


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Hooks:
    """one native context of its own; every method is one launch"""

    def __init__(self):
        self.lib = _lib.lib()
        self.h = self.lib.hg_create(0)
        assert self.h

    def close(self):
        self.lib.hg_destroy(self.h)

    def ok(self, rc):
        assert rc == 0, self.lib.hg_last_error(self.h)

    def rows(self, op, ptrs, strides=(), ints=()):
        a = _lib.hg_test_detr_rows_args()
        for k, t in enumerate(ptrs):
            a.p[k] = None if t is None else t.data_ptr()
        for k, v in enumerate(strides):
            a.s[k] = v
        for k, v in enumerate(ints):
            a.i[k] = v
        self.ok(self.lib.hg_test_detr_rows(self.h, op, C.byref(a), None))

    def gemm(self, a, w, bias, epi, out=None):
        """a [M, K] (fp16 values; fp16 or fp32 tensor), w [N, K], bias [N]; epi 3 adds into `out` [M, N] in place"""
        a, w = a.float().contiguous(), w.contiguous()
        (M, K), N = a.shape, w.shape[0]
        assert w.shape[1] == K and bias.shape == (N,) and bias.is_contiguous()
        if out is None:
            out = torch.full((M, N), float("nan"), device="cuda")
        assert out.shape == (M, N) and out.is_contiguous()
        x = _lib.hg_test_gemm_ex_args()
        x.a, x.w, x.bias, x.out = a.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr()
        x.M, x.N, x.K, x.lda, x.ldc, x.epi, x.kernel = M, N, K, K, N, epi, 0
        self.ok(self.lib.hg_test_gemm_ex(self.h, C.byref(x), None))
        return out

    def attention(self, q, k, v, mask, B, Lq, Lk, heads, layout):
        D = heads * 32
        q, k, v = (t.float().contiguous() for t in (q, k, v))
        out = torch.full((B * Lq + 8, D), float("nan"), device="cuda")
        self.ok(self.lib.hg_test_detr_attention(self.h, q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr() if mask is not None else None,
                                                B, Lq, Lk, heads, -1, layout, 0, out.data_ptr(), None))
        return out[:B * Lq]

    def ffn_partials(self, x, w1, b1, w2, b2, g, b, F):
        M, D = x.shape
        assert self.lib.hg_set_option(self.h, b"detr_ffn", 2) == 0
        y = torch.empty(M, D, device="cuda")
        part = torch.full((F // 128, M, D), float("nan"), device="cuda")
        self.ok(self.lib.hg_test_detr_ffn(self.h, x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), g.data_ptr(), b.data_ptr(),
                                          M, D, F, y.data_ptr(), part.data_ptr(), None))
        return part


@pytest.fixture(scope="module")
def hooks():
    h = Hooks()
    yield h
    h.close()


def row_buffers(M, D):
    f = lambda dt: torch.full((M, D), float("nan"), dtype=dt, device="cuda")
    return f(torch.float32), f(torch.float16), f(torch.float16), f(torch.float32)      # x, x16, xp16, posb


def encoder_by_hooks(hk, sd, cfg, src, pos, mask):
    """hg_detr_encoder's launches (hg_detr.hip), in order -> (out [S, B, D], trace [layers, B * S, D])"""
    D, F, H, NL = cfg["d_model"], cfg["d_ff"], cfg["heads"], cfg["layers"]
    S, B, _ = src.shape
    M = B * S
    x, x16, xp16, posb = row_buffers(M, D)
    trace = torch.full((NL, M, D), float("nan"), device="cuda")
    st = (src.stride(1), src.stride(0))
    hk.rows(ENTRY, [src, pos, x, x16, xp16, posb], (*st, *((pos.stride(1), pos.stride(0)) if pos is not None else (0, 0))), (B, S, D))
    for l in range(NL):
        g = lambda key: sd[f"layers.{l}.{key}"]
        w_in, b_in = g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias")
        qk = hk.gemm(xp16, w_in[:2 * D], b_in[:2 * D], EPI_F16)
        v = hk.gemm(x16, w_in[2 * D:], b_in[2 * D:], EPI_F16)
        att = hk.attention(qk[:, :D], qk[:, D:], v, mask, B, S, S, H, 0)
        hk.gemm(att, g("self_attn.out_proj.weight"), g("self_attn.out_proj.bias"), EPI_RESID, out=x)
        hk.rows(POSTNORM, [x, g("norm1.weight"), g("norm1.bias"), None, x16, None, None], (), (M, D))
        ff = hk.gemm(x16, g("linear1.weight"), g("linear1.bias"), EPI_RELU_F16)
        hk.gemm(ff, g("linear2.weight"), g("linear2.bias"), EPI_RESID, out=x)
        hk.rows(POSTNORM, [x, g("norm2.weight"), g("norm2.bias"), posb, x16, xp16 if l + 1 < NL else None, trace[l]], (), (M, D))
    out = torch.full((S, B, D), float("nan"), device="cuda")
    hk.rows(EXIT, [x, out], (out.stride(1), out.stride(0)), (B, S, D))
    return out, trace


def decoder_by_hooks(hk, sd, cfg, memory, pos, mask, query_pos, split):
    """hg_detr_decoder's launches (hg_detr_dec.hip), in order -> (hs [layers, Q, B, D], trace [layers, B * Q, D])"""
    D, F, H, NL = cfg["d_model"], cfg["d_ff"], cfg["heads"], cfg["layers"]
    S, B, _ = memory.shape
    Q = query_pos.shape[0]
    Ms, Mq = B * S, B * Q
    mx, m16, mp16, mpos = row_buffers(Ms, D)
    hk.rows(ENTRY, [memory, pos, mx, m16, mp16, mpos],
            (memory.stride(1), memory.stride(0), *((pos.stride(1), pos.stride(0)) if pos is not None else (0, 0))), (B, S, D))
    # the k and v rows of every layer's multihead_attn.in_proj, stacked as the loader stacks them: [n_layers * D, D]
    cw = [sd[f"layers.{l}.multihead_attn.in_proj_weight"] for l in range(NL)]
    cb = [sd[f"layers.{l}.multihead_attn.in_proj_bias"] for l in range(NL)]
    kall = hk.gemm(mp16, torch.cat([w[D:2 * D] for w in cw]), torch.cat([b[D:2 * D] for b in cb]), EPI_F16)
    vall = hk.gemm(m16, torch.cat([w[2 * D:] for w in cw]), torch.cat([b[2 * D:] for b in cb]), EPI_F16)
    x, x16, xp16, qposb = row_buffers(Mq, D)
    hk.rows(DEC_ENTRY, [None, query_pos, x, x16, xp16, qposb], (0, 0, 0, query_pos.stride(0)), (B, Q, D))
    trace = torch.full((NL, Mq, D), float("nan"), device="cuda")
    hs = torch.full((NL, Q, B, D), float("nan"), device="cuda")
    nw, nb = sd["norm.weight"], sd["norm.bias"]
    for l in range(NL):
        g = lambda key: sd[f"layers.{l}.{key}"]
        w_in, b_in = g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias")
        qk = hk.gemm(xp16, w_in[:2 * D], b_in[:2 * D], EPI_F16)
        v = hk.gemm(x16, w_in[2 * D:], b_in[2 * D:], EPI_F16)
        att = hk.attention(qk[:, :D], qk[:, D:], v, None, B, Q, Q, H, 0)
        hk.gemm(att, g("self_attn.out_proj.weight"), g("self_attn.out_proj.bias"), EPI_RESID, out=x)
        hk.rows(POSTNORM, [x, g("norm1.weight"), g("norm1.bias"), qposb, x16, xp16, None], (), (Mq, D))
        q = hk.gemm(xp16, cw[l][:D], cb[l][:D], EPI_F16)
        att = hk.attention(q, kall[:, l * D:(l + 1) * D], vall[:, l * D:(l + 1) * D], mask, B, Q, S, H, 1)
        hk.gemm(att, g("multihead_attn.out_proj.weight"), g("multihead_attn.out_proj.bias"), EPI_RESID, out=x)
        hk.rows(POSTNORM, [x, g("norm2.weight"), g("norm2.bias"), None, x16, None, None], (), (Mq, D))
        w1, b1, w2, b2 = g("linear1.weight"), g("linear1.bias"), g("linear2.weight"), g("linear2.bias")
        if split:
            part = hk.ffn_partials(x, w1, b1, w2, b2, g("norm3.weight"), g("norm3.bias"), F)
            tail_b2, n_sl = b2, F // 128
        else:
            ff = hk.gemm(x16, w1, b1, EPI_RELU_F16)
            hk.gemm(ff, w2, b2, EPI_RESID, out=x)
            part, tail_b2, n_sl = None, None, 0
        hk.rows(DEC_TAIL, [x, tail_b2, part, g("norm3.weight"), g("norm3.bias"), qposb, x16, xp16 if l + 1 < NL else None, trace[l], nw, nb, hs[l]],
                (hs.stride(2), hs.stride(1)), (n_sl, Q, Mq, D))
    return hs, trace


def on_device(sd):
    return {k: dev(v) for k, v in sd.items()}


@pytest.mark.parametrize("B", (1, 3))
def test_the_encoder_is_its_launches(hooks, B):
    cfg = ec.SMALL
    sd = ec.weights(cfg, 3)
    m = TransformerEncoder(cfg["d_model"], cfg["heads"], cfg["layers"], cfg["d_ff"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    dsd = on_device(sd)
    for kind in ("rect", "perimage"):
        for with_pos in (True, False):
            src, pos = (dev(a) for a in ec.inputs(B, GH, GW, cfg["d_model"], 70 + B))
            pos = pos if with_pos else None
            mask = dev(ec.mask_of(kind, B, GH, GW))
            out, trace = m.forward_trace(src, src_key_padding_mask=mask, pos=pos)
            want_out, want_trace = encoder_by_hooks(hooks, dsd, cfg, src, pos, mask)
            torch.cuda.synchronize()
            assert torch.isfinite(trace).all() and torch.isfinite(want_trace).all()
            for l in range(cfg["layers"]):
                assert torch.equal(trace[l], want_trace[l]), f"B {B} {kind} pos {with_pos}: the stream after layer {l} is not its launches'"
            assert torch.equal(out, want_out), f"B {B} {kind} pos {with_pos}: out"


@pytest.mark.parametrize("option", (2, 1), ids=("split", "gemms"))
@pytest.mark.parametrize("B", (1, 3))
def test_the_decoder_is_its_launches(hooks, B, option):
    cfg = dd.SMALL
    sd = dd.weights(cfg, 4)
    m = TransformerDecoder(cfg["d_model"], cfg["heads"], cfg["layers"], cfg["d_ff"], True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    m.set_option("detr_ffn", option)
    dsd = on_device(sd)
    for Q in (1, 33):
        for kind in ("rect", "perimage"):
            for with_pos in (True, False):
                qe, mem, pos = (dev(a) for a in dd.inputs(B, GH, GW, Q, cfg["d_model"], 80 + B + Q))
                pos = pos if with_pos else None
                mask = dev(ec.mask_of(kind, B, GH, GW))
                hs, trace = m.forward_trace(None, mem, memory_key_padding_mask=mask, pos=pos, query_pos=qe)
                want_hs, want_trace = decoder_by_hooks(hooks, dsd, cfg, mem, pos, mask, qe, option == 2)
                torch.cuda.synchronize()
                what = f"B {B} Q {Q} {kind} pos {with_pos} detr_ffn {option}"
                assert torch.isfinite(trace).all() and torch.isfinite(hs).all() and torch.isfinite(want_trace).all()
                for l in range(cfg["layers"]):
                    assert torch.equal(trace[l], want_trace[l]), f"{what}: the stream after layer {l} is not its launches'"
                    assert torch.equal(hs[l], want_hs[l]), f"{what}: hs[{l}]"
