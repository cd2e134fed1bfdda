"""The backward kernels of the text tower (hoigen_amd/csrc/hg_text_grad.hip), each in a single launch through hg_test_text_grad on the
caller's buffers, against the float64 references and per-element bounds of tests/text_grad_bound.py (shown to bite in
tests/test_text_grad_rounding_model.py), and hg_assemble_prompts_backward bit for bit against its float32 restatement."""
import ctypes as C

import pytest
import torch

import text_grad_bound as tg
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 64, 77, 80)


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def hook(ctx, op, ptrs, ints, n=0, ok=True):
    a = _lib.hg_test_elem_args()
    for k, t in enumerate(ptrs):
        a.p[k] = t.data_ptr() if t is not None else None
    for k, v in enumerate(ints):
        a.i[k] = v
    a.n = n
    rc = _lib.lib().hg_test_text_grad(ctx, op, C.byref(a), None)
    torch.cuda.synchronize()
    if ok:
        assert rc == 0, _lib.lib().hg_last_error(ctx)
    return rc


def run_attn_bwd(ctx, qkv, dout, n_seq, L, heads):
    """-> dqkv [n_seq * L, 3 D] float32 (from the kernel's fp16) and the two NaN canary rows behind it"""
    M, D = n_seq * L, heads * 64
    out = torch.full((M + 2, 3 * D), float("nan"), device="cuda", dtype=torch.float16)
    hook(ctx, 0, (qkv.cuda().half(), dout.cuda().half(), out), (n_seq, L, heads))
    return out[:M].float().cpu(), out[M:].cpu()


@pytest.mark.parametrize("heads", (2, 8))
@pytest.mark.parametrize("family", tg.ATTN_FAMILIES)
def test_attention_backward_within_bound(ctx, family, heads):
    top, fails = 0.0, []
    for n_seq in (1, 3):
        for L in LENGTHS:
            qkv, dout = tg.make_attn(family, n_seq, L, heads, 3000 + 16 * L + n_seq)
            ref = tg.attn_reference(qkv, dout, n_seq, L, heads)
            got, canary = run_attn_bwd(ctx, qkv, dout, n_seq, L, heads)
            w = tg.worst(got, ref)
            top = max(top, w)
            if not w <= 1.0:
                fails.append(f"n_seq {n_seq} L {L}: worst |err| / B {w:.3f}")
            if not bool(torch.isnan(canary).all()):
                fails.append(f"n_seq {n_seq} L {L}: rows behind the output were written")
            if L == 1:
                D = heads * 64
                if not (torch.equal(got[:, 2 * D:], dout) and not got[:, :2 * D].any()):
                    fails.append(f"n_seq {n_seq} L 1: dV != dO or dQ, dK != 0")
    wm = tg.worst(tg.attn_model(qkv, dout, n_seq, L, heads), ref)
    print(f"TEXT_GRAD_RATIO attn_bwd {family} heads {heads}: worst |err| / B {top:.3f} (restatement at the last case {wm:.3f})")
    assert not fails, "; ".join(fails)


def test_attention_backward_does_not_depend_on_the_batch(ctx):
    qkv, dout = tg.make_attn("randn", 5, 33, 2, 77)
    full, _ = run_attn_bwd(ctx, qkv, dout, 5, 33, 2)
    again, _ = run_attn_bwd(ctx, qkv, dout, 5, 33, 2)
    assert torch.equal(full, again)
    one, _ = run_attn_bwd(ctx, qkv[2 * 33:3 * 33], dout[2 * 33:3 * 33], 1, 33, 2)
    assert torch.equal(one, full[2 * 33:3 * 33])
    assert hook(ctx, 0, (qkv.cuda().half(), dout.cuda().half(), torch.empty(1, device="cuda")), (1, 81, 2), ok=False) != 0


@pytest.mark.parametrize("D", (128, 512, 768))
@pytest.mark.parametrize("family", ("randn", "offset", "constant"))
def test_layernorm_backward_within_bound(ctx, family, D):
    top = 0.0
    for M in (1, 7, 257):
        x, gamma, dy, g = tg.make_ln(family, M, D, 10 * D + M)
        ref = tg.ln_reference(x, gamma, dy, g)
        gd = g.cuda()
        hook(ctx, 1, (x.cuda(), gamma.cuda(), dy.cuda(), gd, None), (M, D, 0))
        w = tg.worst(gd.cpu(), ref)
        top = max(top, w)
        assert w <= 1.0, f"{family} M {M} D {D}: worst |err| / B {w:.3f}"
    # the row-selected form (ln_final): row r of x / dy updates row r * rows_per_seq + sel[r] of g, every other row stays as it is
    R, rows = 7, 5
    x, gamma, dy, _ = tg.make_ln(family, R, D, 99 + D)
    sel = torch.tensor([0, 4, 2, 1, 3, 4, 0], dtype=torch.int32)
    g0 = torch.randn(R * rows, D, generator=torch.Generator().manual_seed(D))
    gd = g0.cuda()
    hook(ctx, 1, (x.cuda(), gamma.cuda(), dy.cuda(), gd, sel.cuda()), (R, D, rows))
    idx = torch.arange(R) * rows + sel.long()
    ref = tg.ln_reference(x, gamma, dy, g0[idx])
    assert tg.worst(gd.cpu()[idx], ref) <= 1.0
    keep = torch.ones(R * rows, dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(gd.cpu()[keep], g0[keep])
    print(f"TEXT_GRAD_RATIO layernorm_bwd {family} D {D}: worst |err| / B {top:.3f}")


def test_qgelu_backward_within_bound(ctx):
    # the MLP's hidden rows [M, 4 D] for D = 128, 512, 768 and 1, 7, 257 rows (the kernel is elementwise: a flat count), and the smallest call
    for n in [8] + [M * 4 * D for D in (128, 512, 768) for M in (1, 7, 257)]:
        df, u = tg.make_qgelu(n, n)
        out = torch.empty(n, device="cuda", dtype=torch.float16)
        hook(ctx, 2, (df.cuda().half(), u.cuda().half(), out), (), n=n)
        w = tg.worst(out.float().cpu(), tg.qgelu_reference(df, u))
        assert w <= 1.0, f"n {n}: worst |err| / B {w:.3f}"
    assert hook(ctx, 2, (out, out, out), (), n=12, ok=False) != 0


def test_scale_and_unscale_are_exact(ctx):
    go = torch.randn(6, 128, generator=torch.Generator().manual_seed(1)) * torch.tensor([1.0, 1e-6, 3e4, 0.0, 1e-30, 7.0])[:, None]
    go16 = torch.empty(6, 128, device="cuda", dtype=torch.float16)
    sinv = torch.empty(6, device="cuda")
    hook(ctx, 3, (go.cuda(), go16, sinv), (6, 128))
    s = tg.pow2_scale(go)
    assert torch.equal(sinv.cpu(), 1.0 / s[:, 0])
    assert torch.equal(go16.cpu().float(), tg.f16(go * s))
    big = go16.float().abs().amax(-1).cpu()
    assert all(1.0 <= float(b) <= 2.0 for r, b in enumerate(big) if r != 3) and big[3] == 0
    g = torch.randn(6 * 3, 128, generator=torch.Generator().manual_seed(2))
    out = torch.full((6, 5, 128), float("nan"), device="cuda")
    hook(ctx, 4, (g.cuda(), sinv, out), (6, 5, 3, 128))
    want = torch.zeros(6, 5, 128)
    want[:, :3] = g.view(6, 3, 128) * (1.0 / s)[:, :, None]
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("R", (1, 256, 257))
def test_assemble_prompts_backward_bit_for_bit(ctx, R):
    L, n_ctx, D = 12, 5, 128
    g = torch.randn(R, L, D, generator=torch.Generator().manual_seed(R))
    gd, gc, gb = g.cuda(), torch.empty(n_ctx, D, device="cuda"), torch.empty(R, D, device="cuda")
    rc = _lib.lib().hg_assemble_prompts_backward(ctx, gd.data_ptr(), R, L, n_ctx, D, gc.data_ptr(), gb.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    want_c, want_b = tg.prompts_bwd_model(g, n_ctx, _lib.HG_PROMPTS_BWD_CHUNK)
    assert torch.equal(gc.cpu(), want_c) and torch.equal(gb.cpu(), want_b)
    gc2 = torch.empty_like(gc)
    assert _lib.lib().hg_assemble_prompts_backward(ctx, gd.data_ptr(), R, L, n_ctx, D, gc2.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(gc2, gc)
