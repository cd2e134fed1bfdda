"""Attention for sequences of 225 .. 640 tokens (hg_attn_long.hip: the 577 tokens of ViT-L/14@336px) through hg_test_attention,
against a plain PyTorch fp32 softmax(QK^T/8)V of the fp16-rounded inputs - the reference and the bound of tests/test_gpu_attention.py
(2e-3 x max|want|: fp16 probabilities and fp16 output) - plus: two launches agree bit for bit, the one-row form is the full
kernel's row, the maximum + 1 is refused, and a non-finite sequence stays in its own rows."""
import pytest
import torch

from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

MAX_L = 640          # include/hoigen_amd.h: hg_test_attention; hg_kernels.h ATTN_LONG_MAX_L
HG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def ref_attention(qkv, n_seq, L, heads, causal):
    D = heads * 64
    x = qkv.half().float().view(n_seq, L, 3, heads, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [n, h, L, 64]
    s = q @ k.transpose(-1, -2) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf"), device=s.device).triu(1)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(n_seq * L, D)


def run_full(ctx, qkv, n_seq, L, heads, causal):
    out = torch.empty(n_seq * L, heads * 64, device="cuda")
    rc = _lib.lib().hg_test_attention(ctx, qkv.data_ptr(), None, None, n_seq, L, heads, int(causal), out.data_ptr(), None)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    torch.cuda.synchronize()
    return out


def run_rows(ctx, qkv, q0, sel, n_seq, L, heads, causal):
    out = torch.empty(n_seq, heads * 64, device="cuda")
    rc = _lib.lib().hg_test_attention(ctx, qkv.data_ptr(), q0.data_ptr(), sel.data_ptr() if sel is not None else None,
                                      n_seq, L, heads, int(causal), out.data_ptr(), None)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    torch.cuda.synchronize()
    return out


CASES = [
    (3, 577, 16, False),        # ViT-L/14@336px
    (40, 577, 16, False),       # 640 items: more than one round of 256 CUs
    (5, 257, 16, False),        # ViT-L/14 at 224 px (two workgroups per CU)
    (4, 225, 4, False),         # first length of this path
    (2, MAX_L, 3, False),       # the stated maximum: K and V fill the LDS
    (2, MAX_L, 2, True),
    (3, 522, 5, False),         # L % 32 = 10: half a key tile, 16 staged rows of which 10 are real
    (3, 543, 5, False),         # L % 32 = 31: the last tile's second half is present, one key short
    (3, 544, 5, False),         # L % 32 = 0: the last tile is full
    (1, 577, 1, False),         # one head, one sequence: a single workgroup
    (3, 577, 16, True),         # causal
    (4, 301, 6, True),          # causal, L % 32 = 13
]


@pytest.mark.parametrize("n_seq,L,heads,causal", CASES)
def test_long_attention_vs_fp32_reference(ctx, n_seq, L, heads, causal):
    g = torch.Generator(device="cuda").manual_seed(L * 131 + heads)
    qkv = torch.randn(n_seq * L, 3 * heads * 64, device="cuda", generator=g) * 1.5
    want = ref_attention(qkv, n_seq, L, heads, causal)
    got = run_full(ctx, qkv, n_seq, L, heads, causal)
    err, top = (got - want).abs().max().item(), want.abs().max().item()
    print(f"n_seq {n_seq} L {L} heads {heads} causal {causal}: max|d| {err:.3e} = {err / top:.3e} of max|want| {top:.3f}")
    assert err <= 2e-3 * top
    assert torch.equal(got, run_full(ctx, qkv, n_seq, L, heads, causal)), "deterministic"


def test_above_the_maximum_is_refused(ctx):
    L, heads = MAX_L + 1, 2
    qkv = torch.zeros(L, 3 * heads * 64, device="cuda")
    out = torch.empty(L, heads * 64, device="cuda")
    lib = _lib.lib()
    assert lib.hg_test_attention(ctx, qkv.data_ptr(), None, None, 1, L, heads, 0, out.data_ptr(), None) == HG_ERR_INVALID
    assert lib.hg_test_attention(ctx, qkv.data_ptr(), None, None, 1, L, heads, 1, out.data_ptr(), None) == HG_ERR_INVALID
    q0 = torch.zeros(1, heads * 64, device="cuda")
    assert lib.hg_test_attention(ctx, qkv.data_ptr(), q0.data_ptr(), None, 1, L, heads, 0, out.data_ptr(), None) == HG_ERR_INVALID


@pytest.mark.parametrize("n_seq,L,heads,causal", [(5, 577, 16, False), (6, 257, 16, False), (3, 577, 4, True), (2, MAX_L, 2, False)])
def test_one_row_variant_is_the_full_kernels_row(ctx, n_seq, L, heads, causal):
    D = heads * 64
    g = torch.Generator(device="cuda").manual_seed(L * 17 + heads)
    qkv = torch.randn(n_seq * L, 3 * D, device="cuda", generator=g)
    full = run_full(ctx, qkv, n_seq, L, heads, causal).view(n_seq, L, D)
    for sel in (None, torch.randint(0, L, (n_seq,), device="cuda", generator=g, dtype=torch.int32),
                torch.full((n_seq,), L - 1, device="cuda", dtype=torch.int32)):
        idx = sel.long() if sel is not None else torch.zeros(n_seq, dtype=torch.long, device="cuda")
        q0 = qkv.view(n_seq, L, 3 * D)[torch.arange(n_seq, device="cuda"), idx, :D].contiguous()
        rows = run_rows(ctx, qkv, q0, sel, n_seq, L, heads, causal)
        assert torch.equal(rows, full[torch.arange(n_seq, device="cuda"), idx]), "same instruction sequence, same bits"


@pytest.mark.parametrize("L", [577, 522])
def test_a_non_finite_sequence_stays_in_its_own_rows(ctx, L):
    """K rows of ONE sequence hold Inf (its last row too: the row the pad rows of the last key tile repeat): its own rows come out
    non-finite, every other sequence's rows are bit for bit what they are without it."""
    n_seq, heads = 4, 16
    D = heads * 64
    g = torch.Generator(device="cuda").manual_seed(L)
    qkv = torch.randn(n_seq * L, 3 * D, device="cuda", generator=g)
    clean = run_full(ctx, qkv, n_seq, L, heads, False).view(n_seq, L, D)
    bad = qkv.clone().view(n_seq, L, 3 * D)
    bad[1, 5, D:2 * D] = float("inf")
    bad[1, L - 1, D:3 * D] = float("inf")
    got = run_full(ctx, bad.view(n_seq * L, 3 * D), n_seq, L, heads, False).view(n_seq, L, D)
    assert not torch.isfinite(got[1]).all()
    for s in (0, 2, 3):
        assert torch.equal(got[s], clean[s]), s
    q0 = bad[:, 0, :D].contiguous()
    rows = run_rows(ctx, bad.view(n_seq * L, 3 * D), q0, None, n_seq, L, heads, False)
    for s in (0, 2, 3):
        assert torch.equal(rows[s], clean[s, 0]), s
