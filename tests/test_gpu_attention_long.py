"""Attention for sequences of 225 .. 640 tokens (hg_attn_long.hip: the 577 tokens of ViT-L/14@336px) through hg_test_attention,
against an exact float64 softmax(QK^T/8)V of the fp16-rounded inputs on the CPU and the per-element rounding bound B of
tests/attention_bound.py - the reference, the bound and the six input families of tests/test_gpu_attention.py - plus: two launches
agree bit for bit, the one-row form is the full kernel's row, the maximum + 1 is refused, and a non-finite sequence stays in its own
rows."""
import pytest
import torch

import attention_bound as ab
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
    """(the name is from when the reference was fp32 PyTorch on the device: it is float64 on the CPU now, the bound per element, and
    the earlier 2e-3 x max|want| on top of it)"""
    g = torch.Generator(device="cuda").manual_seed(L * 131 + heads)
    qkv = torch.randn(n_seq * L, 3 * heads * 64, device="cuda", generator=g) * 1.5
    got = run_full(ctx, qkv, n_seq, L, heads, causal)
    ref = ab.reference(qkv, n_seq, L, heads, causal)
    w = ab.worst(got, ref)
    err, top = (got.cpu().double() - ref["want"]).abs().max().item(), ref["want"].abs().max().item()
    print(f"ATTN_RATIO long      randn1.5 causal {int(causal)} n_seq {n_seq} heads {heads} L {L}: worst |err| / B {w:.3f}; "
          f"max|d| {err:.3e} = {err / top:.3e} of max|want| {top:.3f}")
    assert w <= 1.0, f"worst |err| / B {w:.3f}"
    assert err <= 2e-3 * top
    assert torch.equal(got, run_full(ctx, qkv, n_seq, L, heads, causal)), "deterministic"


# the first length, around every multiple of 16 and 32 a tile boundary falls on (half a key tile staged, one key short of a tile, a
# full tile, one key into the next), 17 and more query tiles (a wave's second round), the maximum and the length below it
SWEEP_L = (225, 240, 241, 256, 257, 272, 273, 522, 543, 544, 577, 609, 639, 640)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("family", ab.FAMILIES)
def test_long_lengths_within_the_bound(ctx, family, causal):
    """each output element within B, a second launch bit-identical, `onehot` rows exact (attention_bound.sweep)"""
    def run(qkv, n_seq, L, heads, causal):
        return run_full(ctx, qkv.cuda(), n_seq, L, heads, causal).cpu()
    failures = ab.sweep(run, "long", family, causal, SWEEP_L, 2, 2)
    assert not failures, "\n".join(failures)


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


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("family", ["randn", "sink", "ramp"])
def test_one_row_variant_on_hard_inputs(ctx, family, causal):
    """rows 0 (sel = null and sel = 0), L - 1 and a random row of every sequence through the one-row kernel: the full kernel's bits
    (which test_long_lengths_within_the_bound holds to the bound at these lengths)"""
    n_seq, heads = 2, 2
    D = heads * 64
    ar = torch.arange(n_seq, device="cuda")
    for L in (225, 577, MAX_L):
        seed = ab.seed_of(family, L, causal, n_seq, heads)
        qkv = ab.make_qkv(family, n_seq, L, heads, seed).cuda()
        full = run_full(ctx, qkv, n_seq, L, heads, causal).view(n_seq, L, D)
        rand = torch.randint(0, L, (n_seq,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).cuda()
        for sel in (None, torch.zeros_like(rand), torch.full_like(rand, L - 1), rand):
            idx = sel.long() if sel is not None else torch.zeros_like(ar)
            q0 = qkv.view(n_seq, L, 3 * D)[ar, idx, :D].contiguous()
            got = run_rows(ctx, qkv, q0, sel, n_seq, L, heads, causal)
            assert torch.equal(got, full[ar, idx]), (L, None if sel is None else sel.tolist())


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
