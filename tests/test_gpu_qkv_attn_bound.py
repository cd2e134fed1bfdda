"""The four fused in_proj + attention kernels (hoigen_amd/csrc/hg_qkv_attn.hip, hg_qkv_attn_text.hip) against the chained per-element
bound of tests/qkv_attn_bound.py, through hg_test_qkv_attn_ex: every element within B_A of the float64 attention of the q | k | v that
was consumed - known a priori on the `sel_*` families (the only judge for heads = 6), returned by the folded GEMM alone and held to
B_P on the dense ones, where the fused kernel must also equal the two launches bit for bit.  Every length of both kernels; more than one
round of work items on hard inputs; the row strides a tower call sets; non-finite neighbours and non-finite pad rows at every tile fill;
the hook's refusals.  Each line QKV_ATTN_RATIO <instance> <family> <worst |err| / B_A> is asserted <= 1.
"""
import ctypes as C

import pytest
import torch

import attention_bound as ab
import qkv_attn_bound as qb
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = 203.25                # the fp16 pattern 0x5A5A the hook fills the output buffer with
CANARY = -77.0                   # what the caller's buffers hold before a call
VISION_L = tuple(range(193, 209))
TEXT12_L = (1, 2, 16, 31, 32, 33, 40, 53, 54, 64, 77, 80)


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def text_seqs(L):
    """two full packs and a pack of one"""
    return 2 * (160 // L) + 1


def call(ctx, c, fused, a=None, lda=0, ldo=0, pad_fill=0, qkv_out=False):
    """One hg_test_qkv_attn_ex call on case c (fused: bit 0 only; the K and mask bits follow from the case) -> (rc, out [M, ldo or D],
    qkv_out [M, 3D] or None), on the device; the caller's buffers hold CANARY before the call."""
    D, K, M = c["D"], c["K"], c["M"]
    ops = [(a if a is not None else c["a"]).cuda().contiguous()] + [c[k].cuda().contiguous() for k in ("w", "bias", "cs", "mr")]
    out = torch.full((M, ldo or D), CANARY, device="cuda")
    qkv = torch.full((M, 3 * D), CANARY, device="cuda") if qkv_out else None
    args = _lib.hg_test_qkv_attn_ex_args(a=ops[0].data_ptr(), w=ops[1].data_ptr(), bias=ops[2].data_ptr(), cs=ops[3].data_ptr(),
                                         mr=ops[4].data_ptr(), out=out.data_ptr(), qkv_out=qkv.data_ptr() if qkv_out else None,
                                         n_seq=c["n_seq"], L=c["L"], heads=c["heads"],
                                         fused=int(fused) | (2 if K > D else 0) | (4 if c["causal"] else 0), lda=lda, ldo=ldo,
                                         pad_fill=pad_fill)
    rc = _lib.lib().hg_test_qkv_attn_ex(ctx, C.byref(args), None)
    torch.cuda.synchronize()
    return rc, out, qkv


def run(ctx, c, fused, **kw):
    rc, out, qkv = call(ctx, c, fused, **kw)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    return (out, qkv) if kw.get("qkv_out") else out


def judge_select(ctx, c):
    """a sel_* case through the fused kernel: worst |err| / B_A against the a-priori qkv16; where the two launches exist, their bits"""
    got = run(ctx, c, 1)
    if c["heads"] * 192 % 256 == 0:
        two, qkv16 = run(ctx, c, 0, qkv_out=True)
        assert torch.equal(qkv16.cpu(), c["qkv16"]), "the folded GEMM on exact operands"
        assert torch.equal(got, two), (c["family"], c["L"])
    return ab.worst(got, qb.reference(c, c["qkv16"]))


def judge_dense(ctx, c):
    """a dense case through the chain: (stage P ratio of the GEMM's qkv16, stage A ratio of the fused kernel)"""
    two, qkv16 = run(ctx, c, 0, qkv_out=True)
    p = qb.stage_p_ratio(qkv16, c)
    got = run(ctx, c, 1)
    assert torch.equal(got, two), (c["family"], c["L"])
    return p, ab.worst(got, qb.reference(c, qkv16.cpu()))


def sweep(ctx, family, shapes):
    """every (n_seq, L, heads, extra, causal) of one kernel instance: prints the worst ratios, returns the failures"""
    top, top_p, bad = 0.0, 0.0, []
    for n_seq, L, heads, extra, causal in shapes:
        c = qb.make_case(family, n_seq, L, heads, extra, causal)
        if family in qb.SELECT:
            p, w = 0.0, judge_select(ctx, c)
        else:
            p, w = judge_dense(ctx, c)
        top, top_p = max(top, w), max(top_p, p)
        if not (w <= 1.0 and p <= 1.0):
            bad.append((L, p, w))
    n_seq, L, heads, extra, causal = shapes[0]
    inst = qb.instance(heads, heads * 64 + extra, causal)
    if family in qb.DENSE:
        print(f"QKV_ATTN_RATIO {inst}-P heads {heads} {family} {top_p:.3f}")
    print(f"QKV_ATTN_RATIO {inst} heads {heads} {family} {top:.3f}")
    return bad


# ---- every length, exact projection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", qb.SELECT)
@pytest.mark.parametrize("heads,extra", [(6, 0), (6, 64), (12, 0), (12, 64)])
def test_vision_kernels_at_every_length_within_the_bound(ctx, heads, extra, family):
    """qkv_attn_kernel (K = D) and qkv_attn_kernel_k1 (K = D + 64) at every L = 193 .. 208: 208 - L foreign rows in the tile"""
    assert not sweep(ctx, family, [(3, L, heads, extra, False) for L in VISION_L])


@pytest.mark.parametrize("family", qb.SELECT)
def test_text_k2_kernel_at_every_length_within_the_bound(ctx, family):
    """qkv_attn_kernel_text_k2 (heads = 8) at every L = 1 .. 80: every pack size, every position of a boundary in a 32-query tile"""
    assert not sweep(ctx, family, [(text_seqs(L), L, 8, 0, True) for L in range(1, 81)])


@pytest.mark.parametrize("family", qb.SELECT)
def test_text_kernel_within_the_bound(ctx, family):
    """qkv_attn_kernel_text (heads = 12)"""
    assert not sweep(ctx, family, [(text_seqs(L), L, 12, 0, True) for L in TEXT12_L])


# ---- dense operands through the chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", qb.DENSE)
@pytest.mark.parametrize("extra", [0, 64])
def test_vision_kernels_on_dense_operands_through_the_chain(ctx, extra, family):
    assert not sweep(ctx, family, [(3, L, 12, extra, False) for L in (193, 197, 200, 208)])


@pytest.mark.parametrize("family", qb.DENSE)
@pytest.mark.parametrize("heads", [8, 12])
def test_text_kernels_on_dense_operands_through_the_chain(ctx, heads, family):
    assert not sweep(ctx, family, [(text_seqs(L), L, heads, 0, True) for L in (1, 13, 16, 54, 77, 80)])


# ---- more than one round of work items ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sel_ramp", "lnfold"])
@pytest.mark.parametrize("n_seq,L,heads,causal", [(44, 197, 12, False), (130, 77, 8, True)])
def test_more_than_one_round_of_items_on_hard_inputs(ctx, n_seq, L, heads, causal, family):
    """264 (sequence, head pair) items and 260 (pack, head pair) items on 256 compute units: the next item's prefetch behind the K loop,
    XCD-wise dealing with a short last round"""
    assert not sweep(ctx, family, [(n_seq, L, heads, 0, causal)])


# ---- the row strides of a tower call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sel_ramp", "lnfold"])
@pytest.mark.parametrize("n_seq,L,heads,extra,causal", [(3, 197, 12, 0, False), (3, 197, 12, 64, False), (5, 77, 8, 0, True)])
def test_row_strides_change_no_bit_and_no_pad_column_is_written(ctx, n_seq, L, heads, extra, causal, family):
    """lda = K + 64 (with finite and with NaN columns behind K), ldo = D + 64, and both: the dense call's bits in columns < D, 203.25
    behind them"""
    c = qb.make_case(family, n_seq, L, heads, extra, causal)
    D, K = c["D"], c["K"]
    dense = run(ctx, c, 1)
    for lda, ldo, pad_fill in ((K + 64, 0, 0), (K + 64, 0, 1), (0, D + 64, 0), (K + 64, D + 64, 0), (K + 64, D + 64, 1)):
        out = run(ctx, c, 1, lda=lda, ldo=ldo, pad_fill=pad_fill)
        assert torch.equal(out[:, :D], dense), (lda, ldo, pad_fill)
        assert bool((out[:, D:] == SENTINEL).all()), (lda, ldo, pad_fill)


# ---- non-finite neighbours and pad rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
@pytest.mark.parametrize("heads,extra", [(6, 0), (6, 64), (12, 0), (12, 64)])
def test_vision_non_finite_sequence_does_not_reach_its_neighbours(ctx, heads, extra, poison):
    """The odd sequence of three non-finite, at every L: sequence 0 has 208 - L of its rows in its tile; the even sequences come out
    finite and with the bits of the clean run, the odd one does not come out finite."""
    for L in VISION_L:
        c = qb.make_case("sel_randn", 3, L, heads, extra, False)
        clean = run(ctx, c, 1).view(3, L, -1)
        out = run(ctx, c, 1, a=qb.poisoned(c, poison)["a"]).view(3, L, -1)
        assert not torch.isfinite(out[1::2]).all(dim=(1, 2)).any(), f"L {L}: the poisoned sequence came out finite"
        assert bool(torch.isfinite(out[0::2]).all()), f"L {L}: a clean sequence is poisoned"
        assert torch.equal(out[0::2], clean[0::2]), L


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_text_non_finite_sequence_does_not_reach_its_pack_neighbours_at_any_length(ctx, poison):
    """(tests/test_gpu_qkv_attn_text.py has L = 16 and 77) every L = 1 .. 80, heads 8: every pack size and boundary position"""
    for L in range(1, 81):
        n_seq = text_seqs(L)
        c = qb.make_case("sel_randn", n_seq, L, 8, 0, True)
        clean = run(ctx, c, 1).view(n_seq, L, -1)
        out = run(ctx, c, 1, a=qb.poisoned(c, poison)["a"]).view(n_seq, L, -1)
        assert not torch.isfinite(out[1::2]).all(dim=(1, 2)).any(), f"L {L}: a poisoned sequence came out finite"
        assert bool(torch.isfinite(out[0::2]).all()), f"L {L}: a clean sequence is poisoned"
        assert torch.equal(out[0::2], clean[0::2]), L


@pytest.mark.parametrize("heads,extra", [(6, 0), (6, 64), (12, 0), (12, 64)])
def test_vision_non_finite_pad_rows_change_no_bit(ctx, heads, extra):
    """three sequences: the last one's tile reaches up to 15 rows behind the operand's last row"""
    for L in VISION_L:
        c = qb.make_case("sel_randn", 3, L, heads, extra, False)
        assert torch.equal(run(ctx, c, 1, pad_fill=1), run(ctx, c, 1)), L


@pytest.mark.parametrize("heads", [8, 12])
def test_text_non_finite_pad_rows_change_no_bit(ctx, heads):
    """a last pack of one sequence: the rest of its 160-row tile is pad"""
    for L in (1, 13, 77, 80):
        c = qb.make_case("sel_randn", text_seqs(L), L, heads, 0, True)
        assert torch.equal(run(ctx, c, 1, pad_fill=1), run(ctx, c, 1)), L


# ---- the hook ---------------------------------------------------------------------------------------------------------------------
def test_hook_refusals_write_nothing(ctx):
    c = qb.make_case("sel_randn", 3, 197, 12, 0, False)
    D, K = c["D"], c["K"]
    for kw in (dict(lda=K - 8), dict(lda=K + 4), dict(ldo=D + 4), dict(pad_fill=2), dict(qkv_out=True)):
        rc, out, qkv = call(ctx, c, 1, **kw)
        assert rc == -1, kw                                           # HG_ERR_INVALID
        assert bool((out == CANARY).all()) and (qkv is None or bool((qkv == CANARY).all())), kw
    rc, out, _ = call(ctx, qb.make_case("sel_randn", 3, 81, 8, 0, True), 1)      # what the launchers refuse: L > 80
    assert rc == -1 and bool((out == CANARY).all())
    args = _lib.hg_test_qkv_attn_ex_args()
    assert _lib.lib().hg_test_qkv_attn_ex(ctx, C.byref(args), None) == -1
    # the dense call of the earlier hook is this one with every new argument zero
    ops = [c[k].cuda().contiguous() for k in ("a", "w", "bias", "cs", "mr")]
    old = torch.empty(c["M"], D, device="cuda")
    assert _lib.lib().hg_test_qkv_attn(ctx, *(t.data_ptr() for t in ops), 3, 197, 12, 1, old.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(old, run(ctx, c, 1))
