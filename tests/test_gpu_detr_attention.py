"""The DETR attention kernel (hoigen_amd/csrc/hg_detr_attn.hip: head dim 32, Lq != Lk, key padding mask) through
hg_test_detr_attention, against the exact float64 reference and the per-element bound B of tests/detr_attn_bound.py: every output
element inside B over the lengths, masks and input families; the chunked form bit for bit the resident one; a sequence without a
visible key NaN in its own rows only; nothing written outside the output; the refusals."""
import pytest
import torch

import detr_attn_bound as db
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

MAX_L = 1792          # hoigen_amd/csrc/hg_kernels.h DETR_ATTN_MAX_L
HG_ERR_INVALID = -1
CANARY = 203.25       # the fp16 value of the byte 0x5A twice: what the hook fills the kernel's output buffer with

SMALL_L = (1, 2, 31, 32, 33, 63, 64, 65, 97, 221)          # 3 sequences x 2 heads
LARGE_L = (950, 1280, 1281, 1444, 1764, 1792)              # 1 sequence x 2 heads
CROSS = ((1, 97), (33, 221), (100, 950), (100, 1444))      # (Lq, Lk)


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def run(ctx, q, k, v, mask, n_seq, Lq, Lk, heads, chunk=0, layout=None, ldo=0, check=True):
    """-> [n_seq * Lq, heads * 32] on the CPU; the canary rows and columns are checked on the way"""
    D = heads * 32
    ld = ldo or D
    out = torch.full((n_seq * Lq + 8, ld), float("nan"), device="cuda")
    if layout is None:
        layout = 0 if Lq == Lk else 1
    mk = mask.cuda().contiguous() if mask is not None else None
    qd, kd, vd = q.cuda().contiguous(), k.cuda().contiguous(), v.cuda().contiguous()
    rc = _lib.lib().hg_test_detr_attention(ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(),
                                           mk.data_ptr() if mk is not None else None, n_seq, Lq, Lk, heads, chunk, layout, ldo,
                                           out.data_ptr(), None)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    torch.cuda.synchronize()
    out = out.cpu()
    if check:
        assert (out[n_seq * Lq:] == CANARY).all(), "rows behind the output were written"
        assert (out[:, D:] == CANARY).all(), "columns behind heads * 32 were written"
    return out[:n_seq * Lq, :D].contiguous()


def one_case(ctx, family, n_seq, Lq, Lk, heads, mask, ldo=0):
    q, k, v = db.make_qkv(family, n_seq, Lq, Lk, heads, db.seed_of(family, Lq, Lk, mask, n_seq, heads))
    mk = db.make_mask(mask, n_seq, Lk)
    ref = db.reference(q, k, v, mk, n_seq, Lq, Lk, heads)
    got = run(ctx, q, k, v, mk, n_seq, Lq, Lk, heads, ldo=ldo)
    w = db.worst(got, ref)
    fails = []
    if not w <= 1.0:
        r = db.ratio(got, ref)
        fails.append(f"{family} Lq {Lq} Lk {Lk} {mask}: worst |err| / B {w:.3f}, {int((r > 1).sum())} of {r.numel()} elements above B")
    if family == "onehot":
        bad, n = db.onehot_exact_rows(got, v, mk, n_seq, Lq, Lk, heads)
        if bad:
            fails.append(f"{family} Lq {Lq} Lk {Lk} {mask}: {bad} of {n} elements are not fp16(v[j*])")
    return w, fails


@pytest.mark.parametrize("family", db.FAMILIES)
def test_small_lengths_every_mask_within_the_bound(ctx, family):
    top, where, fails = 0.0, None, []
    for L in SMALL_L:
        for mask in db.MASKS:
            w, f = one_case(ctx, family, 3, L, L, 2, mask, ldo=2 * 32 + 8)      # canary columns beside every row, tails and partial tiles included
            fails += f
            if w > top:
                top, where = w, (L, mask)
    print(f"DETR_ATTN_RATIO small {family:8s} n_seq 3 heads 2 L {SMALL_L[0]}..{SMALL_L[-1]} all masks: worst |err| / B {top:.3f} at {where}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("heads", (8, 16))
def test_the_detectors_head_counts_within_the_bound(ctx, heads):
    """8 heads (the detector) and 16 (d_model 512): the (sequence, head) decomposition of the block index, held to the per-element bound"""
    top, where, fails = 0.0, None, []
    for family in ("randn", "ramp"):
        for L in (33, 97):
            w, f = one_case(ctx, family, 2, L, L, heads, "rect", ldo=heads * 32 + 8)
            fails += f
            if w > top:
                top, where = w, (family, L)
    print(f"DETR_ATTN_RATIO heads {heads} n_seq 2 L 33, 97 rect: worst |err| / B {top:.3f} at {where}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", db.FAMILIES)
def test_large_lengths_within_the_bound(ctx, family):
    """the resident form up to 1 280 keys, the chunked form beyond; each length under the rectangle mask and one more"""
    others = ("none", "head64", "midrun", "middle", "last", "first")
    top, where, fails = 0.0, None, []
    for i, L in enumerate(LARGE_L):
        for mask in ("rect", others[i]):
            w, f = one_case(ctx, family, 1, L, L, 2, mask)
            fails += f
            if w > top:
                top, where = w, (L, mask)
    print(f"DETR_ATTN_RATIO large {family:8s} n_seq 1 heads 2 L {LARGE_L[0]}..{LARGE_L[-1]}: worst |err| / B {top:.3f} at {where}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", db.FAMILIES)
def test_query_and_key_lengths_differ(ctx, family):
    top, where, fails = 0.0, None, []
    for Lq, Lk in CROSS:
        n_seq = 3 if Lk <= 221 else 1
        for mask in ("none", "rect", "perseq", "head64"):
            w, f = one_case(ctx, family, n_seq, Lq, Lk, 2, mask)
            fails += f
            if w > top:
                top, where = w, (Lq, Lk, mask)
    print(f"DETR_ATTN_RATIO cross {family:8s} heads 2 (Lq, Lk) {CROSS}: worst |err| / B {top:.3f} at {where}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("Lk", [97, 221])
def test_the_chunked_form_is_the_resident_form_bit_for_bit(ctx, Lk):
    n_seq, heads = 3, 2
    for family, mask in (("randn", "rect"), ("ramp", "perseq"), ("sink", "midrun"), ("ramp", "head64")):
        for Lq in (Lk, 33):
            q, k, v = db.make_qkv(family, n_seq, Lq, Lk, heads, db.seed_of(family, Lq, Lk, mask, n_seq, heads))
            mk = db.make_mask(mask, n_seq, Lk)
            resident = run(ctx, q, k, v, mk, n_seq, Lq, Lk, heads, chunk=0)
            for chunk in (32, 64):
                assert torch.equal(run(ctx, q, k, v, mk, n_seq, Lq, Lk, heads, chunk=chunk), resident), (family, mask, Lq, chunk)


def test_chunk_sizes_and_layouts_agree_at_a_length_that_does_not_fit(ctx):
    """1 444 keys (38 x 38) do not fit the LDS: the default 512-key chunks, 1 280-key and 96-key chunks, and the three operand layouts"""
    n_seq, heads, L = 1, 2, 1444
    q, k, v = db.make_qkv("ramp", n_seq, L, L, heads, 5)
    mk = db.make_mask("rect", n_seq, L)
    base = run(ctx, q, k, v, mk, n_seq, L, L, heads)
    for chunk in (1280, 96):
        assert torch.equal(run(ctx, q, k, v, mk, n_seq, L, L, heads, chunk=chunk), base), chunk
    for layout in (1, 2):
        assert torch.equal(run(ctx, q, k, v, mk, n_seq, L, L, heads, layout=layout), base), layout
    assert torch.equal(run(ctx, q, k, v, mk, n_seq, L, L, heads, ldo=heads * 32 + 24), base), "ldo"


@pytest.mark.parametrize("n_seq,L", [(1, 950), (4, 950), (3, 97), (1, 33)])
def test_every_slab_size_gives_the_same_bits(n_seq, L):
    """option detr_attn_waves: 128-query slabs (the default) and 32-, 64-query slabs, for one image and for a batch"""
    heads, lib = 8, _lib.lib()
    h = lib.hg_create(0)
    try:
        q, k, v = db.make_qkv("randn", n_seq, L, L, heads, L + n_seq)
        mk = db.make_mask("rect", n_seq, L)
        base = run(h, q, k, v, mk, n_seq, L, L, heads)
        assert db.worst(base, db.reference(q, k, v, mk, n_seq, L, L, heads)) <= 1.0
        for waves in (1, 2, 4):
            assert lib.hg_set_option(h, b"detr_attn_waves", waves) == 0
            assert torch.equal(run(h, q, k, v, mk, n_seq, L, L, heads), base), waves
        assert lib.hg_set_option(h, b"detr_attn_waves", 3) == 0
        out = torch.full((n_seq * L + 8, heads * 32), float("nan"), device="cuda")
        z = torch.zeros(n_seq * L, heads * 32, device="cuda")
        assert lib.hg_test_detr_attention(h, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, n_seq, L, L, heads, 0, 0, 0, out.data_ptr(), None) == HG_ERR_INVALID
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    finally:
        lib.hg_destroy(h)


@pytest.mark.parametrize("L,chunk", [(97, 0), (97, 32), (221, 64), (1444, 0)])
def test_a_sequence_without_a_visible_key_is_nan_and_alone(ctx, L, chunk):
    n_seq, heads = 3, 2
    q, k, v = db.make_qkv("randn", n_seq, L, L, heads, L)
    mk = db.make_mask("rect", n_seq, L)
    clean = run(ctx, q, k, v, mk, n_seq, L, L, heads, chunk=chunk).view(n_seq, L, -1)
    dead = mk.clone()
    dead[1] = 1
    got = run(ctx, q, k, v, dead, n_seq, L, L, heads, chunk=chunk).view(n_seq, L, -1)
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    assert db.worst(got.view(n_seq * L, -1), db.reference(q, k, v, dead, n_seq, L, L, heads)) <= 1.0


def test_non_finite_values_under_the_mask_and_behind_lk_stay_out(ctx):
    """NaN in the K rows of masked keys does not reach the output (a masked score is replaced, not added to); NaN in ANOTHER sequence's
    rows - what follows this sequence's last key in memory - does not either (the LDS rows behind Lk repeat this sequence's last row and
    are read as zeros)"""
    n_seq, heads, L = 3, 2, 97
    q, k, v = db.make_qkv("randn", n_seq, L, L, heads, 11)
    mk = db.make_mask("head64", n_seq, L)
    clean = run(ctx, q, k, v, mk, n_seq, L, L, heads).view(n_seq, L, -1)
    k2, v2 = k.clone().view(n_seq, L, -1), v.clone().view(n_seq, L, -1)
    k2[0, :64] = float("nan")          # masked keys of sequence 0
    k2[2], v2[2] = float("nan"), float("nan")      # the whole of sequence 2, behind sequence 1's last key
    got = run(ctx, q, k2.view(n_seq * L, -1), v2.view(n_seq * L, -1), mk, n_seq, L, L, heads).view(n_seq, L, -1)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1])
    assert not torch.isfinite(got[2]).any()


def test_refusals_write_nothing(ctx):
    heads, D = 2, 64
    lib = _lib.lib()
    big = torch.zeros(MAX_L + 1, D, device="cuda")
    out = torch.full((MAX_L + 9, D), float("nan"), device="cuda")
    for Lq, Lk, chunk, layout in ((MAX_L, MAX_L + 1, 0, 1), (MAX_L + 1, MAX_L, 0, 1), (0, 32, 0, 1), (32, 0, 0, 1), (32, 32, 48, 0),
                                  (32, 32, 1312, 0), (32, 64, 0, 0), (32, 32, 0, 3)):
        rc = lib.hg_test_detr_attention(ctx, big.data_ptr(), big.data_ptr(), big.data_ptr(), None, 1, Lq, Lk, heads, chunk, layout, 0,
                                        out.data_ptr(), None)
        assert rc == HG_ERR_INVALID, (Lq, Lk, chunk, layout)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    got = run(ctx, big[:MAX_L].cpu(), big[:MAX_L].cpu(), big[:MAX_L].cpu() + 1, None, 1, MAX_L, MAX_L, heads)      # the maximum itself runs
    assert (got == 1).all()
