"""The per-element bound of tests/detr_attn_bound.py, tested on the CPU: no GPU, no library.

`detr_attn_bound.model` restates the loop of hoigen_amd/csrc/hg_detr_attn.hip.  Proved here:

* the correct restatement stays within the bound B on every input family, mask and shape tried;
* every wrong kernel tried - the scale of head dim 64, the mask ignored, shifted by one key or taken from the neighbouring sequence, a
  running maximum that starts at -inf under a tile without a visible key, a dropped partial tile, flushed fp16 subnormals, NaN in the V
  rows behind Lk - breaks B (or is not NaN / is NaN where it must not be) wherever it changes anything at all;
* the reference's own module, nn.MultiheadAttention with key_padding_mask, gives NaN rows for a sequence without a visible key and
  leaves the other sequences alone - the rule the bound module states for such sequences - and agrees with `reference` elsewhere.
"""
import functools

import pytest
import torch

import detr_attn_bound as db

N_SEQ, HEADS = 3, 2
SHAPES = [(33, 33), (1, 97), (33, 221), (70, 130)]          # (Lq, Lk)
# the masks under which `sink` keeps key 0 visible with many keys far below it: where flushed subnormals must show
FLUSH_MASKS = ("none", "rect", "midrun")


@functools.lru_cache(maxsize=None)
def case(family, Lq, Lk, mask):
    q, k, v = db.make_qkv(family, N_SEQ, Lq, Lk, HEADS, db.seed_of(family, Lq, Lk, mask, N_SEQ, HEADS))
    mk = db.make_mask(mask, N_SEQ, Lk)
    return q, k, v, mk, db.reference(q, k, v, mk, N_SEQ, Lq, Lk, HEADS)


@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_the_correct_restatement_stays_within_the_bound(Lq, Lk):
    top = {}
    for family in db.FAMILIES:
        for mask in db.MASKS:
            q, k, v, mk, ref = case(family, Lq, Lk, mask)
            w = db.worst(db.model(q, k, v, mk, N_SEQ, Lq, Lk, HEADS), ref)
            top[family] = max(top.get(family, 0.0), w)
            assert w <= 1.0, (family, mask, w)
    print(f"Lq {Lq} Lk {Lk}: " + "  ".join(f"{f} {w:.3f}" for f, w in top.items()))


@pytest.mark.parametrize("Lq,Lk", SHAPES)
@pytest.mark.parametrize("mutant", db.MUTANTS)
def test_every_mutant_breaks_the_bound(mutant, Lq, Lk):
    seen = 0
    for mask in db.MASKS:
        mk = db.make_mask(mask, N_SEQ, Lk)
        if mutant == "scale" and not db.alive(mutant, mk, N_SEQ, Lk):      # one visible key: its probability is 1 at any scale
            continue
        if not db.alive(mutant, mk, N_SEQ, Lk):
            q, k, v, mk, _ = case("randn", Lq, Lk, mask)      # dead here: the mutant IS the correct restatement, bit for bit
            a, b = db.model(q, k, v, mk, N_SEQ, Lq, Lk, HEADS, mutant), db.model(q, k, v, mk, N_SEQ, Lq, Lk, HEADS)
            assert torch.equal(a, b), (mutant, mask)
            continue
        if mutant == "flush" and (mask not in FLUSH_MASKS or Lk < 64 or Lq < 32):      # (one query is too small a sample of subnormal probabilities)
            continue
        got = {}
        for family in db.FAMILIES:
            q, k, v, mk, ref = case(family, Lq, Lk, mask)
            got[family] = db.worst(db.model(q, k, v, mk, N_SEQ, Lq, Lk, HEADS, mutant), ref)
        print(f"{mutant} Lq {Lq} Lk {Lk} {mask}: " + "  ".join(f"{f} {w:.2f}" for f, w in got.items()))
        assert max(got.values()) > 1.5, (mask, got)
        seen += 1
    assert seen or mutant in ("drop_last", "pad_v_nan", "flush"), "alive nowhere at this shape"


def test_every_mutant_is_alive_somewhere():
    for mutant in db.MUTANTS:
        assert any(db.alive(mutant, db.make_mask(mask, N_SEQ, Lk), N_SEQ, Lk) for _, Lk in SHAPES for mask in db.MASKS), mutant


def test_a_sequence_without_a_visible_key_is_nan_in_its_own_rows_as_in_multihead_attention():
    """nn.MultiheadAttention (what detr/models/transformer.py:132,155 runs) with a key_padding_mask row that is all True: NaN in that
    sequence's rows, the others untouched; `reference` and `model` say the same, and agree with the module's SDPA elsewhere."""
    Lq = Lk = 40
    D = HEADS * db.HD
    q, k, v = db.make_qkv("randn", N_SEQ, Lq, Lk, HEADS, 7)
    mk = db.make_mask("rect", N_SEQ, Lk)
    mk[1] = 1
    mha = torch.nn.MultiheadAttention(D, HEADS).double().eval()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(D, dtype=torch.float64).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(D, dtype=torch.float64))
        mha.out_proj.bias.zero_()
        sbc = lambda t, L: t.double().view(N_SEQ, L, D).transpose(0, 1)
        # (called as the reference calls it, need_weights left at its default: the softmax of a row of -inf is NaN; the fused inference
        # fast path would not run the same code)
        torch.backends.mha.set_fastpath_enabled(False)
        try:
            out = mha(sbc(q, Lq), sbc(k, Lk), sbc(v, Lk), key_padding_mask=mk.bool())[0].transpose(0, 1)
        finally:
            torch.backends.mha.set_fastpath_enabled(True)
    ref = db.reference(q, k, v, mk, N_SEQ, Lq, Lk, HEADS)
    assert ref["dead"].tolist() == [False, True, False]
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all()
    want = ref["want"].view(N_SEQ, Lq, D)
    assert torch.isnan(want[1]).all()
    for n in (0, 2):
        assert torch.allclose(out[n], want[n], rtol=1e-10, atol=1e-12)
    got = db.model(q, k, v, mk, N_SEQ, Lq, Lk, HEADS).view(N_SEQ, Lq, D)
    assert torch.isnan(got[1]).all() and db.worst(got.view(-1, D), ref) <= 1.0
    clean = db.model(q, k, v, db.make_mask("rect", N_SEQ, Lk), N_SEQ, Lq, Lk, HEADS).view(N_SEQ, Lq, D)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_reference_quantities():
    """want, pav, Z, vsum against a loop written out for one query under a rectangle mask"""
    Lq, Lk = 33, 221
    q, k, v, mk, ref = case("randn", Lq, Lk, "rect")
    q64, k64, v64 = db.split(q, N_SEQ, Lq, HEADS), db.split(k, N_SEQ, Lk, HEADS), db.split(v, N_SEQ, Lk, HEADS)
    n, h, i = 1, 1, 20
    keep = ~mk[n].bool()
    assert 0 < int(keep.sum()) < Lk
    s = (k64[n, h][keep] @ q64[n, h, i]) * db.SCALE
    e = torch.exp(s - s.max())
    row, cols = n * Lq + i, slice(h * db.HD, (h + 1) * db.HD)
    assert torch.allclose(ref["want"][row, cols], (e / e.sum()) @ v64[n, h][keep], rtol=1e-12, atol=0)
    assert torch.allclose(ref["pav"][row, cols], (e / e.sum()) @ v64[n, h][keep].abs(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["Z"][row, cols], e.sum().expand(db.HD), rtol=1e-12, atol=0)
    assert torch.allclose(ref["vsum"][row, cols], v64[n, h][keep].abs().sum(0), rtol=1e-12, atol=0)
    assert float(ref["Z"].min()) >= 1.0
