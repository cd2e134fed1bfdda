"""The chained per-element bound of tests/qkv_attn_bound.py, tested on the CPU: no GPU, no library.

`qkv_attn_bound.model` restates the fused in_proj + attention kernels: gb.model's epilogue 8, then ab.model's tile loop with the
kernels' tile geometry (a 208-row tile per sequence, or a 160-row pack of floor(160 / L) sequences, so that the rows behind a sequence
are really a neighbour's).  Proved here, at the vision shapes L = 193, 197, 208 x heads 6, 12 x K = D, D + 64 (3 sequences) and the text
shapes L = 1, 13, 33, 77, 80 x heads 8, 12 (two full packs and a pack of one):

* the correct restatement stays within B_A on every family - at most 0.85 B_A as measured (vision 0.79: `randn`; text 0.85: `lnfold`
  and `sel_randn` at L = 13), the projection within B_P (0.93: `lnfold`) - and on finite data it is ab.model of gb.model bit for bit;
* every wrong kernel tried (qkv_attn_bound.MUTANTS) breaks B_A on every family of CATCHERS at every shape where it is alive, and
  equals the correct restatement bit for bit where it is dead; every mutant is alive somewhere.  Measured, the smallest ratio over
  the shapes: neighbour_key 18 (`randn`) .. 44, mr_by_tile_row 3e3, bcs_heads_swapped 3e4, k_wrong_head 3e3, drop_e_columns 1e3,
  rstd_after_bias 9e2, mean_uncentred 1e3; neighbour_v is dead on finite data and makes a clean sequence non-finite on the poisoned
  form of a case wherever a key tile reaches into a poisoned neighbour's rows;
* the `sel_*` projections are exact in fp32 in two K orders, and the dense families' largest visible |score| stays at the cap.

The comparison this stands beside (3e-3 x max|ref| against fp64 SDPA of the fp32 PyTorch projection) passes every attention mutant of
tests/test_attention_rounding_model.py on some input.
"""
import pytest
import torch

import attention_bound as ab
import qkv_attn_bound as qb

VISION = [(3, L, heads, extra, False) for L in (193, 197, 208) for heads in (6, 12) for extra in (0, 64)]
TEXT = [(2 * (160 // L) + 1, L, heads, 0, True) for L in (1, 13, 33, 77, 80) for heads in (8, 12)]
SHAPES = VISION + TEXT
# the families that must catch a mutant wherever it is alive on them
CATCHERS = {"neighbour_key": ("sel_randn", "sel_voffset", "randn"), "neighbour_v": ("sel_randn", "lnfold"),
            "mr_by_tile_row": ("sel_randn", "sel_ramp", "lnfold"), "bcs_heads_swapped": ("randn", "lnfold"),
            "k_wrong_head": ("sel_randn", "sel_ramp", "randn"), "drop_e_columns": ("sel_randn", "sel_sink", "lnfold"),
            "rstd_after_bias": ("sel_voffset", "lnfold"), "mean_uncentred": ("randn", "lnfold")}


def consumed(c):
    """the q | k | v the reference is built on: a priori for sel_*, the correct projection (held to B_P) for the dense families"""
    if c["family"] in qb.SELECT:
        return c["qkv16"]
    qkv16 = qb.project(c)
    p = qb.stage_p_ratio(qkv16, c)
    print(f"QKV_ATTN_RATIO model-P {c['family']:12s} {p:.3f}")
    assert p <= 1.0, (c["family"], p)
    return qkv16


@pytest.mark.parametrize("n_seq,L,heads,extra,causal", SHAPES)
def test_the_correct_restatement_stays_within_the_bound(n_seq, L, heads, extra, causal):
    for family in qb.FAMILIES:
        c = qb.make_case(family, n_seq, L, heads, extra, causal)
        qkv16 = consumed(c)
        got = qb.model(c)
        w = ab.worst(got, qb.reference(c, qkv16))
        print(f"QKV_ATTN_RATIO model-{qb.instance(heads, c['K'], causal)} L {L} {family:12s} {w:.3f}")
        assert w <= 0.9, (family, w)
        assert torch.equal(got, ab.model(qkv16, n_seq, L, heads, causal)), "finite data: the tile geometry must not show"
        if family in qb.SELECT:
            assert qb.select_is_exact(c), family
            assert bool(torch.isfinite(c["qkv16"]).all())
        else:
            cap = qb.score_cap(c["qkv64"], n_seq, L, heads, causal)
            assert cap <= qb.SCORE_CAP * 1.01, (family, cap)


@pytest.mark.parametrize("n_seq,L,heads,extra,causal", SHAPES)
def test_every_mutant_breaks_the_bound(n_seq, L, heads, extra, causal):
    for family in sorted({f for fs in CATCHERS.values() for f in fs}):
        c = qb.make_case(family, n_seq, L, heads, extra, causal)
        ref = qb.reference(c, c["qkv16"] if family in qb.SELECT else qb.project(c))
        good = qb.model(c)
        for mutant in qb.MUTANTS:
            if mutant == "neighbour_v":
                continue
            got = qb.model(c, mutant)
            if not qb.alive(mutant, c):
                assert (got == good).all(), (mutant, family)      # dead here: the mutant IS the correct restatement
            elif family in CATCHERS[mutant]:
                w = ab.worst(got, ref)
                print(f"{mutant} L {L} heads {heads} K {c['K']} {family}: {w:.3g}")
                assert w > 1.5, (mutant, family, w)


@pytest.mark.parametrize("n_seq,L,heads,extra,causal", SHAPES)
def test_a_non_finite_neighbour_stays_out_unless_its_v_rows_are_kept(n_seq, L, heads, extra, causal):
    for family in CATCHERS["neighbour_v"]:
        c = qb.make_case(family, n_seq, L, heads, extra, causal)
        good = qb.model(c).view(n_seq, L, -1)
        assert (qb.model(c, "neighbour_v").view(n_seq, L, -1) == good).all(), "dead on finite data"
        for poison in (float("nan"), float("inf")):
            p = qb.poisoned(c, poison)
            got = qb.model(p).view(n_seq, L, -1)
            assert bool(torch.isfinite(got[0::2]).all()) and (got[0::2] == good[0::2]).all()
            assert not torch.isfinite(got[1::2]).all(dim=(1, 2)).any(), "a poisoned sequence came out finite"
            leak = qb.model(p, "neighbour_v").view(n_seq, L, -1)[0::2]
            assert bool(torch.isfinite(leak).all()) != qb.alive("neighbour_v", c, poison=True), (family, L)


def test_every_mutant_is_alive_somewhere():
    for mutant in qb.MUTANTS:
        assert any(qb.alive(mutant, dict(family=f, n_seq=s[0], L=s[1], heads=s[2], D=64 * s[2], K=64 * s[2] + s[3], causal=s[4]), True)
                   for s in SHAPES for f in CATCHERS[mutant]), mutant


def test_the_select_projection_by_matmul():
    """the gathered qkv64 of a sel_* case is the float64 matmul of its operands, and the rotation reaches the extra block"""
    for extra, causal, L in ((0, False, 193), (64, False, 197), (0, True, 13)):
        c = qb.make_case("sel_voffset", 3, L, 6 if not causal else 8, extra, causal)
        mean, rstd = c["mr"].double()[:, :1], c["mr"].double()[:, 1:]
        want = (c["a"].double() @ c["w"].double().t() - c["cs"].double()[None] * mean) * rstd + c["bias"].double()[None]
        assert (want == c["qkv64"]).all()
        assert int((c["w"] != 0).sum(1).min()) == 1 and int((c["w"] != 0).sum(1).max()) == 1
        assert bool((c["w"][:, c["D"]:] != 0).any()) == bool(extra)
        assert float((c["qkv16"].double() - c["qkv64"]).abs().max()) <= 2.0 ** -9      # one fp16 rounding of 7 + small
