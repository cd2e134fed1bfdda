"""CPU side of the heads' rule (tests/heads_bound.py): the restatements of hg_cache_logits (with hg_load_cache's folding, the padded
layouts, the chunk loop and copy_cols) and of hg_mlp_net stay inside the per-element bound on every family and are bit-equal to the
float64 result on the exact families; every named mutant is rejected - by the bound, or by the exact family's bits - on the committed
cases.  Prints HEADS_RATIO lines (the `model` rows of the table in heads_bound's docstring).

File total on the build machine: about 3 s."""
import pytest
import torch

import heads_bound as hb

# (R, S, C, K, chunk_rows): C and S off the 128 grid (Nout < Np), Sp of two and three 128-blocks, several chunks with an absorbed tail
SHAPES = [(45, 77, 24, 64, 16), (37, 129, 117, 256, 32), (20, 300, 256, 64, 1 << 30)]
MLP_SHAPES = [(33, 64, 128, 128), (17, 512, 512, 512), (9, 1536, 256, 128)]


def judge(c, got, rows=None):
    """(worst |err| / E, bit-equal on the exact family or None)"""
    if "dims" in c:
        want, E = hb.mlp_reference(c, rows)
        exact = hb.mlp_exact(c, rows) if c["family"] == "exact" else None
    else:
        want, E = hb.cache_reference(c, rows)
        exact = hb.cache_exact(c, rows) if c["family"] in hb.EXACT_FAMILIES else None
    return hb.worst(got, want, E), (None if exact is None else bool(torch.equal(got, exact)))


@pytest.mark.parametrize("family", hb.CACHE_FAMILIES)
@pytest.mark.parametrize("labels", [True, False])
def test_cache_model_is_inside_the_bound(family, labels):
    worst = 0.0
    for R, S, C, K, chunk in SHAPES:
        c = hb.cache_case(family, R, S, C, K, labels)
        r, bits = judge(c, hb.cache_model(c, None, chunk))
        worst = max(worst, r)
        assert r <= 1.0, (family, labels, R, S, C, K, r)
        assert bits is not False, "the exact family is not bit for bit the float64 result"
    print(f"\nHEADS_RATIO cache {'labels' if labels else 'linear'} {family} model: worst |err| / E {worst:.3f}")


@pytest.mark.parametrize("family", hb.MLP_FAMILIES)
def test_mlp_model_is_inside_the_bound(family):
    worst = 0.0
    for R, d_in, hid, d_out in MLP_SHAPES:
        c = hb.mlp_case(family, R, d_in, hid, d_out)
        r, bits = judge(c, hb.mlp_model(c))
        worst = max(worst, r)
        assert r <= 1.0, (family, d_in, hid, d_out, r)
        assert bits is not False
    print(f"\nHEADS_RATIO mlp_net {family} model: worst |err| / E {worst:.3f}")


def test_chunk_rule():
    assert hb.chunks(1088, 512) == [512, 576] and hb.chunks(1089, 512) == [512, 512, 65] and hb.chunks(289, 256) == [256, 33]
    assert hb.chunks(288, 256) == [288] and hb.chunks(45, 16) == [16, 16, 13] and hb.chunks(0, 512) == []


@pytest.mark.parametrize("mutant", hb.CACHE_MUTANTS)
def test_cache_mutant_is_rejected(mutant):
    """on (45, 77, 24, 64) in chunks of 16 rows and (37, 129, 117, 256) in chunks of 32 (Sp = 256 != Cp = 128)"""
    seen = {}
    for R, S, C, K, chunk in SHAPES[:2]:
        for family in ("exact", "rounded", "randn", "biasdom"):
            c = hb.cache_case(family, R, S, C, K, True)
            r, bits = judge(c, hb.cache_model(c, mutant, chunk))
            seen[(family, K)] = (round(r, 3), bits)
    print(f"\nHEADS_MUTANT {mutant}: (worst |err| / E, exact bits) {seen}")
    assert any(r > 1.0 or bits is False for r, bits in seen.values()), seen
    if mutant != "phi_truncate":          # one fp16 step of phi is inside the bound by construction: the exact family's bits carry it
        assert any(r > 1.0 for r, _ in seen.values()), seen


@pytest.mark.parametrize("mutant", hb.MLP_MUTANTS)
def test_mlp_mutant_is_rejected(mutant):
    seen = {}
    for family in ("exact", "randn"):
        c = hb.mlp_case(family, *MLP_SHAPES[0])
        seen[family] = judge(c, hb.mlp_model(c, mutant))
    print(f"\nHEADS_MUTANT {mutant}: {seen}")
    assert all(r > 1.0 for r, _ in seen.values()) and seen["exact"][1] is False


def test_phi_beyond_fp16_is_refused_by_the_reference():
    c = dict(hb.cache_case("randn", 4, 77, 24, 64, True))
    c["f"] = c["f"] * 3e5
    with pytest.raises(AssertionError, match="65504"):
        hb.cache_reference(c)
