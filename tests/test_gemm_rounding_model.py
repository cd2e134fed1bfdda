"""The per-element GEMM bound of tests/gemm_bound.py, tested on the CPU: no GPU, no library.

`gemm_bound.model` restates a tile's arithmetic (fp32 accumulation K-tile by K-tile, the epilogue in fp32 in the source's order, RNE to
fp16, per-group (sum, M2) and finalize_stats_row).  Three statements are proved here:

* the correct restatement stays within the bound B on every input family, epilogue, with and without bias, at the small shapes
  tests/test_gpu_gemm.py runs, and gives the `exact` / `tiny` expectations bit for bit;
* every wrong kernel tried (gemm_bound.MUTANTS) breaks B somewhere; KILLERS names, per mutant, the family, shape, epilogue and checked
  quantity that must catch it, so that a family cannot lose its purpose unnoticed;
* the reference quantities agree with a loop written out element by element.

The comparison this replaces (3e-3 x max|want| against an fp32 matmul on the device) passed every one of these mutants on some input.
"""
import math

import pytest
import torch

import gemm_bound as gb

# the small shapes of tests/test_gpu_gemm.py: the simple kernel's (any M, N % 128) and the smallest ring / duo shapes (N % 256)
SHAPES = [(1, 128, 64), (127, 128, 64), (129, 256, 128), (130, 384, 256), (257, 128, 3072), (641, 256, 256), (513, 768, 320),
          (641, 256, 832)]
PATCH = dict(G=4, L=5)          # epilogue 5: 32 images x 4 patches -> 160 output rows, class rows 0, 5, 10, ...
PATCH_SHAPE = (128, 128, 64)


def epilogues(family, N):
    if family in gb.LN_FAMILIES:
        return [8, 9] if N % 256 == 0 else []
    if family in gb.RESID_FAMILIES:
        return [10, 12] if N % 256 == 0 else []
    return [0, 1, 2, 3, 4, 6, 7, 11] + ([8, 9, 10, 12] if N % 256 == 0 else [])


def kwargs(epi):
    return {"n_split": 64} if epi == 11 else {}


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_the_correct_restatement_stays_within_the_bound(M, N, K):
    for family in gb.FAMILIES + gb.LN_FAMILIES + gb.RESID_FAMILIES:
        c = gb.make_case(family, M, N, K)
        for epi in epilogues(family, N):
            for bias in (True, False):
                r = gb.ratios(c, epi, gb.model(c, epi, bias=bias, **kwargs(epi)), bias=bias, **kwargs(epi))
                print(f"GEMM_RATIO model {epi} {family} bias {int(bias)} " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
                assert max(r.values()) <= 1.0, (family, epi, bias, r)
                if family in ("exact", "tiny") and epi in ((0, 2, 3, 4, 6, 7, 11) if family == "exact" else (0,)):
                    assert torch.equal(gb.model(c, epi, bias=bias, **kwargs(epi))["out"], gb.exact_expected(c, epi, bias=bias, **kwargs(epi)))


def test_patch_epilogue_in_the_model():
    M, N, K = PATCH_SHAPE
    for family in ("exact", "randn"):
        c = gb.make_case(family, M, N, K, M // PATCH["G"] * PATCH["L"])
        for pos in (True, False):
            got = gb.model(c, 5, pos=pos, **PATCH)
            assert gb.ratios(c, 5, got, pos=pos, **PATCH)["out"] <= 1.0
            assert torch.equal(got["out"][::PATCH["L"]], c["x0"][::PATCH["L"]]), "class-token rows"
            if family == "exact":
                assert torch.equal(got["out"], gb.exact_expected(c, 5, pos=pos, **PATCH))
            assert gb.ratios(c, 5, gb.model(c, 5, "patch_no_cls", pos=pos, **PATCH), pos=pos, **PATCH)["out"] > 1.5


# mutant -> (family, shape, epilogue, checked quantity) that must catch it (measured ratios in the comments; B must be broken by a quarter at least)
KILLERS = {
    "bias_shift4": [("randn", (129, 256, 128), 0, "out"), ("exact", (127, 128, 64), 4, "out"), ("offset", (641, 256, 256), 10, "out")],   # 5e3, 4e3, 2e3
    "drop_last_k": [("exact", (127, 128, 64), 4, "out"), ("randn", (641, 256, 832), 0, "out")],                                        # 1e4, 170
    "f16_partials": [("outlier", (641, 256, 832), 0, "out"), ("randn", (127, 128, 64), 4, "out")],                                     # 12, 32
    "gelu_1p7": [("randn", (127, 128, 64), 1, "out"), ("lnfold", (641, 256, 256), 9, "out")],                                          # 4.4, 4.0
    "f16_truncate": [("exact", (641, 256, 256), 0, "out"), ("tiny", (129, 256, 128), 0, "out"), ("offset", (641, 256, 256), 10, "copy")],   # 1.9, 2.0, 2.0
    "f16_flush": [("tiny", (129, 256, 128), 0, "out"), ("tiny", (641, 256, 832), 2, "out")],                                           # 2e3
    "rstd_after_bias": [("lnfold", (641, 256, 256), 8, "out"), ("lnfold", (129, 256, 128), 9, "out")],                                # 1e4
    "mean_uncentred": [("offset", (641, 256, 256), 10, "mr0"), ("wide", (129, 256, 128), 12, "mr0")],                                 # 2e5
    "var_naive": [("offset", (641, 256, 256), 10, "rstd"), ("offset", (641, 256, 832), 12, "rstd")],                                  # 200, 110
    "copy_new_mean": [("randn", (641, 256, 256), 10, "copy"), ("wide", (641, 256, 832), 12, "copy")],                                 # 4e6
    "relu_split_swapped": [("randn", (127, 128, 64), 11, "out"), ("exact", (641, 256, 832), 11, "out")],                             # 2e5, 2e3
}


@pytest.mark.parametrize("mutant", sorted(KILLERS))
def test_every_mutant_breaks_the_bound(mutant):
    for family, (M, N, K), epi, key in KILLERS[mutant]:
        c = gb.make_case(family, M, N, K)
        r = gb.ratios(c, epi, gb.model(c, epi, mutant, **kwargs(epi)), **kwargs(epi))
        print(f"{mutant} {family} {M}x{N}x{K} epilogue {epi}: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert r[key] > 1.25, (mutant, family, (M, N, K), epi, r)


def test_every_mutant_is_alive_somewhere():
    assert set(KILLERS) | {"patch_no_cls"} == set(gb.MUTANTS)          # (patch_no_cls: test_patch_epilogue_in_the_model)
    for mutant, killers in KILLERS.items():
        family, (M, N, K), epi, _ = killers[0]
        c = gb.make_case(family, M, N, K)
        a, b = gb.model(c, epi, mutant, **kwargs(epi)), gb.model(c, epi, **kwargs(epi))
        assert any(not torch.equal(a[k], b[k]) for k in a), mutant


def test_truncation_is_caught_bit_for_bit_where_the_bound_is_loose():
    """K = 3072: the accumulation term K 2^-23 S is ten times the fp16 term and B no longer sees a truncated conversion; the `exact`
    family's torch.equal expectation does"""
    c = gb.make_case("exact", 257, 128, 3072)
    got = gb.model(c, 0, "f16_truncate")
    assert gb.ratios(c, 0, got)["out"] <= 1.0
    assert not torch.equal(got["out"], gb.exact_expected(c, 0))
    assert torch.equal(gb.model(c, 0)["out"], gb.exact_expected(c, 0))


def test_tiny_family_has_subnormal_outputs():
    c = gb.make_case("tiny", 129, 128, 320)
    want = gb.exact_expected(c, 0)
    sub = (want != 0) & (want.abs() < 2.0 ** -14)
    assert 0.08 < float(sub.float().mean()) < 0.16
    flushed = gb.model(c, 0, "f16_flush")["out"]
    assert torch.equal(flushed != want, sub), "flushing changes exactly the subnormal outputs"


def test_reference_quantities():
    """acc, S and the expressions of epilogues 0, 1, 3, 7, 8, 11 against a loop written out, 5 x 8 x 64"""
    M, N, K = 5, 8, 64
    c = gb.make_case("randn", M, N, K)
    a, w, b, x0, sc = c["a"].tolist(), c["w"].tolist(), c["bias"].tolist(), c["x0"].tolist(), c["scale"].tolist()
    mr, mu, cs = c["mr"].tolist(), c["mu"].tolist(), c["cs"].tolist()
    k = float(gb.K_GELU)
    wants = {e: gb.reference(c, e, **kwargs(e))[0] for e in (0, 1, 3, 7, 8, 11)}
    for m in range(M):
        for n in range(N):
            acc = math.fsum(a[m][i] * w[n][i] for i in range(K))
            S = math.fsum(abs(a[m][i] * w[n][i]) for i in range(K))
            assert math.isclose(float(c["acc"][m, n]), acc, rel_tol=1e-12, abs_tol=1e-14)
            assert math.isclose(float(c["S"][m, n]), S, rel_tol=1e-12)
            v = acc + b[n]
            expect = {0: v, 1: v / (1 + 2.0 ** (k * v)), 3: x0[m][n] + v, 7: x0[m][n] + v * sc[n],
                      8: (acc - cs[n] * mr[m][0]) * mr[m][1] + b[n],
                      11: max(v + mu[m] * math.fsum(w[n]), 0.0)}
            for e, val in expect.items():
                assert math.isclose(float(wants[e][m, n]), val, rel_tol=1e-11, abs_tol=1e-13), (e, m, n)
    # epilogue 11 at n_split = 64 > N: every column below the split, ReLU on all of them
    assert bool((gb.reference(c, 11, n_split=64)[0] >= 0).all())
    # the accumulation term alone, where nothing else is added: fp32 output without a bias
    _, B = gb.reference(c, 4, bias=False)
    assert torch.equal(B, K * 2.0 ** -23 * c["S"])
