"""The per-element bounds of tests/elem_bound.py, tested on the CPU: no GPU, no library.

`elem_bound.model_*` restate the arithmetic kernels of hg_elem.hip in fp32 numpy (LayerNorm, rowstats_cast - layernorm_rowstats
is the one behind the other -, finalize_stats_row in both of its addition orders, fold_ln).  Proved here:

* the correct restatement stays within the bound on every family at every shape tests/test_gpu_elem.py runs, and meets the bit-for-bit
  expectations of the `constant` and `exact` families;
* every wrong kernel tried (elem_bound.MUTANTS) breaks the bound at a named family (KILLERS);
* the reference quantities agree with a loop written out element by element, and the lo layout with the index formula spelled out.
"""
import math

import numpy as np
import pytest

import elem_bound as eb

f32 = np.float32
FIN_SHAPES = [(2, 64), (4, 64), (8, 64), (12, 64), (16, 64), (12, 32)]
FIN_MS = (1, 255, 256, 257)
FOLD_SHAPES = [(1, 64), (5, 64), (128, 768), (7, 1000)]
_worst = {}


def note(kernel, family, r):
    _worst[(kernel, family)] = max(_worst.get((kernel, family), 0.0), r)


def flush():
    """one line per kernel and family, as the GPU tests print them"""
    for (kernel, family), r in sorted(_worst.items()):
        print(f"ELEM_RATIO model {kernel} {family} {r:.3f}")
    _worst.clear()


@pytest.mark.parametrize("D", eb.DS)
def test_layernorm_and_rowstats_model_within_the_bound(D):
    w, b = eb.make_affine(D)
    for M in eb.MS:
        for family in eb.ROW_FAMILIES:
            if family == "nonfinite":
                continue
            x = eb.make_rows(family, M, D)
            for f16 in (True, False):
                want, B = eb.layernorm_reference(x, w, b, f16)
                y = eb.model_layernorm(x, w, b, f16)
                r = eb.worst(y, want, B)
                note(f"layernorm_{'f16' if f16 else 'f32'}", family, r)
                assert r <= 1.0, ("layernorm", f16, family, M, D, r)
                eb.check_constant_layernorm(family, x, y, b.astype(np.float16).astype(f32) if f16 else b)
            for gamma in (None, w):
                got = eb.model_rowstats(x, gamma)
                r = eb.family_stats_ratios(family, x, got["mr"], got["mu"], got["x16"], gamma)
                for k, v in r.items():
                    note(f"rowstats_cast{'_gamma' if gamma is not None else ''}.{k}", family, v)
                assert max(r.values()) <= 1.0, ("rowstats", family, M, D, r)
                assert not np.any(got["mr"][:, 0]) and np.array_equal(got["mu"], got["muc"])
    flush()


def test_nonfinite_rows_stay_in_their_rows_in_the_model():
    M, D = 5, 260
    w, b = eb.make_affine(D)
    x, clean = eb.make_rows("nonfinite", M, D), eb.make_rows("randn", M, D)
    bad = eb.nonfinite_rows(M)
    good = [r for r in range(M) if r not in bad]
    y, y0 = eb.model_layernorm(x, w, b, False), eb.model_layernorm(clean, w, b, False)
    assert np.array_equal(y[good], y0[good]) and not np.isfinite(y[bad]).any()


@pytest.mark.parametrize("nt,gw", FIN_SHAPES)
def test_finalize_stats_model_within_the_bound(nt, gw):
    for M in FIN_MS:
        for family in ("randn", "offset", "small", "wide"):
            for centred in (False, True):
                stats, mu = eb.make_stats(family, M, nt, gw, centred)
                for order in ("loop",) + (("nt12",) if nt == 12 else ()):
                    got = eb.model_finalize(stats, mu, gw, centred, order)
                    r = eb.finalize_ratios(stats, mu, gw, centred, got["mr"], got["mu"])
                    for k, v in r.items():
                        note(f"finalize_stats{'_nt12' if order == 'nt12' else ''}.{k}", family, v)
                    assert max(r.values()) <= 1.0, (family, M, nt, gw, centred, order, r)
                    assert np.array_equal(got["muc"], mu)
    flush()


@pytest.mark.parametrize("N,K", FOLD_SHAPES)
def test_fold_ln_model_within_the_bound(N, K):
    for family in eb.FOLD_FAMILIES:
        w16, gamma, beta, bias = eb.make_fold(family, N, K)
        for bs in (bias, None):
            got = eb.model_fold(w16, gamma, beta, bs)
            assert np.array_equal(got["wf16"].view(np.uint16), eb.fold_wf16_expected(w16, gamma).view(np.uint16))
            r = eb.fold_ratios(w16, gamma, beta, bs, got)
            for k, v in r.items():
                note(f"fold_ln.{k}", family, v)
            assert max(r.values()) <= 1.0, (family, N, K, r)
    flush()


def _rowstats_ratio(family, M, D, key, mutant, gamma=False):
    x = eb.make_rows(family, M, D)
    g = eb.make_affine(D)[0] if gamma else None
    got = eb.model_rowstats(x, g, mutant)
    return eb.stats_ratios(x, got["mr"], got["mu"], got["x16"], g)[key]


def _ln_ratio(family, M, D, f16, mutant):
    x = eb.make_rows(family, M, D)
    w, b = eb.make_affine(D)
    want, B = eb.layernorm_reference(x, w, b, f16)
    return eb.worst(eb.model_layernorm(x, w, b, f16, mutant), want, B)


def _finalize_ratio(family, M, nt, gw, key, mutant, order="loop"):
    stats, mu = eb.make_stats(family, M, nt, gw)
    got = eb.model_finalize(stats, mu, gw, False, order, mutant)
    return eb.finalize_ratios(stats, mu, gw, False, got["mr"], got["mu"])[key]


def _fold_ratio(family, N, K, key, mutant):
    w16, gamma, beta, bias = eb.make_fold(family, N, K)
    return eb.fold_ratios(w16, gamma, beta, bias, eb.model_fold(w16, gamma, beta, bias, mutant))[key]


# mutant -> the named family, shape and quantity that must catch it (B broken by a quarter at least)
KILLERS = {
    "var_naive": [lambda m: _rowstats_ratio("offset", 1027, 256, "rstd", m), lambda m: _rowstats_ratio("offset", 5, 768, "rstd", m)],
    "no_eps": [lambda m: _ln_ratio("constant", 4, 64, False, m), lambda m: _rowstats_ratio("small", 5, 252, "rstd", m),
               lambda m: _finalize_ratio("small", 255, 12, 64, "rstd", m)],
    "unbiased": [lambda m: _rowstats_ratio("randn", 5, 256, "rstd", m), lambda m: _ln_ratio("randn", 3, 1024, True, m)],
    "copy_uncentred": [lambda m: _rowstats_ratio("offset", 3, 260, "copy", m), lambda m: _rowstats_ratio("wide", 5, 64, "copy", m, True)],
    "f16_truncate": [lambda m: _rowstats_ratio("randn", 1027, 64, "copy", m), lambda m: _ln_ratio("randn", 1027, 256, True, m)],
    "f16_flush": [lambda m: _rowstats_ratio("small", 1027, 1024, "copy", m)],
    "chan_no_cross": [lambda m: _finalize_ratio("randn", 257, 12, 64, "rstd", m, "nt12"), lambda m: _finalize_ratio("wide", 1, 2, 64, "rstd", m)],
    "mr0_sign": [lambda m: _finalize_ratio("offset", 256, 12, 64, "mr0", m), lambda m: _finalize_ratio("randn", 255, 16, 64, "mr0", m)],
    "cs_unrounded": [lambda m: _fold_ratio("drift", 5, 64, "cs", m), lambda m: _fold_ratio("drift", 7, 1000, "cs", m)],
}


@pytest.mark.parametrize("mutant", eb.MUTANTS)
def test_every_mutant_breaks_the_bound(mutant):
    for k, killer in enumerate(KILLERS[mutant]):
        r = killer(mutant)
        print(f"{mutant} killer {k}: {r:.3g}")
        assert r > 1.25, (mutant, k, r)
        assert killer(None) <= 1.0


def test_reference_quantities():
    """mean, M2, rstd, LayerNorm, Chan's merge, fold_ln's sums and the loss against loops written out"""
    M, D = 3, 8
    x = eb.make_rows("wide", M, D)
    w, b = eb.make_affine(D)
    s = eb.row_stats_reference(x)
    want, _ = eb.layernorm_reference(x, w, b, False)
    for m in range(M):
        row = [float(v) for v in x[m]]
        mean = math.fsum(row) / D
        M2 = math.fsum((v - mean) ** 2 for v in row)
        rstd = 1.0 / math.sqrt(M2 / D + eb.EPS32)
        assert math.isclose(s["mean"][m], mean, rel_tol=1e-13) and math.isclose(s["rstd"][m], rstd, rel_tol=1e-12)
        for j in range(D):
            assert math.isclose(want[m, j], (row[j] - mean) * rstd * float(w[j]) + float(b[j]), rel_tol=1e-11, abs_tol=1e-13)
    stats, mu = eb.make_stats("wide", 3, 4, 64)
    full = eb.make_rows("wide", 3, 256).astype(np.float64)
    r = eb.finalize_reference(stats, mu, 64, False)
    assert np.allclose(r["mean"], full.mean(1), rtol=1e-6) and np.allclose(r["rstd"], 1 / np.sqrt(full.var(1) + eb.EPS32), rtol=1e-5)
    assert np.allclose(r["mr0"], full.mean(1) - mu, atol=1e-5)
    w16, gamma, beta, bias = eb.make_fold("randn", 2, 64)
    fr = eb.fold_reference(w16, gamma, beta, bias, eb.fold_wf16_expected(w16, gamma))
    for n in range(2):
        assert math.isclose(fr["bf"][n], float(bias[n]) + math.fsum(float(w16[n, k]) * float(beta[k]) for k in range(64)), rel_tol=1e-12)
        assert math.isclose(fr["csg"][n], math.fsum(float(w16[n, k]) * float(gamma[k]) for k in range(64)), rel_tol=1e-12)
    g = np.random.default_rng(5)
    a = [g.standard_normal((2, 3)).astype(f32) for _ in range(4)]
    loss, _ = eb.vae_loss_reference(*a)
    tot = math.fsum((float(a[0][i, j]) - float(a[1][i, j])) ** 2 - 0.5 * (1 + float(a[3][i, j]) - float(a[2][i, j]) ** 2 - math.exp(float(a[3][i, j])))
                    for i in range(2) for j in range(3))
    assert math.isclose(loss, tot / 2, rel_tol=1e-12)


def test_lo_fragment_order_against_the_index_formula():
    """the reshape / transpose of elem_bound.lo_fragment_order against the comment's formula evaluated element by element"""
    R, D = 256, 512
    lo = (np.arange(R * D, dtype=np.int64) * 2654435761 % 251).astype(np.uint8).reshape(R, D)
    flat = eb.lo_fragment_order(lo)
    g = np.random.default_rng(1)
    for row, col in zip(g.integers(0, R, 500), g.integers(0, D, 500)):
        tile = (row // 128) * (D // 256) + col // 256
        wave = (row % 64) // 32 * 4 + (col % 128) // 32
        piece = (row // 64 % 2) * 4 + (col // 128 % 2) * 2 + col // 16 % 2
        lane = (col % 16) // 4 * 16 + row % 16
        byte = (row % 32) // 16 * 4 + col % 4
        assert flat[(((tile * 8 + wave) * 8 + piece) * 64 + lane) * 8 + byte] == lo[row, col]


def test_families_are_what_they_claim():
    x = eb.make_rows("exact", 5, 260).astype(np.float64)
    assert np.array_equal(x * 8, np.round(x * 8)) and np.array_equal(x.sum(1) / 260 * 4, np.round(x.sum(1) / 260 * 4))
    x = eb.make_rows("constant", 7, 64)
    assert np.all(x[::3] == x[::3, :1]) and np.all(x[1].std() > 0.5)
    x = eb.make_rows("small", 1027, 1024).astype(np.float64)
    d = np.abs(x - x.mean(1, keepdims=True))
    assert 1e-4 < float(((d < 2.0 ** -14) & (d > 0)).mean()) < 1e-2, "some of the copy's elements are fp16 subnormals"
    x = eb.make_rows("nonfinite", 5, 64)
    assert np.isinf(x[0]).sum() == 1 and np.isnan(x[2]).sum() == 1 and np.isfinite(x[[1, 3, 4]]).all()
    assert np.array_equal(eb.remainder_expected(f32([1.0, 1.0 + 2.0 ** -12, 1e-30, -0.0])).astype(np.float64), [0.0, 0.5, 0.0, 0.0])
