"""Why tests/test_gpu_nonfinite_history.py poisons the workspaces with NaN and Inf: three numpy models of the ways a kernel reads what an
earlier, larger call left in a grow-only buffer, each in a leaky form (the stale value meets an exact zero in a product) and in the
closed form the code base uses (select instead of multiplying; real zeros in the pad).

  pv          masked softmax: a key behind the sequence's end gets probability exp(-inf) = 0, its V row is stale
  k_pad       a GEMM tile whose K is padded to the tile: the padded columns of the activations are stale, the weights' are zero
  row_reduce  a row tile behind M: its pad rows enter a column reduction (partial sums of statistics) with weight 0

For each: with FINITE stale data the leaky form returns the closed form's bits - 0 * x adds an exact zero, so a history test on finite
data passes on the leaky kernel -, with NaN or Inf it does not: 0 * NaN = 0 * Inf = NaN, and the poisoned-history test fails on it.
fp32 throughout, one rounding per operation in a fixed order, as an accumulator does."""
import numpy as np
import pytest

F = np.float32
STALE = {"finite": 3.0e4, "finite_huge": -3.0e38, "nan": float("nan"), "inf": float("inf")}


def accumulate(terms):
    """sum over axis 0 in order, rounded to fp32 after every addition"""
    acc = np.zeros(terms.shape[1:], F)
    for t in terms:
        acc = (acc + t).astype(F)
    return acc


def rng_rows(*shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


# ---- the three models: (stale value, leaky) -> output ----------------------------------------------------------------------------------------
def pv(stale, leaky, Lq=5, L=13, tile=32, d=8):
    q, k, v = rng_rows(Lq, d, seed=1), rng_rows(tile, d, seed=2), rng_rows(tile, d, seed=3)
    v[L:] = stale      # rows of the V tile behind the sequence: what the last call left
    k[L:] = 0          # (their keys are masked whatever they hold)
    s = (q @ k.T).astype(F)
    s[:, L:] = -np.inf
    with np.errstate(invalid="ignore"):
        p = np.exp(s - s.max(axis=1, keepdims=True)).astype(F)
        p = (p / accumulate(p.T)[:, None]).astype(F)
        assert (p[:, L:] == 0).all()
        if not leaky:
            v = np.where(np.arange(tile)[:, None] < L, v, 0).astype(F)      # pad rows of V stored as real zeros
        return accumulate((p.T[:, :, None] * v[:, None, :]).astype(F))      # every key of the tile: 0 * (pad row)


def k_pad(stale, leaky, M=7, N=6, K=40, tile=64):
    a, w = rng_rows(M, tile, seed=4), rng_rows(N, tile, seed=5)
    a[:, K:] = stale   # padded K columns of the activation copy
    w[:, K:] = 0       # the packed weights are zero there
    kk = tile if leaky else K
    with np.errstate(invalid="ignore"):
        return accumulate((a[:, :kk].T[:, :, None] * w[:, :kk].T[:, None, :]).astype(F))


def row_reduce(stale, leaky, M=21, tile=32, D=8):
    x = rng_rows(tile, D, seed=6)
    x[M:] = stale      # rows of the tile behind M
    weight = (np.arange(tile) < M).astype(F)
    with np.errstate(invalid="ignore"):
        terms = weight[:, None] * x if leaky else np.where(weight[:, None] != 0, x, 0)
        return accumulate(terms.astype(F))


MODELS = {"pv": pv, "k_pad": k_pad, "row_reduce": row_reduce}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


@pytest.mark.parametrize("name", list(MODELS))
def test_finite_stale_data_is_invisible_and_non_finite_is_not(name):
    model = MODELS[name]
    want = model(0.0, leaky=False)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    for kind, stale in STALE.items():
        closed, leaky = model(stale, leaky=False), model(stale, leaky=True)
        assert np.array_equal(bits(closed), bits(want)), f"{name}: the closed form depends on the stale data ({kind})"
        if np.isfinite(stale):
            assert np.array_equal(bits(leaky), bits(want)), f"{name}: finite stale data ({kind}) changed a bit - the model is not the exact-zero leak"
        else:
            assert not np.isfinite(leaky).all(), f"{name}: {kind} behind an exact zero stayed out of the leaky form"
            assert not np.array_equal(bits(leaky), bits(want)), f"{name}: the poisoned-history test would pass on the leaky form ({kind})"


@pytest.mark.parametrize("name", list(MODELS))
def test_a_finite_history_test_passes_on_the_leaky_form(name):
    """what tests/test_gpu_history_independence.py does, on the model: random finite histories of any size, bit-equal results"""
    model = MODELS[name]
    want = model(0.0, leaky=True)
    for stale in np.random.default_rng(9).standard_normal(16) * 1e3:
        assert np.array_equal(bits(model(F(stale), leaky=True)), bits(want))
