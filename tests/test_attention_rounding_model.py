"""The per-element attention bound of tests/attention_bound.py, tested on the CPU: no GPU, no library.

`attention_bound.model` restates the kernels' tile loop (tile_softmax_pv, hg_attn_dev.h).  Two statements are proved here:

* the correct restatement stays within the bound B on every input family - at most 0.75 B as measured (worst: `ramp`, causal, L = 77:
  0.71), so a kernel has a quarter of B left for what the restatement does not carry (the order of fp32 additions in the MFMA, v_exp_f32);
* every wrong kernel tried - the softmax scale off by 0.3 %, key L unmasked (with the V row the kernels stage behind it, and with a zero
  V row), fp16 subnormal probabilities flushed to zero, the causal diagonal missing for the last query of a tile, key L - 1 dropped -
  breaks B on at least one family at every length and mask where it changes anything at all.  Which family catches which mutant is
  asserted as well (CATCHERS), so that a family cannot lose its purpose unnoticed.

The comparison this replaces (2e-3 x max|want| against fp32 PyTorch on the device) passed every one of these mutants on some input.
"""
import functools

import pytest

import attention_bound as ab

N_SEQ, HEADS = 2, 2
CASES = [(33, False), (77, True), (197, False), (225, False)]          # (L, causal)
# the families that must catch a mutant wherever it is alive (measured: scale 5.6 - 13 x B, unmasked key 20 - 790 x on randn / ramp and
# 4.8 - 30 x on uniform with a zero V row, flush 37 - 71 x, diagonal 90 - 6500 x, dropped key 350 - 100 000 x)
CATCHERS = {"scale": ("randn", "ramp"), "unmasked_key": ("randn", "ramp"), "unmasked_key_zero_v": ("uniform", "randn"),
            "flush": ("sink",), "diagonal": ("randn", "ramp"), "drop_last": ("randn", "ramp")}


@functools.lru_cache(maxsize=None)
def case(family, L, causal):
    qkv = ab.make_qkv(family, N_SEQ, L, HEADS, ab.seed_of(family, L, causal, N_SEQ, HEADS))
    return qkv, ab.reference(qkv, N_SEQ, L, HEADS, causal)


@pytest.mark.parametrize("L,causal", CASES)
def test_the_correct_restatement_stays_within_the_bound(L, causal):
    for family in ab.FAMILIES:
        qkv, ref = case(family, L, causal)
        w = ab.worst(ab.model(qkv, N_SEQ, L, HEADS, causal), ref)
        print(f"L {L} causal {int(causal)} {family:8s} model {w:.3f} B")
        assert w <= 0.75, (family, w)


@pytest.mark.parametrize("L,causal", CASES)
@pytest.mark.parametrize("mutant", ab.MUTANTS)
def test_every_mutant_breaks_the_bound(mutant, L, causal):
    if not ab.alive(mutant, L, causal):
        # dead here: the mutant IS the correct restatement, bit for bit (nothing to catch)
        for family in ("randn", "uniform"):
            qkv, _ = case(family, L, causal)
            assert (ab.model(qkv, N_SEQ, L, HEADS, causal, mutant) == ab.model(qkv, N_SEQ, L, HEADS, causal)).all()
        return
    got = {}
    for family in ab.FAMILIES:
        qkv, ref = case(family, L, causal)
        got[family] = ab.worst(ab.model(qkv, N_SEQ, L, HEADS, causal, mutant), ref)
    print(f"{mutant} L {L} causal {int(causal)}: " + "  ".join(f"{f} {w:.2f}" for f, w in got.items()))
    assert max(got.values()) > 1.0, got
    for family in CATCHERS[mutant]:
        assert got[family] > 1.5, (family, got)


def test_every_mutant_is_alive_somewhere():
    for mutant in ab.MUTANTS:
        assert any(ab.alive(mutant, L, causal) for L, causal in CASES), mutant


def test_reference_quantities():
    """want, pav, Z, vsum against a loop written out for one query, and the `uniform` family's closed form"""
    import torch

    L, causal = 33, True
    qkv, ref = case("randn", L, causal)
    q, k, v = ab.split(qkv, N_SEQ, L, HEADS)
    n, h, i = 1, 0, 20
    s = (k[n, h, :i + 1] @ q[n, h, i]) * 0.125
    e = torch.exp(s - s.max())
    row, cols = n * L + i, slice(h * 64, h * 64 + 64)
    assert torch.allclose(ref["want"][row, cols], (e / e.sum()) @ v[n, h, :i + 1], rtol=1e-12, atol=0)
    assert torch.allclose(ref["pav"][row, cols], (e / e.sum()) @ v[n, h, :i + 1].abs(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["Z"][row, cols], e.sum().expand(64), rtol=1e-12, atol=0)
    assert torch.allclose(ref["vsum"][row, cols], v[n, h, :i + 1].abs().sum(0), rtol=1e-12, atol=0)
    assert float(ref["Z"].min()) >= 1.0
    qkv, ref = case("uniform", L, causal)
    _, _, v = ab.split(qkv, N_SEQ, L, HEADS)
    mean = v.cumsum(2) / torch.arange(1, L + 1, dtype=torch.float64)[None, None, :, None]
    assert torch.allclose(ref["want"], ab.rows(mean, N_SEQ, L, HEADS), rtol=1e-13, atol=0)
