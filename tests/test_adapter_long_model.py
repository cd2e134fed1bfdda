"""The key-chunked softmax of the instance adapter at 225 .. 640 tokens (tests/adapter_long_model.py) against the rounding model the
kernels are held to (tests/test_adapter_rounding_model.py), on the CPU: the correct restatement stays inside the project's rule, three
wrong kernels break it, and which input family catches which of them.  No GPU, no library.

Measured here (self memory, width 256, 3 sequences, L = 225, 448, 449, 577, 640; ratios to rm.model's worst row / median row):

    correct restatement          0.93 .. 1.03    0.99 .. 1.01     (fp16 probabilities against the running maximum, not the final one)
    last key chunk dropped       unit 6.8 .. 95, ramp 126 .. 552, outlier 8 .. 83; small 0.97 .. 1.01: NOT caught
    boundary key counted twice   unit 4.9 .. 17, ramp 15 .. 112; small 0.99 .. 1.02: NOT caught; outlier caught at 225 and 449 only
    no rescale                   unit 5.6 .. 30, ramp 136 .. 602, outlier 15 .. 60; small: NOT caught; reversed ramp: the median row never
                                 moves (1.00 .. 1.01), at L = 225 no row does - its maximum settles in the first chunk

so tests/test_gpu_adapter_long.py runs unit and ramp at every length, and the small-spread family is there for down_proj, not for the softmax.
"""
import functools

import pytest

import adapter_long_model as alm
import test_adapter_rounding_model as rm


@functools.lru_cache(maxsize=None)
def case(family, L, mode=0):
    x = alm.make_stream(family, 3, L, 256, 900 + 7 * L)
    _, a = rm.oracle_parts(x, rm.SD1, rm.P0, None)
    base = rm.row_errors(rm.model(x, rm.SD1, rm.P0, None, mode)["a"], a)
    return x, a, base


def ratios(family, L, mut=None, mode=0):
    x, a, base = case(family, L, mode)
    return rm.rule(rm.row_errors(alm.model_self(x, rm.SD1, rm.P0, mode, mut)["a"], a), base)


def test_one_chunk_is_the_existing_model():
    """up to 224 keys the chunked softmax is rm.model's, bit for bit"""
    for L in (33, 224):
        x = alm.make_stream("unit", 3, L, 256, 900 + 7 * L)
        for mode in (0, 1):
            want = rm.model(x, rm.SD1, rm.P0, None, mode)["a"]
            assert bool((alm.model_self(x, rm.SD1, rm.P0, mode)["a"] == want).all()), (L, mode)


@pytest.mark.parametrize("family", alm.FAMILIES)
@pytest.mark.parametrize("L", alm.LENGTHS)
def test_the_chunked_softmax_stays_inside_the_rule(L, family):
    ok, rw, rmed = ratios(family, L)
    assert ok, (rw, rmed)
    assert 0.9 <= rw <= 1.05 and 0.98 <= rmed <= 1.02, f"the restatement moved away from the model it restates: {rw:.3f} {rmed:.3f}"


@pytest.mark.parametrize("mut", alm.MUTANTS)
@pytest.mark.parametrize("family", ["unit", "ramp"])
@pytest.mark.parametrize("L", alm.LENGTHS)
def test_a_wrong_kernel_breaks_the_rule_on_unit_and_ramp(L, family, mut):
    ok, rw, rmed = ratios(family, L, mut)
    assert not ok, f"{mut}: worst-row ratio {rw:.2f}, median ratio {rmed:.2f} stays inside the rule"


@pytest.mark.parametrize("L", alm.LENGTHS)
def test_what_the_other_families_catch(L):
    # a small-spread stream (scores all but equal, every key weighs 1 / L) catches neither a dropped chunk nor a doubled key
    for mut in ("drop_last", "double"):
        ok, rw, rmed = ratios("small", L, mut)
        assert ok, f"small, {mut}: {rw:.2f} {rmed:.2f} - the family catches it after all: move it up"
    # the outlier family catches a dropped chunk and a missing rescale
    for mut in ("drop_last", "no_rescale"):
        assert not ratios("outlier", L, mut)[0], mut
    # the reversed ramp: the maximum settles in the first chunk, the median row never sees a missing rescale
    ok, rw, rmed = ratios("ramp_rev", L, "no_rescale")
    assert rmed <= 1.02, rmed
    if L == 225:
        assert ok, (rw, rmed)
    # ... while it does catch the other two
    for mut in ("drop_last", "double"):
        assert not ratios("ramp_rev", L, mut)[0], mut


def test_mode_1_reads_the_centred_copy():
    """the LayerNorm-folded path (mode 1) differs from mode 0 only in the copy down_proj reads"""
    ok, rw, rmed = ratios("unit", 577, None, 1)
    assert rw <= 1.05 and rmed <= 1.02, (rw, rmed)
    assert not ratios("unit", 577, "no_rescale", 1)[0]
