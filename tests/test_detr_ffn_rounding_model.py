"""The bound of tests/detr_ffn_bound.py proved on the CPU: the restatement of the split FFN kernel and the decoder layer's tail stays
inside it on every family, at the pre-norm sum, the stream and the final norm's output; on the families whose arithmetic is exact in
fp32 the partial sums and the pre-norm sum equal the float64 values bit for bit; and each wrong kernel breaks it.  No GPU, no library."""
import numpy as np
import pytest

import detr_ffn_bound as fb

SHAPES = ((1, 128, 128), (33, 128, 256), (70, 256, 512), (100, 256, 2048))


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(family, shape):
        key = (family, shape)
        if key not in memo:
            c = fb.make_case(family, *shape, seed=5)
            memo[key] = (c, fb.reference(c), fb.bounds(c), fb.model(c))
        return memo[key]
    return get


@pytest.mark.parametrize("family", fb.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_stays_inside_the_bound(cases, family, shape):
    c, (s, y, o), (Es, Ey, Eo), (part, ms, my, mo) = cases(family, shape)
    assert np.isfinite(Ey).all() and np.isfinite(Eo).all()
    r = [fb.worst_ratio(ms, s, Es), fb.worst_ratio(my, y, Ey), fb.worst_ratio(mo, o, Eo)]
    print(f"{family} {shape}: worst |err| / bound: pre-norm sum {r[0]:.3f}, stream {r[1]:.3f}, out {r[2]:.3f}")
    assert max(r) <= 1.0
    if family in fb.EXACT_FAMILIES:      # every product and partial sum is exact: the fp32 results are the float64 ones
        x16 = fb.f16(c["x"]).astype(np.float64)
        h = fb.f16(np.maximum(x16 @ c["w1"].astype(np.float64).T + c["b1"], 0)).astype(np.float64)
        for sl in range(shape[2] // fb.SLICE):
            u = slice(sl * fb.SLICE, (sl + 1) * fb.SLICE)
            assert np.array_equal(part[sl].astype(np.float64), h[:, u] @ c["w2"].astype(np.float64)[:, u].T)
        assert np.array_equal(ms.astype(np.float64), c["x"].astype(np.float64) + c["b2"] + h @ c["w2"].astype(np.float64).T)


# the family and shape on which each wrong kernel is shown to break the bound
BREAKS = {"drop_slice": "randn", "double_slice": "randn", "b1_wrong_slice": "randn", "b2_per_slice": "randn", "no_relu": "randn",
          "truncate_f16": "trunc", "tail_rows_neighbour": "randn", "norms_swapped": "randn", "final_norm_written_back": "randn"}


@pytest.mark.parametrize("mutant", sorted(BREAKS))
def test_a_wrong_kernel_breaks_the_bound(cases, mutant):
    shape = (70, 256, 512)
    c, (s, y, o), (Es, Ey, Eo), _ = cases(BREAKS[mutant], shape)
    _, ms, my, mo = fb.model(c, mutant)
    r = [fb.worst_ratio(ms, s, Es), fb.worst_ratio(my, y, Ey), fb.worst_ratio(mo, o, Eo)]
    print(f"{mutant}: worst |err| / bound: pre-norm sum {r[0]:.2f}, stream {r[1]:.2f}, out {r[2]:.2f}")
    assert max(r) > 1.0
    if mutant == "tail_rows_neighbour":      # ... in the last row tile only
        assert fb.worst_ratio(my[:64], y[:64], Ey[:64]) <= 1.0 < fb.worst_ratio(my[64:], y[64:], Ey[64:])


def test_relu_after_a_flushing_conversion_is_caught_where_it_changes_anything(cases):
    """fp16(a) with negative subnormals flushed to -0, then the ReLU: relu(-0) feeds -0 into linear2, where it adds nothing; the result
    has to be either the correct kernel's bits or outside the bound - there is no third way"""
    for shape in ((33, 128, 256), (70, 256, 512)):
        c, (s, y, o), (Es, Ey, Eo), (part, ms, my, mo) = cases("subn", shape)
        x16 = fb.f16(c["x"]).astype(np.float64)
        a = x16 @ c["w1"].astype(np.float64).T + c["b1"]
        assert ((a < 0) & (a > -2.0 ** -14)).mean() > 0.2, "the family has negative subnormal hidden values"
        p2, s2, y2, o2 = fb.model(c, "relu_after_flush")
        same = np.array_equal(my.view(np.int32), y2.view(np.int32)) and np.array_equal(part.view(np.int32) & 0x7fffffff, p2.view(np.int32) & 0x7fffffff)
        assert same or max(fb.worst_ratio(s2, s, Es), fb.worst_ratio(y2, y, Ey)) > 1.0


def test_positive_subnormal_hidden_values_survive():
    """a kernel that flushes fp16 subnormals to zero loses the `subn` family's hidden layer: the bound's 2^-25 term does not cover it"""
    c = fb.make_case("subn", 33, 128, 256, seed=5)
    c2 = dict(c, b1=np.full_like(c["b1"], 2.0 ** -20))
    h = fb.f16(np.maximum(fb.f16(c2["x"]).astype(np.float64) @ c2["w1"].astype(np.float64).T + c2["b1"], 0))
    assert ((h > 0) & (h < 2.0 ** -14)).mean() > 0.2
