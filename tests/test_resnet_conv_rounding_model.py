"""The bound of tests/resnet_bound.py proved on the CPU: the restatement of the convolution kernel (`model()`) stays inside the per-element
bound on every family and equals the exact expectation of the exact families, and each of fifteen wrong kernels is rejected by the bound
or by an exact family on at least one case."""
import pytest
import torch

import resnet_bound as rb
import resnet_cases as rc

# (B, H, W, Cin, Cout, R, stride, epi): both kernel sizes and strides, two channel blocks, two images, an even side under stride 2
CASES = [(2, 5, 7, 128, 64, 3, 1, 1), (2, 8, 8, 64, 64, 3, 2, 3), (2, 5, 7, 128, 64, 1, 2, 2), (1, 8, 8, 64, 64, 1, 1, 3),
         (3, 4, 3, 64, 64, 3, 1, 3), (1, 1, 1, 64, 64, 3, 1, 1)]


def runs(mutant):
    for shape in CASES:
        for fam in rc.FAMILIES:
            c = rc.make_conv_case(fam, *shape)
            yield shape, fam, c, rb.check(c, rb.model(c, mutant))


def test_the_restatement_is_inside_the_bound_and_exact_where_it_must_be():
    top, fails = {}, []
    for shape, fam, c, (f, ratios) in runs(None):
        fails += [f"{fam} {shape}: {m}" for m in f]
        top.update({k: max(top.get(k, 0.0), v) for k, v in ratios.items()})
    print("RESNET_CONV_MODEL worst |err| / bound of the restatement: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])
    assert 0.01 < max(top.values()) <= 1.0, "a bound a hundred times the error would prove nothing"


@pytest.mark.parametrize("mutant", rb.MUTANTS)
def test_a_wrong_kernel_is_rejected(mutant):
    rejected = sum(bool(f) for _, _, _, (f, _) in runs(mutant))
    print(f"RESNET_CONV_MUTANT {mutant}: rejected by {rejected} case runs")
    assert rejected >= 1


def test_the_nan_family_reaches_exactly_the_windows_that_hold_it():
    c = rc.make_conv_case("nan", 2, 5, 7, 64, 64, 3, 1, 1)
    want = rb.reference(c)["want"]
    hit = torch.zeros(2, 5, 7, dtype=torch.bool)
    for b, y, x in rc.nan_pixels(2, 5, 7):
        hit[b, max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
    assert torch.equal(torch.isnan(want).all(1), hit) and torch.equal(torch.isnan(want).any(1), hit)
    got, clean = rb.model(c)["out16"], rb.model(rc.without_nan(c))["out16"]
    assert torch.equal(torch.isnan(got).any(1), hit)
    assert torch.equal(got[~torch.isnan(got)], clean[~torch.isnan(got)]), "a NaN changed an output outside its windows"


def test_scale_and_bias_are_made_in_double():
    n = (torch.tensor([0.7, 1e-3]), torch.tensor([0.1, -0.2]), torch.tensor([0.3, 5.0]), torch.tensor([1e-12, 0.9]), 1e-5)
    s, b = rb.scale_bias(n)
    assert torch.isfinite(s).all() and s.dtype == torch.float32
    assert abs(float(s[0]) - 0.7 / (1e-12 + 1e-5) ** 0.5) < 1e-4 * float(s[0]) and abs(float(b[1]) - (-0.2 - 5.0 * float(s[1]))) < 1e-6
