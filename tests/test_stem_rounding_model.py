"""The bound of tests/stem_bound.py proved on the CPU: the restatement of the stem kernel (`model()`) stays inside the per-element bound
on every family and shape and equals the exact expectation of the exact families, and each of twenty wrong kernels is rejected by the
bound, by an exact family or by the non-finite set on at least one case.  Also pins the float64 statement to the fixture
tests/golden/g23_resnet_stem.npz, which holds the reference's own FrozenBatchNorm2d."""
import os

import numpy as np
import pytest
import torch

import resnet_cases as rc
import stem_bound as sb
import stem_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_resnet_stem.npz")
_REF = {}


def cases():
    for shape in sc.SHAPES:
        for fam in sc.FAMILIES:
            key = (fam,) + shape
            if key not in _REF:      # computed once, shared, left unchanged
                c = sc.make_stem_case(fam, *shape)
                _REF[key] = (c, sb.reference(c))
            yield shape, fam, _REF[key]


def runs(mutant):
    for shape, fam, (c, ref) in cases():
        yield shape, fam, c, sb.check(c, sb.model(c, mutant), ref)


def test_the_restatement_is_inside_the_bound_and_exact_where_it_must_be():
    top, fails = {}, []
    for shape, fam, c, (f, ratios) in runs(None):
        fails += [f"{fam} {shape}: {m}" for m in f]
        top.update({k: max(top.get(k, 0.0), v) for k, v in ratios.items()})
    print("RESNET_STEM_MODEL worst |err| / bound of the restatement: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])
    assert 0.01 < max(top.values()) <= 1.0, "a bound a hundred times the error would prove nothing"


@pytest.mark.parametrize("mutant", sb.MUTANTS)
def test_a_wrong_kernel_is_rejected(mutant):
    rejected = sum(bool(f) for _, _, _, (f, _) in runs(mutant))
    print(f"RESNET_STEM_MUTANT {mutant}: rejected by {rejected} case runs")
    assert rejected >= 1


def test_the_nan_family_reaches_exactly_the_windows_that_hold_it():
    B, Hi, Wi = 3, 13, 18
    c = sc.make_stem_case("nan", B, Hi, Wi)
    want = sb.reference(c)["want"]
    Hp, Wp = sc.out_hw(Hi, Wi)
    hit = torch.zeros(B, Hp, Wp, dtype=torch.bool)
    for b, _, y, x in sc.nan_pixels(B, Hi, Wi):
        for ph in range(Hp):
            for pw in range(Wp):
                # the pooled pixel's valid conv pixels, and the input rows / columns their 7 x 7 windows cover
                rows = [ch for ch in (2 * ph - 1, 2 * ph, 2 * ph + 1) if 0 <= ch < sc.conv_size(Hi)]
                cols = [cw for cw in (2 * pw - 1, 2 * pw, 2 * pw + 1) if 0 <= cw < sc.conv_size(Wi)]
                if any(abs(y - 2 * ch) <= 3 for ch in rows) and any(abs(x - 2 * cw) <= 3 for cw in cols):
                    hit[b, ph, pw] = True
    assert torch.equal(torch.isnan(want).all(1), hit) and torch.equal(torch.isnan(want).any(1), hit)
    got, clean = sb.model(c), sb.model(sc.without_nan(c))
    for k in ("out32", "out16"):
        assert torch.equal(torch.isnan(got[k]).any(1), hit)
        assert torch.equal(got[k][~torch.isnan(got[k])], clean[k][~torch.isnan(got[k])]), "a NaN changed an output outside its windows"


def test_the_fixture_is_the_seeded_recipe_and_the_statement_is_the_references():
    g = np.load(GOLDEN)
    net = rc.make_resnet()
    x = sc.g23_input()
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert torch.equal(torch.from_numpy(g["x"]), x) and torch.equal(torch.from_numpy(g["conv1.weight"]), net.conv1.weight.detach())
    for k in ("weight", "bias", "running_mean", "running_var"):
        assert torch.equal(torch.from_numpy(g[f"bn1.{k}"]), getattr(net.bn1, k))
    out = torch.from_numpy(g["out"])
    assert tuple(out.shape) == (2, 64) + sc.out_hw(37, 45) == (2, 64, 10, 12)
    ref = sb.reference(sc.case_of_module(net, x), exact_norm=True)
    d64, own = float((ref["want"] - out.double()).abs().max()), float(g["out_fp32_vs_fp64_max_abs"])
    print(f"RESNET g23: float64 statement against the reference's fp32 run max abs {d64:.2e} (its own fp32-against-fp64 distance {own:.1e})")
    assert d64 <= 1.5 * own + 1e-9, "the float64 statement is not the reference's arithmetic"
    m = sb.model(sc.case_of_module(net, x))
    worst = float(((m["out32"].double() - out.double()).abs() / (ref["b32"] + 4 * own)).max())
    print(f"RESNET g23 restatement: worst |err| / (bound + 4 x {own:.1e}) {worst:.3f}")
    assert worst <= 1.0 and torch.equal(m["out16"], m["out32"].half().float())
