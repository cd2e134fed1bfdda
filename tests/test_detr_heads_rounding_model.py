"""tests/detr_heads_bound.py on the CPU: the fp16 / fp32 restatement of hg_detr_heads.hip (`model()`) is inside `bounds()` of the float64
reference on every family and shape the GPU test runs, the exact families are exact (every sum an integer number of quanta below 2^24,
the fp32 logits equal the float64 ones), at most 15 % of a case's rows are ambiguous, and twelve wrong kernels (`MUTANTS`) are each
rejected by the bound, the label rule or an exact family.  No GPU, no library."""
import numpy as np
import pytest

import detr_heads_bound as hb


@pytest.mark.parametrize("D", (128, 256))
@pytest.mark.parametrize("C1", hb.C1S)
def test_the_restatement_is_inside_the_bound_on_every_family_and_shape(D, C1):
    top = {}
    for L, B, Q in hb.SHAPES:
        for family in hb.FAMILIES:
            c = hb.make_case(family, L, B, Q, D, C1, seed=hb.SEED)
            ref, m = hb.reference(c), hb.model(c)
            fails, stats = hb.verdict(c, m, ref)
            assert not fails, (family, L, B, Q, fails)
            assert stats["ambiguous"] <= hb.MAX_AMBIGUOUS
            top = {k: max(top.get(k, 0.0), v) for k, v in stats.items()}
            if family in hb.EXACT_FAMILIES:
                assert hb.exact_margin(c) < 1.0, (family, L, B, Q)
                assert np.array_equal(m["logits"].astype(np.float64), ref["logits"]), "the exact family's logits are not exact in fp32"
                if C1 >= 4 and B * Q >= 4:      # the planted rows: a tie at the maximum goes to the lower index; no-object greatest
                    lg = m["logits"][-1].reshape(B * Q, C1)
                    kind = (np.arange(L * B * Q) % 4)[-B * Q:]
                    r1, r3 = np.nonzero(kind == 1)[0][0], np.nonzero(kind == 3)[0][0]
                    assert lg[r1, 1] == lg[r1, C1 - 2] == lg[r1, :-1].max() and m["labels"].reshape(-1)[r1] == 1
                    assert lg[r3].argmax() == C1 - 1 and m["labels"].reshape(-1)[r3] < C1 - 1
    print(f"D {D} C1 {C1}: restatement worst |err| / bound and most ambiguous case {top}")


# mutant -> (family, (L, B, Q), C1, class_rows): a case on which the mutant differs from the kernel
CASES = {
    "softmax_foreground_only": ("randn", (1, 2, 33), 17, None),
    "max_with_no_object": ("exact_int", (1, 2, 33), 17, None),
    "tie_to_higher": ("exact_pow2", (1, 2, 33), 17, None),
    "no_relu_2": ("randn", (1, 2, 33), 17, None),
    "no_sigmoid": ("randn", (1, 2, 33), 17, None),
    "full_width": ("randn", (1, 2, 33), 17, None),
    "hw_swapped": ("randn", (1, 2, 33), 17, None),
    "scale_of_image_0": ("randn", (1, 2, 33), 17, None),
    "truncate_f16": ("exact_pow2", (1, 2, 33), 17, None),
    "class_rows_ignored": ("randn", (1, 2, 33), 17, tuple(range(2, 36, 2))),
    "level_0": ("randn", (2, 1, 257), 17, None),
    "padded_column": ("randn", (1, 2, 33), 17, None),
}


@pytest.mark.parametrize("mutant", hb.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    assert len(hb.MUTANTS) >= 10 and set(CASES) == set(hb.MUTANTS)
    family, (L, B, Q), C1, rows = CASES[mutant]
    for D in (128, 256):
        c = hb.make_case(family, L, B, Q, D, C1, seed=21, class_rows=rows)
        assert not hb.verdict(c, hb.model(c))[0], "the kernel's own restatement passes on this case"
        fails = hb.verdict(c, hb.model(c, mutant))[0]
        print(mutant, D, fails[:3])
        assert fails, f"{mutant} passes at D = {D}"


def test_class_rows_gather_is_the_direct_load():
    rows = list(range(91, 10, -1))      # 81 rows of a 94-row head, in descending order
    c = hb.make_case("randn", 1, 2, 33, 128, len(rows), seed=22, class_rows=rows)
    wc, bc = hb.class_head(c)
    direct = dict(c, wc=wc, bc=bc, class_rows=None)
    a, b = hb.model(c), hb.model(direct)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["logits"], hb.model(c, "class_rows_ignored")["logits"])
