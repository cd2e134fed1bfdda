"""tests/detections_bound.py against itself, on the CPU: the restatement equals the reference's own statements on every family (rule 2),
its labels and det_gt equal the float64 definition's outside the screen (rule 3), the screen sets aside at most 5 % of a family's images,
the constructed images have the hand-derived answers, and judge() rejects each wrong kernel of FLAWS.

Flaws that only the constructed images catch (the random families draw continuous coordinates and scores, so exact ties, an IoU exactly on
the threshold and NaN never occur there): iou_ge, score_ties_high, nan_zero.  Every other flaw is also rejected on a random family
(CAUGHT_BY below names one each; argmax_last shows there through the IoUs that are exactly 0)."""
import functools

import numpy as np
import pytest

import detections_bound as db

MAX_SCREENED = 0.05
ONLY_CONSTRUCTED = ("iou_ge", "score_ties_high", "nan_zero")
CAUGHT_BY = {"argmax_last": "b8_nc63", "no_class_filter": "b8_nc63", "every_gt_candidate": "b8_nc117_conv", "tp_per_detection": "b8_nc63", "rank_by_iou": "b8_nc63",
             "human_only": "b8_nc63", "product": "b8_nc63", "union_no_inter": "b8_nc63", "column_major": "b8_nc63",
             "conversion_transposed": "b3_nc24_conv", "cx_minus_w": "b3_nc24_conv", "gt_unscaled": "b3_nc24_conv", "hw_swapped": "b3_nc24_conv"}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, restatement, float64 definition).  Cached: leave unchanged."""
    case = db.constructed()[0] if name == "constructed" else db.family(name)
    return case, db.restate(case), db.definition(case)


@pytest.mark.parametrize("name", tuple(db.FAMILIES))
def test_restatement_is_the_reference_and_the_definition(name):
    case, exp, defn = expected(name)
    n_screened = db.judge(db.literal(case), case, exp, defn)          # rule 2 (judge's rule 1 on the literal run) and rule 3
    print(f"DET_SCREENED {name} {n_screened} of {case['B']}")
    assert n_screened <= MAX_SCREENED * case["B"]


def test_screen_rate_of_the_draw():
    """the families' draw over 320 images of 20 pairs and 5 ground-truth pairs: at most 5 % screened, none of the others disagrees"""
    total = 0
    for seed in range(5):
        case = db.random_case(100 + seed, 24, (20,) * 64, (5,) * 64, gt_format=seed % 2)
        total += db.judge(db.restate(case), case)
    print(f"DET_SCREENED draw {total} of 320")
    assert total <= MAX_SCREENED * 320


def test_constructed_images():
    case, index, known = db.constructed()
    _, exp, _ = expected("constructed")
    db.check_known(exp, case, index, known)
    db.judge(db.literal(case), case, exp, skip_rule3=range(case["B"]))      # (built ON the thresholds: held to the known answers)
    assert list(exp["status"]) == [0] * (case["B"] - 1) + [1]


def test_screen_fires_on_the_threshold_and_on_a_tie():
    case, index, _ = db.constructed()
    assert db.screened(case, index["iou_exactly_half"]) and db.screened(case, index["equal_over_two_gt"])
    assert not db.screened(case, index["other_class"]) and not db.screened(case, index["no_ground_truth"])


def rejected(case, exp, defn, flaw, constructed=False):
    got = db.restate(case, flaw)
    try:
        db.judge(got, case, exp, defn, skip_rule3=range(case["B"]) if constructed else ())
        if constructed:
            db.check_known(got, *db.constructed())
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("flaw", db.FLAWS)
def test_wrong_kernel_is_rejected(flaw):
    case, exp, defn = expected("constructed")
    on_constructed = rejected(case, exp, defn, flaw, constructed=True)
    if flaw in ONLY_CONSTRUCTED:
        assert on_constructed
        return
    case, exp, defn = expected(CAUGHT_BY[flaw])
    assert rejected(case, exp, defn, flaw), f"{flaw} passes on {CAUGHT_BY[flaw]}"


def test_only_constructed_is_what_it_says():
    """the three flaws above pass on every random family: the constructed images are what rejects them"""
    for flaw in ONLY_CONSTRUCTED:
        for name in ("b3_nc24_conv", "b8_nc63", "b3_nc65"):
            assert not rejected(*expected(name), flaw), (flaw, name)


def test_apply_cap():
    case, exp, _ = expected("b8_nc63")
    cut = db.apply_cap(exp, int(exp["det_off"][3]) - 1)
    assert list(cut["status"] & 4) == [0, 0, 4, 4, 4, 4, 4, 4] and len(cut["verb"]) == exp["det_off"][3] - 1
    assert np.array_equal(cut["det_off"], exp["det_off"])
