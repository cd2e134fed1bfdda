"""tests/props_bound.py against itself, on the CPU: the rule-form selection against the reference's statements, the known answers of
the constructed images, the screen's cap, and that every wrong kernel of props_bound.FLAWS fails the rules the GPU test applies."""
import functools

import numpy as np
import pytest

import props_bound as pb

RANDOM = tuple(pb.FAMILIES)


def all_cases():
    return [(n, pb.family(n)) for n in RANDOM] + [("constructed", pb.constructed()[0])]


@functools.lru_cache(maxsize=None)
def expected(name):
    case = dict(all_cases())[name]
    return case, pb.restate(case), pb.definition(case)


@pytest.mark.parametrize("name", RANDOM + ("constructed",))
def test_rule_equals_literal_statements(name):
    case = dict(all_cases())[name]
    p = case["params"]
    args = (p["human_idx"], p["box_score_thresh"], p["min_instances"], p["max_instances"])
    some = 0
    for b in range(case["B"]):
        lo, hi = case["q_off"][b], case["q_off"][b + 1]
        sc, lb, bx = case["scores"][lo:hi], case["labels"][lo:hi], case["boxes"][lo:hi]
        surv = pb.nms(sc, lb, bx, p["nms_thresh"])
        assert np.all(np.diff(sc[surv].astype(np.float64)) <= 0)
        k1, h1 = pb.select_rule(sc, lb, surv, *args)
        k2, h2 = pb.select_literal(sc, lb, surv, *args)
        assert np.array_equal(k1, k2) and h1 == h2, (name, b)
        assert len(k1) <= 2 * p["max_instances"]
        some += len(k1)
    assert some > 0


def test_constructed_known_answers():
    case, index, known = pb.constructed()
    exp = pb.restate(case)
    for name, keep in known.items():
        b = index[name]
        n = exp["counts"][b][0]
        assert list(exp["keep"][b][:n]) == keep, name
    mn, mx = case["params"]["min_instances"], case["params"]["max_instances"]
    for nh, no in ((mn - 1, mx + 1), (mn, mx), (mx, mn), (mx + 1, mn - 1)):      # below the minimum: topped up from under the threshold
        b = index[f"counts_{nh}_{no}"]
        want_h, want_o = min(max(nh, mn), mx), min(max(no, mn), mx)
        assert tuple(exp["counts"][b][:2]) == (want_h + want_o, want_h), (nh, no)
    # the pad rows are the MLP of a zero row, all alike and not zero
    b = index["empty"]
    assert exp["mask"][b].all() and np.abs(exp["priors"][b]).max() > 0 and (exp["priors"][b] == exp["priors"][b][0]).all()


@pytest.mark.parametrize("name", RANDOM)
def test_screen_stays_within_its_cap(name):
    case = pb.family(name)
    aside = sum(pb.screened(case, b) for b in range(case["B"]))
    assert aside <= 0.05 * case["B"] or (case["B"] < 20 and aside == 0), f"{aside} of {case['B']} images set aside"


@pytest.mark.parametrize("name", RANDOM + ("constructed",))
def test_restatement_passes_its_own_rules(name):
    case, exp, defn = expected(name)
    skip = range(case["B"]) if name == "constructed" else ()      # (built ON the threshold: held to the known answers instead)
    worst = pb.judge(exp, case, exp, defn, skip_rule3=skip)
    print(f"PROPS_RATIO {name} restatement {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("flaw", pb.FLAWS)
def test_wrong_kernel_is_rejected(flaw):
    """each flaw must fail `judge` on at least one case; and through rule 2 or 3 (against the float64 definition) where the flaw is one of
    meaning rather than of rounding order, so that the rejection does not rest on the restatement alone"""
    rejected = []
    for name in ("b3_ragged_2cls", "cap8", "constructed"):
        case, exp, defn = expected(name)
        got = pb.restate(case, flaw)
        try:
            pb.judge(got, case, exp, defn, skip_rule3=range(case["B"]) if name == "constructed" else ())
        except AssertionError as e:
            rejected.append((name, str(e)))
    assert rejected, f"{flaw}: passes every rule"
    independent = []
    for name in ("b3_ragged_2cls", "cap8"):
        case, exp, defn = expected(name)
        got = pb.restate(case, flaw)
        try:
            pb.judge(got, case, got, defn)      # rule 1 against itself: only rules 2 and 3 can speak
        except AssertionError as e:
            independent.append(str(e))
    # (visible only on ties, on values AT a threshold and where no coordinate is positive: the constructed images and their known answers)
    if flaw not in ("ties_reverse", "iou_ge", "score_gt", "offset_no_plus1"):
        assert independent, f"{flaw}: only the restatement notices"
    else:
        case, index, known = pb.constructed()
        got = pb.restate(case, flaw)
        assert any(list(got["keep"][index[n]][:got["counts"][index[n]][0]]) != k for n, k in known.items()), f"{flaw}: the known answers miss it"
