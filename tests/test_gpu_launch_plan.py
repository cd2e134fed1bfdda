"""What a tower call launches, pinned: for every path the tower runner can take (hoigen_amd/csrc/hg_tower.hip) the ordered
(kind, M, N, K) records of one call under hg_profile (HG_PROF_ALL) and hg_workspace_bytes after it, in a fresh context, against
tests/golden/launch_plans.json - exactly.  The fixture was recorded on an MI355X before the runner was split into a planning step and
named launch steps; a change that is meant to leave the dispatch alone must not need it regenerated.  The cases and the recorder live
beside the fixture (tests/golden/make_golden_launch_plans.py).

HG_PROF_ALL sees GEMM, attention, fused in_proj + attention and MLP pair launches; the order of the elementwise launches between them
(LayerNorm, row statistics, copies) is covered by the bit-identity and parity tests (test_gpu_stream_trace.py, test_gpu_parity.py).
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_launch_plans as lp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(lp.FIXTURE) as f:
        want = json.load(f)
    yield want
    lp.release()


def test_fixture_holds_exactly_the_cases():
    with open(lp.FIXTURE) as f:
        assert list(json.load(f)) == [c[0] for c in lp.CASES]


@pytest.mark.parametrize("case", lp.CASES, ids=[c[0] for c in lp.CASES])
def test_launches_and_workspace_match_the_recorded_plan(case, golden):
    got, want = lp.record(case), golden[case[0]]
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, f"{case[0]}: launch {i} is (kind, M, N, K) = {g}, recorded {w}"
    assert len(got["launches"]) == len(want["launches"]), f"{case[0]}: launches beyond the common prefix differ"
    assert got["workspace_bytes"] == want["workspace_bytes"], f"{case[0]}: workspace bytes"
