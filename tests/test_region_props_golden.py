"""tests/props_bound.py's restatement (on the CPU) and the HIP path through hoigen_amd.proposals (on the GPU) against
tests/golden/g15_region_props.npz: the outputs of the reference's own prepare_region_proposals, get_prior and MLP, executed on seeded
inputs (tests/golden/make_golden_region_props.py).  Integers and the gathered values match exactly; the priors within 1e-5 - fp32
order noise against torch's own linear over 517 columns.  The NMS inside the fixture is the restatement's: that one step is pinned to
the restatement and to the hand-derived known answers only (tests/golden/README_region_props.md)."""
import os
import sys

import numpy as np
import pytest

import props_bound as pb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import region_props_cases as rc  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_region_props.npz"))


def check(per_image, priors, mask):
    """per_image: [(boxes, scores, labels)] of the selected instances; priors [B, max_n, 64], mask [B, max_n]"""
    for b, (boxes, scores, labels) in enumerate(per_image):
        assert np.array_equal(labels, G[f"labels_{b}"]) and labels.dtype == G[f"labels_{b}"].dtype, b
        assert np.array_equal(boxes, G[f"boxes_{b}"]) and np.array_equal(scores, G[f"scores_{b}"]), b
    assert priors.shape == G["priors"].shape and np.array_equal(mask, G["mask"])
    assert np.abs(priors.astype(np.float64) - G["priors"]).max() <= 1e-5
    assert any(m.any() for m in G["mask"]) and not G["mask"].all()      # pad rows are in the comparison, and so are real ones


def test_restatement_against_the_reference_statements():
    case = rc.case()
    exp = pb.restate(case)
    n = exp["counts"][:, 0]
    per_image = [(exp["boxes"][b, :n[b]], exp["scores"][b, :n[b]], exp["labels"][b, :n[b]].astype(np.int64)) for b in range(case["B"])]
    check(per_image, exp["priors"][:, :n.max()], exp["mask"][:, :n.max()] != 0)


@pytest.mark.gpu
def test_hip_path_against_the_reference_statements():
    import torch

    from hoigen_amd import proposals

    case, w = rc.case(), rc.weights()
    t = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    sd = {f"layers.{i}.{k}": t(w[f"{'w' if k == 'weight' else 'b'}{i}"]) for i in range(3) for k in ("weight", "bias")}
    pri = proposals.InstancePriors(sd, t(w["emb"]))
    try:
        results = []
        for b in range(case["B"]):
            lo, hi = case["q_off"][b], case["q_off"][b + 1]
            results.append(dict(scores=t(case["scores"][lo:hi]), labels=t(case["labels"][lo:hi]), boxes=t(case["boxes"][lo:hi])))
        front = proposals.DetectorFrontEnd(proposals.RegionProposals(**rc.PARAMS), pri)
        region_props, (priors, mask) = front(results, torch.from_numpy(case["image_sizes"]))
    finally:
        pri.close()
    per_image = [tuple(rp[k].cpu().numpy() for k in ("boxes", "scores", "labels")) for rp in region_props]
    check(per_image, priors.cpu().numpy(), mask.cpu().numpy())
