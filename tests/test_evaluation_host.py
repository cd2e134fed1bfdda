"""The host side of hoigen_amd.evaluation, without a GPU: HOIEvaluator against tests/golden/g16_hoi_detections.npz - the reference's own
DetectionAPMeter and BoxPairAssociation executed on seeded inputs (tests/golden/make_golden_detections.py; the IoU under the association
is the restatement's, see tests/golden/README_detections.md) - and the refusals of the façade."""
import os

import numpy as np
import pytest
import torch

import detections_bound as db
from hoigen_amd import evaluation

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_hoi_detections.npz")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    case = {k: g[k] for k in ("pair_off", "box_off", "gt_off", "prior", "scores", "pair_h", "pair_o", "objects", "boxes", "gt_h", "gt_o", "gt_hoi", "gt_sizes")}
    case.update(B=int(g["B"]), NC=int(g["NC"]), gt_format=int(g["gt_format"]), min_iou=float(g["min_iou"]), conversion=None)
    return g, case, db.restate(case)


def batches(exp, labels, per=2):
    """the detections of the fixture as HOIDetections would hand them on, `per` images a batch (CPU tensors: the meter does not care)"""
    B = len(exp["det_off"]) - 1
    dets = [dict(scores=torch.from_numpy(exp["score"][lo:hi]), interactions=torch.from_numpy(exp["interaction"][lo:hi]).long(),
                 tp=torch.from_numpy(labels[lo:hi])) for lo, hi in zip(exp["det_off"][:-1], exp["det_off"][1:])]
    return [dets[i:i + per] for i in range(0, B, per)]


def test_restated_labels_are_the_reference_association(gold):
    g, case, exp = gold
    assert np.array_equal(exp["label"], g["labels"]) and exp["label"].sum() > 30


@pytest.mark.parametrize("algorithm", evaluation.ALGORITHMS)
@pytest.mark.parametrize("tag", ("plain", "num_gt"))
def test_ap_is_the_reference_meter(gold, algorithm, tag):
    g, case, exp = gold
    meter = evaluation.HOIEvaluator(int(g["num_classes"]), num_gt=list(g["num_gt"]) if tag == "num_gt" else None, algorithm=algorithm)
    for batch in batches(exp, g["labels"]):
        meter.append(batch)
    ap = meter.eval()
    want = g[f"ap_{algorithm}_{tag}"]
    assert ap.dtype == np.float64 and np.array_equal(ap, want), (ap, want)
    assert (want[-2:] == 0).all() and (want > 0).sum() >= 3          # two empty classes, and something to compare
    assert np.array_equal(meter.eval(), want)                         # evaluating again changes nothing


def test_num_gt_sanity_check(gold):
    g, case, exp = gold
    num_gt = list(g["num_gt"])
    c = int(np.argmax(np.bincount(exp["interaction"][g["labels"] > 0])))
    num_gt[c] = 1
    meter = evaluation.HOIEvaluator(int(g["num_classes"]), num_gt=num_gt)
    for batch in batches(exp, g["labels"]):
        meter.append(batch)
    with pytest.raises(AssertionError, match=f"Class {c}"):
        meter.eval()


def test_ties_go_to_the_earlier_append():
    """two detections of one class with the same score, the true positive appended second: the stable order keeps the false positive
    first (precision 0, then 1 / 2)"""
    meter = evaluation.HOIEvaluator(1, algorithm="11P")
    mk = lambda tp: [dict(scores=torch.tensor([0.5]), interactions=torch.tensor([0]), tp=torch.tensor([tp]))]      # noqa: E731
    meter.append(mk(0.0))
    meter.append(mk(1.0))
    assert meter.eval()[0] == pytest.approx(0.5)
    meter.reset()
    meter.append(mk(1.0))
    meter.append(mk(0.0))
    assert meter.eval()[0] == pytest.approx(1.0)


def test_meter_refusals():
    with pytest.raises(ValueError):
        evaluation.HOIEvaluator(3, algorithm="VOC")
    with pytest.raises(ValueError):
        evaluation.HOIEvaluator(3, num_gt=[1, 2])
    meter = evaluation.HOIEvaluator(3)
    with pytest.raises(ValueError, match="matched with targets"):
        meter.append([dict(scores=torch.zeros(1), labels=torch.zeros(1))])
    meter.append([dict(scores=torch.tensor([0.5]), interactions=torch.tensor([3]), tp=torch.tensor([1.0]))])
    with pytest.raises(ValueError, match="outside"):
        meter.eval()
    assert (evaluation.HOIEvaluator(3).eval() == 0).all()


def test_facade_refusals():
    """CPU tensors, gradient callers, logits from elsewhere, a conversion of the wrong shape"""
    det = evaluation.HOIDetections()
    logits, prior = torch.zeros(2, 4), torch.zeros(2, 2, 4)
    idx = torch.zeros(2, dtype=torch.int64)
    boxes = [torch.zeros(3, 4)]
    with pytest.raises(RuntimeError, match="HOIHead call returned"):
        det(([logits], [prior], [idx], [idx], [idx]), boxes)
    logits.hg_dense_scores = torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        det(([logits], [prior], [idx], [idx], [idx]), boxes)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="inference only"):
        det(([logits], [prior.clone().requires_grad_()], [idx], [idx], [idx]), boxes)
    with pytest.raises(ValueError, match="one entry per image"):
        det(([logits], [prior], [idx], [idx], [idx]), boxes + boxes)
    with pytest.raises(ValueError):
        evaluation.HOIDetections(gt_format=2)
    with pytest.raises(ValueError):
        evaluation.HOIDetections(conversion=[1, 2, 3])
    conv = evaluation.HOIDetections(conversion=[[0, None], [None, 1]]).conversion
    assert conv.dtype == torch.int32 and conv.tolist() == [[0, -1], [-1, 1]]
    assert evaluation.HOIDetections(conversion=torch.tensor([[0.0, float("nan")]])).conversion.tolist() == [[0, -1]]


def test_batch_tensor_is_found_again_or_rebuilt():
    """the per-image views of a HOIHead call lead back to its batch tensor; anything else is concatenated"""
    base = torch.arange(24.0).reshape(2, 6, 2).clone()
    views = [base[:, :2], base[:, 2:2], base[:, 2:]]
    assert evaluation._batch_of(views, 1).data_ptr() == base.data_ptr()
    swapped = [base[:, 2:], base[:, :2]]
    got = evaluation._batch_of(swapped, 1)
    assert got.data_ptr() != base.data_ptr() and torch.equal(got, torch.cat(swapped, 1))
    clones = [v.clone() for v in views]
    assert torch.equal(evaluation._batch_of(clones, 1), base)
    part = [base[:, :2], base[:, 2:4]]
    assert torch.equal(evaluation._batch_of(part, 1), base[:, :4])
