#!/usr/bin/env python3
"""Generates tests/golden/g16_hoi_detections.npz by executing the reference's own BoxPairAssociation
(pocket/pocket/utils/association.py:17-116) and DetectionAPMeter (pocket/pocket/utils/meters.py:414-639, nproc = 1) on seeded inputs:

    python tests/golden/make_golden_detections.py --reference DIR          (DIR = a checkout of the reference; or $HG_REFERENCE)

The two files are loaded by path under a stand-in package, because the pocket package itself cannot be imported (it needs torchvision,
which is not installed): `..ops` is a stub with
  box_iou     torchvision's formula written out here - area = (x2 - x1) * (y2 - y1), inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2)
              - max(y1), 0), iou = inter / (area_1[:, None] + area_2 - inter) - so the IoU of this fixture is pinned to the restatement
              and to the hand-derived answers of detections_bound.constructed(), NOT to the real library (README_detections.md)
  to_tensor   never called on this path (the meter starts empty).
The loop around the association is test_hico's (utils_tip_cache_and_union_finetune.py:394-409), typed out in this script's own words
on detections_bound's compacted detections.  Inputs: six images of detections_bound.random_case (30 pairs, 6 verbs, 12 ground-truth pairs,
pixel boxes, interaction = verb), appended as three batches of two; 8 classes, so that two classes stay empty; scores without ties.
The fixture holds data only: the case's arrays, the labels, and the APs of the three algorithms with and without num_gt."""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import detections_bound as db  # noqa: E402

NUM_CLASSES = 8
CASE = dict(seed=16, NC=6, pairs=(30,) * 6, gts=(12,) * 6)
ALGORITHMS = ("AUC", "INT", "11P")


def box_iou(boxes_1, boxes_2, encoding="coord"):
    assert encoding == "coord"
    a1 = (boxes_1[:, 2] - boxes_1[:, 0]) * (boxes_1[:, 3] - boxes_1[:, 1])
    a2 = (boxes_2[:, 2] - boxes_2[:, 0]) * (boxes_2[:, 3] - boxes_2[:, 1])
    lt = torch.max(boxes_1[:, None, :2], boxes_2[:, :2])
    rb = torch.min(boxes_1[:, None, 2:], boxes_2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (a1[:, None] + a2 - inter)


def load_reference(root):
    def to_tensor(*a, **k):
        raise NotImplementedError("the stub of pocket.ops.to_tensor: not on this path")

    pkg, utils, ops = types.ModuleType("pocket_ref"), types.ModuleType("pocket_ref.utils"), types.ModuleType("pocket_ref.ops")
    pkg.__path__, utils.__path__ = [], []
    ops.box_iou, ops.to_tensor = box_iou, to_tensor
    sys.modules.update({"pocket_ref": pkg, "pocket_ref.utils": utils, "pocket_ref.ops": ops})
    mods = {}
    for name in ("association", "meters"):
        spec = importlib.util.spec_from_file_location(f"pocket_ref.utils.{name}", os.path.join(root, "pocket", "pocket", "utils", f"{name}.py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["association"].BoxPairAssociation, mods["meters"].DetectionAPMeter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HG_REFERENCE"))
    o = ap.parse_args()
    assert o.reference, "--reference DIR or $HG_REFERENCE"
    BoxPairAssociation, DetectionAPMeter = load_reference(o.reference)
    case = db.random_case(**CASE)
    ent = db.compact(case)
    associate = BoxPairAssociation(min_iou=0.5)
    per_image = []
    for b in range(case["B"]):
        lo, hi = ent["det_off"][b], ent["det_off"][b + 1]
        bx = torch.from_numpy(case["boxes"][case["box_off"][b]:case["box_off"][b + 1]])
        boxes_h, boxes_o = bx[torch.from_numpy(ent["h"][lo:hi]).long()], bx[torch.from_numpy(ent["o"][lo:hi]).long()]
        scores, interactions = torch.from_numpy(ent["score"][lo:hi]), torch.from_numpy(ent["interaction"][lo:hi]).long()
        assert len(scores.unique()) == len(scores), "score ties"
        g0, g1 = case["gt_off"][b], case["gt_off"][b + 1]
        gt_h, gt_o, hoi = torch.from_numpy(case["gt_h"][g0:g1]), torch.from_numpy(case["gt_o"][g0:g1]), torch.from_numpy(case["gt_hoi"][g0:g1]).long()
        labels = torch.zeros_like(scores)
        for cls in interactions.unique():
            gt_idx = torch.nonzero(hoi == cls).squeeze(1)
            det_idx = torch.nonzero(interactions == cls).squeeze(1)
            if len(gt_idx):
                labels[det_idx] = associate((gt_h[gt_idx].view(-1, 4), gt_o[gt_idx].view(-1, 4)), (boxes_h[det_idx].view(-1, 4), boxes_o[det_idx].view(-1, 4)),
                                            scores[det_idx].view(-1))
        per_image.append((scores, interactions, labels))
    labels_all = torch.cat([p[2] for p in per_image]).numpy()
    n_tp = np.bincount(torch.cat([p[1] for p in per_image]).numpy()[labels_all > 0], minlength=NUM_CLASSES)
    num_gt = (np.maximum(n_tp, 1) + np.arange(NUM_CLASSES) % 3).astype(np.int64)      # >= the true positives; 10-ths and 11-ths among the recalls
    out = {k: v for k, v in case.items() if isinstance(v, np.ndarray)}
    out.update(B=np.int64(case["B"]), NC=np.int64(case["NC"]), gt_format=np.int64(case["gt_format"]), min_iou=np.float32(case["min_iou"]))
    out.update(labels=labels_all, num_gt=num_gt, num_classes=np.int64(NUM_CLASSES))
    for alg in ALGORITHMS:
        for tag, ngt in (("plain", None), ("num_gt", [int(v) for v in num_gt])):
            meter = DetectionAPMeter(NUM_CLASSES, nproc=1, num_gt=ngt, algorithm=alg)
            for i in range(0, len(per_image), 2):       # three batches of two images
                for s, c, l in per_image[i:i + 2]:
                    meter.append(s, c, l)
            with contextlib.redirect_stdout(io.StringIO()):      # (the empty classes print a warning)
                out[f"ap_{alg}_{tag}"] = meter.eval().numpy().astype(np.float64)
    path = os.path.join(HERE, "g16_hoi_detections.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", int(labels_all.sum()), "true positives of", len(labels_all),
          "; mAP 11P", float(out["ap_11P_plain"].mean()))


if __name__ == "__main__":
    main()
