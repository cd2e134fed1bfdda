#!/usr/bin/env python3
"""Generates tests/golden/g15_region_props.npz by executing the reference's own statements
(upt_tip_cache_model_free_finetune_distill3.py): the MLP class (:40-52), prepare_region_proposals (:1361-1406) and get_prior (from :1445
to the end of the function; run with prior_method 0, prior_type 'cbe') on the seeded inputs of region_props_cases.py.  The file cannot be
imported (it needs pocket, torchvision, detr ...), so the statements are read from the reference tree at run time and exec'd with a
stand-in `self` that only carries what they touch; nothing of their text is stored.  `batched_nms` is bound to tests/props_bound.py's
restatement: there is no torchvision to import (README_region_props.md), so that one step stays pinned to the restatement and to the
hand-derived known answers only.  Run in the build container:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_region_props.py
"""
import contextlib
import io
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F_
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import props_bound as pb  # noqa: E402
import region_props_cases as rc  # noqa: E402

REF = "/root/reference/upt_tip_cache_model_free_finetune_distill3.py"


def lines(src, first, last):
    return textwrap.dedent("\n".join(src[first - 1:last]))


def batched_nms(boxes, scores, idxs, iou_threshold):
    return torch.from_numpy(pb.nms(scores.numpy(), idxs.numpy(), boxes.numpy(), iou_threshold))


def main():
    src = open(REF).read().split("\n")
    assert src[39].startswith("class MLP(") and src[1360].lstrip().startswith("def prepare_region_proposals(") and src[1444].lstrip().startswith("def get_prior(")
    end = next(i for i in range(1445, len(src)) if src[i].startswith("    def "))      # the next method
    ns = dict(torch=torch, nn=nn, F=F_, batched_nms=batched_nms)
    exec(lines(src, 40, 52), ns)
    exec(lines(src, 1361, 1406), ns)
    exec(lines(src, 1445, end), ns)
    case, w = rc.case(), rc.weights()
    mlp = ns["MLP"](rc.E + 5, rc.HIDDEN, rc.OUT, 3)
    with torch.no_grad():
        for i in range(3):
            mlp.layers[i].weight.copy_(torch.from_numpy(w[f"w{i}"]))
            mlp.layers[i].bias.copy_(torch.from_numpy(w[f"b{i}"]))
    p = rc.PARAMS
    self = types.SimpleNamespace(box_score_thresh=p["box_score_thresh"], human_idx=p["human_idx"], min_instances=p["min_instances"],
                                 max_instances=p["max_instances"], priors_initial_dim=rc.E + 5, visual_output_dim=rc.E, prior_type="cbe",
                                 obj_affordance=False, object_embedding=torch.from_numpy(w["emb"]), priors_downproj=mlp)
    results = []
    for b in range(case["B"]):
        lo, hi = case["q_off"][b], case["q_off"][b + 1]
        results.append(dict(scores=torch.from_numpy(case["scores"][lo:hi]), labels=torch.from_numpy(case["labels"][lo:hi]),
                            boxes=torch.from_numpy(case["boxes"][lo:hi])))
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        region_props = ns["prepare_region_proposals"](self, results)
        priors, mask = ns["get_prior"](self, region_props, torch.from_numpy(case["image_sizes"]), 0)
    out = dict(priors=priors.numpy(), mask=mask.numpy())
    for b, rp in enumerate(region_props):
        for k in ("boxes", "scores", "labels"):
            out[f"{k}_{b}"] = rp[k].numpy()
    path = os.path.join(HERE, "g15_region_props.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", [len(rp["scores"]) for rp in region_props])


if __name__ == "__main__":
    main()
