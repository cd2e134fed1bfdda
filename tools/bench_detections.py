#!/usr/bin/env python
"""Time hg_hoi_detections (one call per batch) against the per-image loop it replaces.

    python tools/bench_detections.py [--reps 60] [--out profiles/detections.txt]

one call  hoigen_amd.evaluation.HOIDetections with targets: the concatenations, the copy of the ground truth to the device,
          hg_hoi_detections, the one device-to-host copy of det_off and the status, the dicts
loop      what exists without it: HOIHead.postprocess (a nonzero and five gathers per image), then test_hico's per-image body restated
          in torch as the reference runs it - every tensor of the image to the CPU, conversion[objects, verbs], recover_boxes, the
          per-class loop with BoxPairAssociation's statements on a box_iou written from torchvision's formula.  The meter's append is
          left out of both legs.
compact   the C call without ground truth (det_count + det_scan + det_write), no host copy
full      the C call with ground truth (+ det_assoc), no host copy; assoc = the difference

Device events around each leg, legs alternating, median and minimum over --reps rounds after 5 warm-up rounds.  Cases: the six head sizes
of DESIGN.md §11's table (B = 4 and 8; 6, 12 and 30 boxes an image, half of them humans: 15, 66 and 435 pairs an image), 117 verbs, 80
object classes with 12 target verbs each, a conversion table to 960 interactions, 5 and 20 ground-truth pairs an image in normalised
(cx, cy, w, h) (tests/detections_bound.random_case)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import detections_bound as db                        # noqa: E402
from hoigen_amd import _lib, evaluation, interaction   # noqa: E402

NC, N_OBJ, TARGETS = 117, 80, 12


def timed(legs, reps, warmup=5):
    out = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[k].append(a.elapsed_time(b))
    return out


def box_iou(b1, b2):
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (a1[:, None] + a2 - inter)


def associate(gt, det, scores, min_iou):
    """BoxPairAssociation.__call__ in its own order of statements"""
    iou = torch.min(box_iou(gt[0], det[0]), box_iou(gt[1], det[1]))
    max_iou, max_idx = iou.max(0)
    match = torch.zeros_like(iou)
    match[max_idx, torch.arange(iou.shape[1])] = max_iou
    match = match > min_iou
    labels = torch.zeros_like(scores)
    for m in match:
        match_idx = torch.nonzero(m).squeeze(1)
        if len(match_idx) == 0:
            continue
        labels[match_idx[scores[match_idx].argmax()]] = 1
    return labels


def recover_boxes(boxes, size):
    cx, cy, w, h = boxes.unbind(-1)
    b = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)
    ih, iw = size
    return b * torch.stack([iw, ih, iw, ih])


def make_case(B, n, G, dev):
    n_h = n // 2
    case = db.random_case(seed=B * 1000 + n * 10 + G, NC=NC, pairs=(n_h * (n - 1),) * B, gts=(G,) * B, gt_format=1, n_obj=N_OBJ, targets=TARGETS)
    t = lambda k, dt=None: torch.from_numpy(case[k] if dt is None else case[k].astype(dt)).to(dev)      # noqa: E731
    pair_off = [int(v) for v in case["pair_off"]]
    logits, prior, dense = torch.zeros(pair_off[-1], NC, device=dev), t("prior"), t("scores")
    out = interaction.split_outputs(pair_off, logits, prior, t("pair_h"), t("pair_o"), t("objects"))
    for b, lg in enumerate(out[0]):
        lg.hg_dense_scores = dense[pair_off[b]:pair_off[b + 1]]
    boxes = [t("boxes")[case["box_off"][b]:case["box_off"][b + 1]] for b in range(B)]
    targets = []
    for b in range(B):
        lo, hi = case["gt_off"][b], case["gt_off"][b + 1]
        targets.append(dict(boxes_h=torch.from_numpy(case["gt_h"][lo:hi]), boxes_o=torch.from_numpy(case["gt_o"][lo:hi]),
                            hoi=torch.from_numpy(case["gt_hoi"][lo:hi].astype(np.int64)), size=torch.from_numpy(case["gt_sizes"][b].astype(np.int64))))
    o2t = torch.from_numpy((case["conversion"] >= 0).astype(np.uint8))
    return case, out, boxes, targets, o2t


def loop_leg(case, out, boxes, targets):
    logits, prior, bh, bo, objects = out
    conversion = torch.from_numpy(np.where(case["conversion"] >= 0, case["conversion"], np.nan).astype(float))
    sizes = [t["size"] for t in targets]

    def loop():
        detections = interaction.HOIHead.postprocess(None, boxes, bh, bo, logits, prior, objects, sizes)
        all_labels = []
        for output, target in zip(detections, targets):
            output = {k: v.cpu() for k, v in output.items()}
            bx = output["boxes"]
            boxes_h, boxes_o = bx[output["pairing"]].unbind(0)
            scores, verbs = output["scores"], output["labels"]
            interactions = conversion[output["objects"], verbs]
            gt_bx_h, gt_bx_o = recover_boxes(target["boxes_h"], target["size"]), recover_boxes(target["boxes_o"], target["size"])
            labels = torch.zeros_like(scores)
            for hoi_idx in interactions.unique():
                gt_idx = torch.nonzero(target["hoi"] == hoi_idx).squeeze(1)
                det_idx = torch.nonzero(interactions == hoi_idx).squeeze(1)
                if len(gt_idx):
                    labels[det_idx] = associate((gt_bx_h[gt_idx].view(-1, 4), gt_bx_o[gt_idx].view(-1, 4)),
                                                (boxes_h[det_idx].view(-1, 4), boxes_o[det_idx].view(-1, 4)), scores[det_idx].view(-1), 0.5)
            all_labels.append(labels)
        return all_labels

    return loop


def c_leg(case, dev, assoc):
    """the raw C call on preallocated buffers (no host copy)"""
    B, cap = case["B"], int(case["pair_off"][-1]) * TARGETS
    t = lambda k, dt=None: torch.from_numpy(np.ascontiguousarray(case[k] if dt is None else case[k].astype(dt))).to(dev)      # noqa: E731
    ins = [t("prior"), t("scores"), t("pair_h"), t("pair_o"), t("objects"), t("boxes"), t("conversion"), t("gt_h"), t("gt_o"), t("gt_hoi")]
    ints, flts, head = torch.empty(7, cap, dtype=torch.int32, device=dev), torch.empty(3, cap, device=dev), torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
    a = _lib.hg_hoi_detections_args()
    a.prior, a.scores, a.pair_h, a.pair_o, a.objects, a.boxes, a.conversion, a.gt_boxes_h, a.gt_boxes_o, a.gt_hoi = (x.data_ptr() for x in ins)
    I32 = _lib.C.c_int32
    hostv = [(I32 * (B + 1))(*[int(v) for v in case[k]]) for k in ("pair_off", "box_off", "gt_off")] + [(I32 * (2 * B))(*[int(v) for v in case["gt_sizes"].reshape(-1)])]
    a.pair_off, a.box_off, a.B, a.num_classes, a.n_obj_classes, a.cap = hostv[0], hostv[1], B, NC, N_OBJ, cap
    a.det_off, a.status = head.data_ptr(), head.data_ptr() + 4 * (B + 1)
    a.det_pair, a.det_verb, a.det_h, a.det_o, a.det_object, a.det_interaction = (ints[i].data_ptr() for i in range(6))
    a.det_score = flts[0].data_ptr()
    if assoc:
        a.gt_off, a.gt_sizes, a.gt_format, a.min_iou = hostv[2], hostv[3], 1, 0.5
        a.det_gt, a.det_label, a.det_max_iou = ints[6].data_ptr(), flts[1].data_ptr(), flts[2].data_ptr()
    lib, ctx = _lib.lib(), _lib.ctx(0)

    def run(keep=(ins, ints, flts, head, hostv)):
        rc = lib.hg_hoi_detections(ctx, _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.hg_last_error(ctx)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    assert o.reps >= 50, "median of at least 50"
    dev = torch.device("cuda:0")
    lines = [f"hg_hoi_detections against HOIHead.postprocess + the per-image association on the CPU: median (min) of {o.reps} alternating rounds; "
             f"{NC} verbs, {N_OBJ} object classes, {TARGETS} targets each",
             f"{'B':>2} {'pairs':>6} {'dets':>6} {'gt/img':>6} {'TP':>4} | {'one call ms':>17} {'loop ms':>19} {'loop/call':>9} | {'compact us':>15} {'full us':>15} {'assoc us':>8}"]
    for B in (4, 8):
        for n in (6, 12, 30):
            for G in (5, 20):
                case, out, boxes, targets, o2t = make_case(B, n, G, dev)
                conv = torch.from_numpy(case["conversion"])
                call = evaluation.HOIDetections(conv, min_iou=0.5, gt_format=1, obj2target=o2t)
                loop = loop_leg(case, out, boxes, targets)
                # the two legs agree before they are timed
                got, want = call(out, boxes, targets), loop()
                assert all(torch.equal(g["tp"].cpu(), w) for g, w in zip(got, want))
                n_det, n_tp = sum(len(g["tp"]) for g in got), int(sum(float(w.sum()) for w in want))
                tm = timed({"call": lambda: call(out, boxes, targets), "loop": loop}, o.reps)
                tk = timed({"compact": c_leg(case, dev, False), "full": c_leg(case, dev, True)}, o.reps)
                med = {k: statistics.median(v) for k, v in {**tm, **tk}.items()}
                mn = {k: min(v) for k, v in {**tm, **tk}.items()}
                lines.append(f"{B:>2} {int(case['pair_off'][-1]):>6} {n_det:>6} {G:>6} {n_tp:>4} | {med['call']:8.3f} ({mn['call']:6.3f}) "
                             f"{med['loop']:9.3f} ({mn['loop']:7.3f}) {med['loop'] / med['call']:>9.1f} | "
                             f"{1e3 * med['compact']:7.1f} ({1e3 * mn['compact']:5.1f}) {1e3 * med['full']:7.1f} ({1e3 * mn['full']:5.1f}) "
                             f"{1e3 * (med['full'] - med['compact']):>8.1f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
