"""What follows the interaction head, for a whole batch in one call (``hg_hoi_detections``), and the evaluation meter behind it.

Counterpart of ``UPT.postprocessing`` (upt_tip_cache_model_free_finetune_distill3.py:1408-1427) and of the per-image body of ``test_hico``
(utils_tip_cache_and_union_finetune.py:376-409: ``conversion[objects, verbs]``, ``recover_boxes``, the per-class
``BoxPairAssociation(min_iou)`` loop) and of ``DetectionAPMeter`` (pocket/pocket/utils/meters.py:414-639):

    head = HOIHead(...)
    dets = HOIDetections(conversion, min_iou=0.5, obj2target=object_class_to_target_class)
    meter = HOIEvaluator(600, num_gt=dataset.anno_interaction)
    for images, targets in loader:
        out = head(feat_global, feat_local, image_sizes, region_props)        # (logits, prior, bh, bo, objects)
        meter.append(dets(out, boxes, targets))
    ap = meter.eval()

``HOIDetections`` without targets returns what ``HOIHead.postprocess`` returns, from one call and one device-to-host copy (``det_off`` and
the status) instead of a ``nonzero`` per image.  Inference only; CPU tensors and gradient callers raise ``RuntimeError`` (there is no CPU
fallback).  ``HOIEvaluator`` is host code on purpose: it runs once per evaluation.
"""
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .interaction import target_table

ALGORITHMS = ("AUC", "INT", "11P")


def _batch_of(views: Sequence[torch.Tensor], dim: int) -> torch.Tensor:
    """the batch tensor a HOIHead call cut ``views`` from along ``dim`` (they are its consecutive slices), or their concatenation"""
    base = views[0]._base
    if base is not None and base.is_contiguous() and all(v._base is base for v in views) and base.dim() == views[0].dim() and \
            base.shape[dim] == sum(v.shape[dim] for v in views):
        at = base.storage_offset()
        for v in views:      # consecutive slices, in order
            if v.storage_offset() != at or v.stride() != base.stride():
                break
            at += v.shape[dim] * base.stride(dim)
        else:
            return base
    return torch.cat(list(views), dim).contiguous()


class HOIDetections:
    """``HOIDetections(conversion=None, min_iou=0.5, gt_format=1, obj2target=None)``.

    ``conversion``: ``object_n_verb_to_interaction`` as ``[n_obj_classes, num_classes]`` (a nested list with ``None``, or an integer array /
    tensor with -1, where a combination has no interaction), or ``None`` when the interaction is the verb (``num_classes`` 600, :385-388).
    ``gt_format``: 1 = the targets' boxes are normalised (cx, cy, w, h), recovered as ``UPT.recover_boxes`` does; 0 = (x1, y1, x2, y2) in
    pixels.  ``obj2target``: the table the ``HOIHead`` was built with; it bounds the detections of a pair row by the largest number of
    targets an object class has (a prior is exactly 0 off them).  Without it the bound is ``num_classes`` a row."""

    def __init__(self, conversion=None, min_iou: float = 0.5, gt_format: int = 1, obj2target=None):
        if gt_format not in (0, 1):
            raise ValueError("gt_format is 0 (x1, y1, x2, y2 in pixels) or 1 (normalised cx, cy, w, h)")
        self.min_iou, self.gt_format = float(min_iou), int(gt_format)
        self.conversion = None
        if conversion is not None:
            if isinstance(conversion, torch.Tensor):
                c = conversion.detach().cpu().numpy()
            else:
                try:
                    c = np.asarray([[-1 if v is None else v for v in row] for row in conversion])
                except TypeError:
                    raise ValueError("conversion must be [n_obj_classes, num_classes]") from None
            c = np.where(np.isfinite(c.astype(np.float64)), c, -1)
            if c.ndim != 2:
                raise ValueError("conversion must be [n_obj_classes, num_classes]")
            self.conversion = torch.from_numpy(np.ascontiguousarray(c.astype(np.int32)))
        self.obj2target = obj2target
        self._per_row = None

    def _check(self, tensors):
        if torch.is_grad_enabled() and any(t.is_floating_point() and t.requires_grad for t in tensors):
            raise RuntimeError("hoigen_amd: HOIDetections is inference only (an input requires grad); call it under torch.no_grad() or "
                               "detach the inputs")
        if any(t.device.type != "cuda" for t in tensors):
            raise RuntimeError("hoigen_amd: HOIDetections runs only on a HIP device (there is no CPU fallback)")

    def __call__(self, head_outputs, boxes: List[torch.Tensor], targets: Optional[List[dict]] = None, image_sizes=None) -> List[dict]:
        """``head_outputs``: the five lists a ``HOIHead`` call returned; ``boxes``: the per-image boxes as ``postprocess`` takes them
        (in the head's order, humans first); ``targets``: per image ``boxes_h``, ``boxes_o`` ``[G, 4]``, ``hoi [G]`` and ``size`` = (h, w), as
        the loader delivers them (at most 256 ground-truth pairs an image).  -> the reference's list of detection dicts, views into the
        batch tensors: ``boxes``, ``pairing``, ``scores``, ``labels``, ``objects``, ``size`` (``image_sizes[b]`` if given, else the target's),
        and with targets ``interactions``, ``tp``, ``gt`` and ``max_iou``."""
        logits, prior, bh, bo, objects = head_outputs
        B = len(logits)
        if not (len(prior) == len(bh) == len(bo) == len(objects) == len(boxes) == B) or (targets is not None and len(targets) != B):
            raise ValueError("one entry per image in every list")
        dense = [getattr(lg, "hg_dense_scores", None) for lg in logits]
        if any(d is None for d in dense):
            raise RuntimeError("hoigen_amd: HOIDetections takes the logits tensors that a HOIHead call returned")
        self._check(list(prior) + dense + list(boxes))
        if B == 0:
            return []
        dev = prior[0].device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        NC = int(prior[0].shape[2])
        pair_off, box_off = [0], [0]
        for pr, bx in zip(prior, boxes):
            pair_off.append(pair_off[-1] + int(pr.shape[1]))
            box_off.append(box_off[-1] + int(bx.shape[0]))
        Pt = pair_off[-1]
        if self.conversion is not None:
            if self.conversion.shape[1] != NC:
                raise ValueError(f"conversion has {self.conversion.shape[1]} columns, the head {NC} classes")
            if self.conversion.device != dev:
                self.conversion = self.conversion.to(dev)
        if self._per_row is None:
            self._per_row = NC if self.obj2target is None else max(1, int(target_table(self.obj2target, NC).sum(1).max()))
        cap = Pt * min(self._per_row, NC)
        prior_b = _batch_of(prior, 1).detach()
        dense_b = _batch_of(dense, 0).detach()
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        cat32 = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).to(torch.int32) if Pt else torch.zeros(0, **i32)      # noqa: E731
        pair_h, pair_o, obj = cat32(bh), cat32(bo), cat32(objects)
        boxes_b = torch.cat([b.detach().reshape(-1, 4) for b in boxes]).float().contiguous()
        head = torch.empty(2 * B + 1, **i32)                   # det_off [B + 1] | status [B]: the one transfer of the call
        ints = torch.empty(7, max(cap, 1), **i32)              # pair, verb, h, o, object, interaction, gt
        flts = torch.empty(3, max(cap, 1), **f32)              # score, label, max_iou
        a = _lib.hg_hoi_detections_args()
        a.prior, a.scores, a.pair_h, a.pair_o, a.objects, a.boxes = (t.data_ptr() for t in (prior_b, dense_b, pair_h, pair_o, obj, boxes_b))
        I32 = _lib.C.c_int32
        pair_c, box_c = (I32 * (B + 1))(*pair_off), (I32 * (B + 1))(*box_off)
        a.pair_off, a.box_off, a.B, a.num_classes, a.cap = pair_c, box_c, B, NC, cap
        if self.conversion is not None:
            a.conversion, a.n_obj_classes = self.conversion.data_ptr(), self.conversion.shape[0]
        a.det_off, a.status = head.data_ptr(), head.data_ptr() + 4 * (B + 1)
        a.det_pair, a.det_verb, a.det_h, a.det_o, a.det_object, a.det_interaction = (ints[i].data_ptr() for i in range(6))
        a.det_score = flts[0].data_ptr()
        if targets is not None:
            gt_off, sizes = [0], []
            for t in targets:
                gt_off.append(gt_off[-1] + int(t["hoi"].numel()))
                sizes += [int(v) for v in t["size"]]
            gh = torch.cat([t["boxes_h"].detach().reshape(-1, 4) for t in targets]).to(device=dev, dtype=torch.float32).contiguous()
            go = torch.cat([t["boxes_o"].detach().reshape(-1, 4) for t in targets]).to(device=dev, dtype=torch.float32).contiguous()
            ghoi = torch.cat([t["hoi"].detach().reshape(-1) for t in targets]).to(device=dev, dtype=torch.int32).contiguous()
            gt_c, size_c = (I32 * (B + 1))(*gt_off), (I32 * (2 * B))(*sizes)
            a.gt_boxes_h, a.gt_boxes_o, a.gt_hoi, a.gt_off, a.gt_sizes = gh.data_ptr(), go.data_ptr(), ghoi.data_ptr(), gt_c, size_c
            a.gt_format, a.min_iou = self.gt_format, self.min_iou
            a.det_gt, a.det_label, a.det_max_iou = ints[6].data_ptr(), flts[1].data_ptr(), flts[2].data_ptr()
        with torch.cuda.device(idx):
            rc = _lib.lib().hg_hoi_detections(_lib.ctx(idx), _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
        _lib.check(idx, rc, "hg_hoi_detections")
        host = head.cpu().tolist()
        det_off, status = host[:B + 1], host[B + 1:]
        for b, st in enumerate(status):
            if st:
                why = [w for bit, w in ((1, "a detection whose (object, verb) has no interaction in the conversion table"),
                                        (2, "a non-finite ground-truth box"), (4, "more detections than the capacity")) if st & bit]
                raise RuntimeError(f"hoigen_amd: hg_hoi_detections: image {b}: " + "; ".join(why))
        n = det_off[-1]
        pairing = torch.stack([ints[2, :n], ints[3, :n]]).to(torch.int64)
        labels = ints[1, :n].to(torch.int64)
        objs = ints[4, :n].to(objects[0].dtype)
        interactions = ints[5, :n].to(torch.int64)
        sizes_out = image_sizes if image_sizes is not None else [t["size"] for t in targets] if targets is not None else [None] * B
        out = []
        for b in range(B):
            lo, hi = det_off[b], det_off[b + 1]
            d = dict(boxes=boxes[b], pairing=pairing[:, lo:hi], scores=flts[0, lo:hi], labels=labels[lo:hi], objects=objs[lo:hi], size=sizes_out[b])
            if targets is not None:
                d.update(interactions=interactions[lo:hi], tp=flts[1, lo:hi], gt=ints[6, lo:hi], max_iou=flts[2, lo:hi])
            out.append(d)
        return out


def _linspace11():
    """torch.linspace(0, 1, 11, dtype=float64) as torch computes it: from the start in the first half, from the end in the second"""
    step = 1.0 / 10
    return [0.0 + step * i if i < 5 else 1.0 - step * (10 - i) for i in range(11)]


def precision_recall(output: np.ndarray, labels: np.ndarray, num_gt=None):
    """``DetectionAPMeter.compute_pr_for_each`` (meters.py:560-583) in float64; the order is a STABLE descending sort - ties go to the
    earlier append, which the reference's ``argsort(descending=True)`` leaves open"""
    order = np.argsort(-output, kind="stable")
    tp = labels[order]
    fp = 1 - tp
    tp, fp = np.cumsum(tp), np.cumsum(fp)
    prec = tp / (tp + fp)
    denom = float(labels.sum()) if num_gt is None else num_gt
    rec = np.zeros_like(tp) if denom == 0 else tp / denom
    return prec, rec


def ap_auc(prec, rec):
    """meters.py:207-227, index for index (``rec[idx - 1]`` at idx 0 is the last recall, as there)"""
    ap, max_rec = 0.0, rec[-1]
    for i in range(len(prec)):
        if rec[i] >= max_rec:
            break
        d_x = rec[i] - rec[i - 1]
        if d_x == 0:
            continue
        ap += prec[i] * rec[i] if i == 0 else 0.5 * (prec[i] + prec[i - 1]) * d_x
    return ap


def ap_int(prec, rec):
    """meters.py:229-252"""
    ap, max_rec = 0.0, rec[-1]
    for i in range(len(prec)):
        if rec[i] >= max_rec:
            break
        d_x = rec[i] - rec[i - 1]
        if d_x == 0:
            continue
        max_ = prec[i:].max()
        ap += max_ * rec[i] if i == 0 else 0.5 * (max_ + max(prec[i - 1], max_)) * d_x
    return ap


def ap_11p(prec, rec):
    """meters.py:254-269"""
    ap = 0.0
    for t in _linspace11():
        inds = rec >= t
        if inds.any():
            ap += prec[inds].max() / 11
    return ap


_AP = {"AUC": ap_auc, "INT": ap_int, "11P": ap_11p}


class HOIEvaluator:
    """``HOIEvaluator(num_classes, num_gt=None, algorithm='11P')``: ``DetectionAPMeter`` (``nproc = 1``) behind ``HOIDetections``.

    ``append(dets)`` keeps the batch's ``(score, interaction, tp)`` where they are (on the device) and transfers nothing; ``eval()`` brings
    everything appended since the last ``eval()`` to the host in one copy and returns the per-class AP as float64 ``[num_classes]`` over all
    that was ever appended (``reset()`` starts over)."""

    def __init__(self, num_classes: int, num_gt=None, algorithm: str = "11P"):
        if algorithm not in ALGORITHMS:
            raise ValueError(f"unknown algorithm {algorithm!r}; one of {ALGORITHMS}")
        if num_gt is not None and len(num_gt) != num_classes:
            raise ValueError("num_gt must have one entry per class")
        self.num_classes, self.algorithm = int(num_classes), algorithm
        self.num_gt = None if num_gt is None else [float(v) for v in num_gt]
        self.reset()

    def reset(self):
        self._pending: List[torch.Tensor] = []
        self._host = np.zeros((3, 0), np.float64)

    def append(self, dets: List[dict]) -> None:
        for d in dets:
            if "tp" not in d or "interactions" not in d:
                raise ValueError("hoigen_amd: HOIEvaluator.append takes detections that HOIDetections matched with targets")
            if d["scores"].numel():
                self._pending.append(torch.stack([d["scores"].detach().to(torch.float64), d["interactions"].detach().to(torch.float64),
                                                  d["tp"].detach().to(torch.float64)]))

    def collected(self) -> np.ndarray:
        """float64 ``[3, n]`` = score, interaction, tp of everything appended, in the order of the appends"""
        if self._pending:
            self._host = np.concatenate([self._host, torch.cat(self._pending, 1).cpu().numpy()], 1)
            self._pending = []
        return self._host

    def eval(self) -> np.ndarray:
        score, inter, tp = self.collected()
        inter = inter.astype(np.int64)
        if inter.size and (inter.min() < 0 or inter.max() >= self.num_classes):
            raise ValueError(f"an interaction outside 0 .. {self.num_classes - 1}")
        order = np.argsort(inter, kind="stable")
        bounds = np.searchsorted(inter[order], np.arange(self.num_classes + 1))
        ap = np.zeros(self.num_classes, np.float64)
        self.max_rec = np.zeros(self.num_classes, np.float64)
        for c in range(self.num_classes):
            sel = order[bounds[c]:bounds[c + 1]]
            out, lab = score[sel], tp[sel]
            n_gt = None if self.num_gt is None else self.num_gt[c]
            if n_gt is not None and lab.sum() > n_gt:      # the sanity check of meters.py:549-551
                raise AssertionError(f"Class {c}: number of true positives larger than that of ground truth")
            if len(out):
                prec, rec = precision_recall(out, lab, n_gt)
                ap[c], self.max_rec[c] = _AP[self.algorithm](prec, rec), rec[-1]
        self.ap = ap
        return ap
