"""Region proposals and instance priors for a whole batch in one call (``hg_region_priors``).

Counterpart of ``UPT.prepare_region_proposals`` (upt_tip_cache_model_free_finetune_distill3.py:1361-1406), ``get_prior`` with
``prior_type 'cbe'``, ``prior_method 0`` (:1445-1495) and ``priors_downproj`` (``MLP(E + 5, 128, 64, 3)``, :40-52, :520):

    proposals = RegionProposals(human_idx, box_score_thresh=0.2, min_instances=3, max_instances=15)
    priors = InstancePriors(upt.priors_downproj, upt.object_embedding)
    front = DetectorFrontEnd(proposals, priors)
    region_props, (priors, mask) = front(results, image_sizes)        # results: what DETR's PostProcess returned

``region_props`` is the reference's list of dicts (``boxes [n, 4]``, ``scores [n]``, ``labels [n]`` in the labels' own dtype), humans
first, each kind by descending score; ``priors [B, max_n, 64]`` and the bool ``mask [B, max_n]`` (True = pad) are what ``get_prior``
returns and ``visual(x, (priors, mask))`` consumes.  Ties between scores go to the lower input index (the reference's unstable
``argsort`` leaves them open).  The class-aware NMS is torchvision's coordinate trick in its own fp32 arithmetic (there is no
torchvision to call).

One device-to-host copy per call - the B counts and statuses, which the list lengths and ``max_n`` need - and no other
synchronisation; pass ``image_sizes`` as a host tensor or a sequence of ``(h, w)`` (a device tensor costs a second copy).  An image with
a non-finite score or coordinate raises ``RuntimeError`` naming it.  Inference only; CPU tensors and gradient callers raise
``RuntimeError`` (there is no CPU fallback).  Out of scope: ``PostProcess``, ``prior_method`` 1 and 2, ``obj_affordance``, the other
``prior_type`` strings, ``batched_nms``' per-class path above 4 000 boxes (an image has at most 512 detections here).
"""
import threading
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

MAX_IMAGES, MAX_DETECTIONS, MAX_ROWS, OUT_DIM = 64, 512, 64, 64      # include/hoigen_amd.h
_free = list(range(_lib.HG_MAX_PRIOR_SLOTS))
_lock = threading.Lock()


class RegionProposals:
    """The thresholds of ``prepare_region_proposals`` (:1361-1406; the NMS threshold is the reference's literal 0.5)."""

    def __init__(self, human_idx: int, box_score_thresh: float = 0.2, min_instances: int = 3, max_instances: int = 15,
                 nms_thresh: float = 0.5):
        self.human_idx, self.box_score_thresh, self.nms_thresh = int(human_idx), float(box_score_thresh), float(nms_thresh)
        self.min_instances, self.max_instances = int(min_instances), int(max_instances)
        if not 0 <= self.min_instances <= self.max_instances or not 1 <= self.max_instances <= MAX_ROWS // 2:
            raise ValueError(f"0 <= min_instances <= max_instances and 1 <= max_instances <= {MAX_ROWS // 2} "
                             f"(got {min_instances}, {max_instances})")

    @property
    def cap(self) -> int:
        return 2 * self.max_instances


def _mlp_tensors(mlp):
    """(w0, b0, w1, b1, w2, b2) of the reference's ``MLP`` module (``.layers``) or of its state dict (``layers.{i}.weight`` ...)"""
    sd = mlp if isinstance(mlp, dict) else mlp.state_dict()
    try:
        t = [sd[f"layers.{i}.{k}"] for i in range(3) for k in ("weight", "bias")]
    except KeyError as e:
        raise ValueError(f"priors_downproj must have the three linears layers.0 .. layers.2 (missing {e})") from None
    if any(k.startswith("layers.3.") for k in sd):
        raise ValueError("priors_downproj must have exactly three linears")
    return t


class InstancePriors:
    """``InstancePriors(priors_downproj, object_embedding)``: the reference's ``MLP`` module or its state dict, and
    ``object_embedding [n_obj_classes, E]``.  The tensors are copied into the native context at construction, with the label-dependent
    part of the first layer folded into a table; call ``update()`` after a training step changed them (with no arguments: from the
    module and the embedding given at construction)."""

    def __init__(self, priors_downproj, object_embedding: torch.Tensor):
        with _lock:
            if not _free:
                raise RuntimeError(f"hoigen_amd: all {_lib.HG_MAX_PRIOR_SLOTS} prior slots are in use; close() or delete an "
                                   "InstancePriors first")
            self.slot = _free.pop(0)
        self._mlp, self._emb = priors_downproj, object_embedding
        try:
            self.update()
        except Exception:
            self.close()
            raise

    def close(self):
        with _lock:
            if getattr(self, "slot", None) is not None:
                _free.append(self.slot)
                _free.sort()
                self.slot = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def update(self, priors_downproj=None, object_embedding: Optional[torch.Tensor] = None):
        if self.slot is None:
            raise RuntimeError("hoigen_amd: this InstancePriors has been closed")
        if priors_downproj is not None:
            self._mlp = priors_downproj
        if object_embedding is not None:
            self._emb = object_embedding
        w0, b0, w1, b1, w2, b2 = _mlp_tensors(self._mlp)
        emb = self._emb
        if emb.dim() != 2 or w0.dim() != 2 or w0.shape[1] != emb.shape[1] + 5:
            raise ValueError(f"the first linear takes E + 5 columns (prior_type 'cbe'): weight {tuple(w0.shape)}, "
                             f"object_embedding {tuple(emb.shape)}")
        hid = w0.shape[0]
        if tuple(w1.shape) != (hid, hid) or tuple(w2.shape) != (OUT_DIM, hid):
            raise ValueError(f"priors_downproj must be MLP(E + 5, hidden, {OUT_DIM}, 3): weights {tuple(w0.shape)}, {tuple(w1.shape)}, "
                             f"{tuple(w2.shape)}")
        if emb.device.type != "cuda" or any(t.device != emb.device for t in (w0, b0, w1, b1, w2, b2)):
            raise RuntimeError("hoigen_amd: InstancePriors runs only on a HIP device (there is no CPU fallback); priors_downproj and "
                               "object_embedding must live on the same one")
        self.device = emb.device.index if emb.device.index is not None else torch.cuda.current_device()
        self.E, self.hidden, self.n_obj_classes = int(emb.shape[1]), int(hid), int(emb.shape[0])
        keep = [t.detach().float().contiguous() for t in (w0, b0, w1, b1, w2, b2, emb)]
        w = _lib.hg_prior_weights()
        w.E, w.hidden, w.out, w.n_obj_classes = self.E, self.hidden, OUT_DIM, self.n_obj_classes
        w.w0, w.b0, w.w1, w.b1, w.w2, w.b2, w.object_embedding = (_lib.tensor(t) for t in keep)
        with torch.cuda.device(self.device):
            rc = _lib.lib().hg_load_priors(_lib.ctx(self.device), self.slot, _lib.C.byref(w))
        _lib.check(self.device, rc, "hg_load_priors")


def host_sizes(image_sizes, B: int) -> List[float]:
    """``image_sizes`` ([B, 2] tensor or a sequence of (h, w)) as 2 B host floats"""
    t = image_sizes.detach().cpu() if isinstance(image_sizes, torch.Tensor) else torch.as_tensor(image_sizes)
    t = t.to(torch.float32).reshape(-1, 2)
    if t.shape[0] != B:
        raise ValueError(f"image_sizes must be [B, 2] = (h, w) per image, B = {B} (got {tuple(t.shape)})")
    return t.reshape(-1).tolist()


def split_region_props(counts, boxes, scores, labels, label_dtype) -> List[dict]:
    """the padded ``[B, cap]`` outputs as the reference's list of dicts; ``counts`` on the host.  The dicts also carry ``n_human``
    (a host int), which a ``HOIHead`` reads instead of transferring the labels."""
    out = []
    for b, row in enumerate(counts):
        n = int(row[0])
        out.append(dict(boxes=boxes[b, :n], scores=scores[b, :n], labels=labels[b, :n].to(label_dtype), n_human=int(row[1])))
    return out


class DetectorFrontEnd:
    """``region_props, (priors, mask) = DetectorFrontEnd(proposals, priors)(results, image_sizes)``; with ``priors=None`` the call
    returns ``region_props, None`` (proposals only)."""

    def __init__(self, proposals: RegionProposals, priors: Optional[InstancePriors] = None):
        if not isinstance(proposals, RegionProposals):
            raise TypeError("proposals must be a hoigen_amd.proposals.RegionProposals")
        if priors is not None and not isinstance(priors, InstancePriors):
            raise TypeError("priors must be a hoigen_amd.proposals.InstancePriors or None")
        self.proposals, self.priors = proposals, priors

    @staticmethod
    def _check(results: Sequence[dict]):
        tensors = [r[k] for r in results for k in ("scores", "labels", "boxes")]
        if torch.is_grad_enabled() and any(t.is_floating_point() and t.requires_grad for t in tensors):
            raise RuntimeError("hoigen_amd: DetectorFrontEnd is inference only (an input requires grad); call it under torch.no_grad() "
                               "or detach the inputs")
        if any(t.device.type != "cuda" for t in tensors):
            raise RuntimeError("hoigen_amd: DetectorFrontEnd runs only on a HIP device (there is no CPU fallback)")

    def __call__(self, results: Sequence[dict], image_sizes) -> Tuple[List[dict], Optional[Tuple[torch.Tensor, torch.Tensor]]]:
        self._check(results)
        B = len(results)
        if B == 0:
            return [], None
        if B > MAX_IMAGES:
            raise ValueError(f"at most {MAX_IMAGES} images a call (got {B})")
        p, pri = self.proposals, self.priors
        if pri is not None and pri.slot is None:
            raise RuntimeError("hoigen_amd: the InstancePriors has been closed")
        sizes = [int(r["scores"].numel()) for r in results]
        if max(sizes) > MAX_DETECTIONS:
            raise ValueError(f"at most {MAX_DETECTIONS} detections an image (got {max(sizes)})")
        for r, q in zip(results, sizes):
            if r["labels"].numel() != q or r["boxes"].numel() != 4 * q:
                raise ValueError("scores [Q], labels [Q] and boxes [Q, 4] of an image must agree")
        dev = results[0]["scores"].device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        if pri is not None and pri.device != idx:
            raise RuntimeError("the results are on a different device than the InstancePriors")
        label_dtype = results[0]["labels"].dtype
        scores = torch.cat([r["scores"].detach().reshape(-1) for r in results]).float().contiguous()
        labels = torch.cat([r["labels"].detach().reshape(-1) for r in results]).to(torch.int32).contiguous()
        boxes = torch.cat([r["boxes"].detach().reshape(-1, 4) for r in results]).float().contiguous()
        cap = p.cap
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        counts, keep, out_labels = torch.empty(B, 4, **i32), torch.empty(B, cap, **i32), torch.empty(B, cap, **i32)
        out_boxes, out_scores = torch.empty(B, cap, 4, **f32), torch.empty(B, cap, **f32)
        a = _lib.hg_region_priors_args()
        a.scores, a.labels, a.boxes = scores.data_ptr(), labels.data_ptr(), boxes.data_ptr()
        q_off = [0]
        for q in sizes:
            q_off.append(q_off[-1] + q)
        off_c = (_lib.C.c_int32 * (B + 1))(*q_off)
        size_c = (_lib.C.c_float * (2 * B))(*host_sizes(image_sizes, B))
        a.q_off, a.image_sizes, a.B = off_c, size_c, B
        a.box_score_thresh, a.nms_thresh = p.box_score_thresh, p.nms_thresh
        a.human_idx, a.min_instances, a.max_instances = p.human_idx, p.min_instances, p.max_instances
        a.prior_slot = pri.slot if pri is not None else -1
        a.counts, a.keep, a.out_boxes, a.out_scores, a.out_labels = (t.data_ptr() for t in (counts, keep, out_boxes, out_scores, out_labels))
        priors = mask = None
        if pri is not None:
            priors, mask = torch.empty(B, cap, OUT_DIM, **f32), torch.empty(B, cap, dtype=torch.uint8, device=dev)
            a.priors, a.mask = priors.data_ptr(), mask.data_ptr()
        with torch.cuda.device(idx):
            rc = _lib.lib().hg_region_priors(_lib.ctx(idx), _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
        _lib.check(idx, rc, "hg_region_priors")
        host = counts.cpu().tolist()      # the one device-to-host copy of the call
        for b, row in enumerate(host):
            if row[2] & 1:
                raise RuntimeError(f"hoigen_amd: image {b} of the batch has a non-finite score or box coordinate")
            if row[2] & 2:
                raise RuntimeError(f"hoigen_amd: image {b} of the batch has a label outside object_embedding's {pri.n_obj_classes} rows")
        region_props = split_region_props(host, out_boxes, out_scores, out_labels, label_dtype)
        for rp, k, row in zip(region_props, keep, host):
            rp["keep"] = k[:row[0]].to(torch.int64)      # indices into the image's detections, for callers that carry more per detection
        if pri is None:
            return region_props, None
        max_n = max(row[0] for row in host)
        return region_props, (priors[:, :max_n], mask[:, :max_n].bool())
