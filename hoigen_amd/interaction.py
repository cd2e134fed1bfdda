"""The interaction head behind the towers, for a whole batch in one call (``hg_hoi_head``).

Counterpart of ``UPT.compute_roi_embeddings`` + ``compute_prior_scores`` + ``postprocessing``
(upt_tip_cache_model_free_finetune_distill3.py:959-1268, :806-833, :1408-1427) in eval mode with ``individual_norm = True``,
``logits_type = 'HO+U+T'``, no ``use_weight_pred``, generated features not appended (the ``eval_ar`` / ``cache`` path):

    head = HOIHead([("human", cache_H, s_H), ("object", cache_O, s_O), ("union", cache_U, s_U), ("union", text, s_T)],
                   object_class_to_target_class, human_idx, num_classes)
    logits, prior, bh, bo, objects = head(feat_global, feat_local, image_sizes, region_props)
    detections = head.postprocess(boxes, bh, bo, logits, prior, objects, image_sizes)

The DINO branch (:1111-1115, :1184-1207; on by default in the reference, main_tip_finetune.py:393) is a sixth branch of source ``"image"``:
one row of cache-model logits per IMAGE, computed once and added to every pair of the image in its place of the list, so
``[H, O, U, text, global, image]`` is the sum of :1205-1207 term for term:

    dino = CacheLogits(dino_cache.T, dino_cache_bias, dino_cache_values, dino_sample_len)
    head = HOIHead([..., ("global", cache_G, s_G), ("image", dino, dino_cache_logit)], ...)
    out = head(feat_global, feat_local, image_sizes, region_props, feat_image=dino_model.normalized(images))      # ResNetFeatures

``region_props`` may be the list ``hoigen_amd.proposals.DetectorFrontEnd`` returned (NMS / ``prepare_region_proposals``, ``get_prior`` /
``priors_downproj`` in one call of their own): its dicts carry the human counts, and no label leaves the device here.  Out of scope,
plain torch in the caller as before: the training-time appended features (``gen_to_dino``, :1122-1127, among them) and losses.  Inference only; CPU tensors and gradient callers raise ``RuntimeError`` (there is no
CPU fallback).
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .cache_model import CacheLogits

SOURCES = tuple(_lib.HG_HOI_SRC)


def plan_batch(labels: Sequence[torch.Tensor], human_idx: int):
    """Host side of a call from the per-image label tensors: the reference's stable permutation that puts humans first
    (:988-996; the identity where they already are), box offsets, human counts and pair counts ``n_h (n - 1)`` (none when
    ``n_h == 0`` or ``n <= 1``, :998) -> ``(perm [list of int64 tensors], box_off [B + 1], n_human [B], pair_off [B + 1])``.
    The labels of the whole batch come to the host in ONE transfer; everything per image below is host arithmetic."""
    perm, box_off, n_human, pair_off = [], [0], [], [0]
    sizes = [int(lb.numel()) for lb in labels]
    flat = torch.cat([lb.detach().reshape(-1) for lb in labels]).cpu() if labels else torch.zeros(0, dtype=torch.int64)
    for lb in torch.split(flat, sizes):
        is_human = lb == human_idx
        n_h, n = int(is_human.sum()), int(lb.numel())
        if not bool(torch.all(lb[:n_h] == human_idx)):
            p = torch.cat([torch.nonzero(is_human).squeeze(1), torch.nonzero(is_human == 0).squeeze(1)])
        else:
            p = torch.arange(n)
        perm.append(p)
        box_off.append(box_off[-1] + n)
        n_human.append(n_h)
        pair_off.append(pair_off[-1] + (n_h * (n - 1) if n > 1 else 0))
    return perm, box_off, n_human, pair_off


def plan_from_counts(sizes: Sequence[int], n_humans: Sequence[int]):
    """``plan_batch`` for region proposals that arrive humans first with their human counts on the host - what
    ``hoigen_amd.proposals.DetectorFrontEnd`` returns (``n_human`` in every dict): the permutation is the identity and no label leaves
    the device."""
    perm, box_off, n_human, pair_off = [], [0], [], [0]
    for n, n_h in zip(sizes, n_humans):
        perm.append(torch.arange(n))
        box_off.append(box_off[-1] + n)
        n_human.append(int(n_h))
        pair_off.append(pair_off[-1] + (n_h * (n - 1) if n > 1 else 0))
    return perm, box_off, n_human, pair_off


def split_outputs(pair_off, logits, prior, pair_h, pair_o, objects, label_dtype=torch.int64):
    """The batch tensors of ``hg_hoi_head`` as the reference's per-image lists: ``logits [p, NC]``, ``prior [2, p, NC]``,
    ``bh``, ``bo`` int64 ``[p]``, ``objects [p]`` in the labels' dtype.  An image without pairs gets ``zeros(0)`` index tensors and
    a ``[2, 0, NC]`` prior as in the reference (:1000-1003), and - unlike the reference, which appends nothing - an empty
    ``[0, NC]`` logits entry, so that every list has one entry per image (``torch.cat(logits)`` is the same tensor either way)."""
    out = ([], [], [], [], [])
    for b in range(len(pair_off) - 1):
        lo, hi = pair_off[b], pair_off[b + 1]
        out[0].append(logits[lo:hi])
        out[1].append(prior[:, lo:hi])
        out[2].append(pair_h[lo:hi].to(torch.int64))
        out[3].append(pair_o[lo:hi].to(torch.int64))
        out[4].append(objects[lo:hi].to(label_dtype))
    return out


def target_table(obj2target, num_classes: int) -> torch.Tensor:
    """multi-hot uint8 ``[n_obj_classes, num_classes]`` from the reference's ``object_class_to_target_class`` (a list of lists of target
    indices per object class), or a tensor of that shape as it is"""
    if isinstance(obj2target, torch.Tensor):
        if obj2target.dim() != 2 or obj2target.shape[1] != num_classes:
            raise ValueError(f"obj2target must be [n_obj_classes, {num_classes}]")
        return (obj2target != 0).to(torch.uint8).contiguous()
    t = torch.zeros(len(obj2target), num_classes, dtype=torch.uint8)
    for o, tar in enumerate(obj2target):
        for k in tar:
            t[o, int(k)] = 1
    return t


class HOIHead:
    """``HOIHead(branches, obj2target, human_idx, num_classes, hyper_lambda=2.8, pool=7)``.

    ``branches``: at most 6 entries ``(source, CacheLogits, scale)`` with ``source`` one of ``"human"``, ``"object"``, ``"union"``,
    ``"human_object"`` (the ``[P, 2C]`` concatenation, :1166) and ``"global"`` (``feat_global[b]`` normalised, repeated over the
    image's pairs, :1132-1138) and ``"image"`` (a ``CacheLogits`` of any ``K % 64 == 0`` up to 4096 on the rows of ``feat_image [B, K]``
    as they are - the caller normalises - computed once per image and read by each of its pairs, :1111-1115, :1184-1207); the logits are ``sum_b scale_b * branch_b`` in list order (:1195-1196).  ``hyper_lambda`` is the power
    of the detection scores in the priors (:814; pass 1.0 for the training-time value)."""

    def __init__(self, branches, obj2target, human_idx: int, num_classes: int, hyper_lambda: float = 2.8, pool: int = 7):
        if len(branches) > _lib.HG_HOI_MAX_BRANCH:
            raise ValueError(f"at most {_lib.HG_HOI_MAX_BRANCH} branches")
        for src, cache, _ in branches:
            if src not in _lib.HG_HOI_SRC:
                raise ValueError(f"unknown branch source {src!r}; one of {SOURCES}")
            if not isinstance(cache, CacheLogits):
                raise TypeError("a branch holds a hoigen_amd.cache_model.CacheLogits")
        self.branches = [(s, c, float(w)) for s, c, w in branches]
        self.num_classes, self.human_idx = int(num_classes), int(human_idx)
        self.hyper_lambda, self.pool = float(hyper_lambda), int(pool)
        self.obj2target = target_table(obj2target, self.num_classes)

    def _check(self, tensors):
        if torch.is_grad_enabled() and any(t is not None and t.is_floating_point() and t.requires_grad for t in tensors):
            raise RuntimeError("hoigen_amd: HOIHead is inference only (an input requires grad); call it under torch.no_grad() or "
                               "detach the inputs")
        if any(t is not None and t.device.type != "cuda" for t in tensors):
            raise RuntimeError("hoigen_amd: HOIHead runs only on a HIP device (there is no CPU fallback)")

    def __call__(self, feat_global: Optional[torch.Tensor], feat_local: torch.Tensor, image_sizes: torch.Tensor,
                 region_props: List[dict], feat_image: Optional[torch.Tensor] = None) -> Tuple[list, list, list, list, list]:
        """``feat_image [B, K]``: the rows of the ``"image"`` branches (``ResNetFeatures.normalized``); needed by such a branch,
        ignored without one."""
        has_image = any(src == "image" for src, _, _ in self.branches)
        if has_image and feat_image is None:
            raise RuntimeError("hoigen_amd: HOIHead has an \"image\" branch: pass feat_image [B, K] (ResNetFeatures.normalized(images))")
        if not has_image:
            feat_image = None
        self._check([feat_global, feat_local, feat_image] + [p[k] for p in region_props for k in ("boxes", "scores")])
        if not region_props:
            return [], [], [], [], []
        if feat_local.dim() != 4 or feat_local.shape[0] != len(region_props):
            raise ValueError("feat_local must be [B, C, H, W] with one region_props entry per image")
        dev = feat_local.device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        B, C, H, W = feat_local.shape
        NC = self.num_classes
        # spatial_scale = 1 / (image_size[0, 0] / local_features.shape[1]) in the tensor's own arithmetic (:1027)
        scale = float(1 / (image_sizes[0, 0] / H))
        labels = [p["labels"] for p in region_props]
        if all(isinstance(p.get("n_human"), int) for p in region_props):      # DetectorFrontEnd's: humans first, counts on the host
            perm, box_off, n_human, pair_off = plan_from_counts([int(lb.numel()) for lb in labels], [p["n_human"] for p in region_props])
        else:
            perm, box_off, n_human, pair_off = plan_batch(labels, self.human_idx)
        N, Pt = box_off[-1], pair_off[-1]
        label_dtype = labels[0].dtype if labels else torch.int64
        order = torch.cat([p + o for p, o in zip(perm, box_off)]).to(dev) if N else torch.zeros(0, dtype=torch.int64, device=dev)
        boxes = torch.cat([p["boxes"].detach().reshape(-1, 4) for p in region_props]).to(dev).float()[order].contiguous()
        scores = torch.cat([p["scores"].detach().reshape(-1) for p in region_props]).to(dev).float()[order].contiguous()
        lab32 = torch.cat([lb.detach().reshape(-1) for lb in labels]).to(dev)[order].to(torch.int32).contiguous()
        if self.obj2target.device != dev:
            self.obj2target = self.obj2target.to(dev)
        fl = feat_local.detach().float().contiguous()
        fg = feat_global.detach().float().contiguous() if feat_global is not None else None
        fi = None
        if feat_image is not None:
            if feat_image.dim() != 2 or feat_image.shape[0] != B:
                raise ValueError(f"feat_image must be [{B}, K] (got {tuple(feat_image.shape)})")
            fi = feat_image.detach().float().contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        pair_h, pair_o, objects = torch.empty(Pt, **i32), torch.empty(Pt, **i32), torch.empty(Pt, **i32)
        logits, prior, dense = torch.zeros(Pt, NC, **f32), torch.zeros(2, Pt, NC, **f32), torch.zeros(Pt, NC, **f32)
        a = _lib.hg_hoi_head_args()
        a.feat_local, a.feat_global = fl.data_ptr(), fg.data_ptr() if fg is not None else None
        a.boxes, a.scores, a.labels = boxes.data_ptr(), scores.data_ptr(), lab32.data_ptr()
        off_c = (_lib.C.c_int32 * (B + 1))(*box_off)
        nh_c = (_lib.C.c_int32 * max(B, 1))(*n_human)
        a.box_off, a.n_human = off_c, nh_c
        a.B, a.C, a.H, a.W, a.P, a.spatial_scale = B, C, H, W, self.pool, scale
        a.n_branch = len(self.branches)
        for i, (src, cache, w) in enumerate(self.branches):
            if cache.slot is None:
                raise RuntimeError("hoigen_amd: a branch's CacheLogits has been closed")
            a.branch[i].source, a.branch[i].slot, a.branch[i].scale = _lib.HG_HOI_SRC[src], cache.slot, w
        a.obj2target, a.n_obj_classes, a.num_classes = self.obj2target.data_ptr(), self.obj2target.shape[0], NC
        a.score_pow = self.hyper_lambda
        a.pair_h, a.pair_o, a.objects = pair_h.data_ptr(), pair_o.data_ptr(), objects.data_ptr()
        a.logits, a.prior, a.scores_out = logits.data_ptr(), prior.data_ptr(), dense.data_ptr()
        with torch.cuda.device(idx):
            if fi is None:
                rc = _lib.lib().hg_hoi_head(_lib.ctx(idx), _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
            else:
                im = _lib.hg_hoi_image_args(fi.data_ptr(), int(fi.shape[1]), None)
                rc = _lib.lib().hg_hoi_head_image(_lib.ctx(idx), _lib.C.byref(a), _lib.C.byref(im), torch.cuda.current_stream().cuda_stream)
        _lib.check(idx, rc, "hg_hoi_head")
        out = split_outputs(pair_off, logits, prior, pair_h, pair_o, objects, label_dtype)
        for b, lg in enumerate(out[0]):      # the dense scores travel with the logits they belong to: postprocess keeps no state
            lg.hg_dense_scores = dense[pair_off[b]:pair_off[b + 1]]
        return out

    def postprocess(self, boxes, bh, bo, logits, prior, objects, image_sizes) -> List[dict]:
        """The reference's detection dicts (:1408-1427).  ``nonzero`` stays a torch op, so the order of the detections is the
        reference's; their scores ``sigmoid(logits) * prior[0] * prior[1]`` are read from the dense matrix the kernel wrote in the
        call that produced ``logits``.  Every logits tensor a ``HOIHead`` call returns carries that matrix with it
        (``hg_dense_scores``), so the batches of any number of calls can be post-processed in any order; logits from elsewhere (a
        clone, a tensor of the caller's) are refused - there is no second implementation of the score here."""
        dense_scores = [getattr(lg, "hg_dense_scores", None) for lg in logits]
        if any(d is None for d in dense_scores):
            raise RuntimeError("hoigen_amd: postprocess takes the logits tensors that a HOIHead call returned")
        detections = []
        for bx, h, o, pr, obj, size, dense in zip(boxes, bh, bo, prior, objects, image_sizes, dense_scores):
            x, y = torch.nonzero(pr.prod(0)).unbind(1)
            detections.append(dict(boxes=bx, pairing=torch.stack([h[x], o[x]]), scores=dense[x, y], labels=y, objects=obj[x], size=size))
        return detections
