"""Feature-regeneration records: the producer of the ``union_embeddings_cachemodel_*.p`` entries that
``UPT.load_cache_model`` reads (/root/reference/upt_tip_cache_model_free_finetune_distill3.py:636-688):

    annotation[file_name] = {'boxes_h': [n,4], 'boxes_o': [n,4], 'verbs': [n], 'objects': [n],
                             'union_features': [n,512], 'object_features': [n,512], 'huamn_features': [n,512]}

(``huamn_features`` is the reference's spelling, :680.)  The reference ships only the consumer; the producer that
made its pickles is not in the tree.  Here every human-object pair of one image is turned into three crops - human
box, object box and their union box (min/max corners, pre_images/crop_images.py:207-209) - pre-processed on the
device (``CropPreprocessor``: PIL crop + CLIP transform, bit-exact with Pillow) and encoded with ``encode_image`` in
ONE batch of 3n crops; features are returned un-normalised (the consumer divides by the norm itself, :678-680).
BASELINE.json config 5 ("pre-extracted-feature regeneration") is this loop over a dataset with the batch sharded
over the GPUs (hoigen_amd.distributed).
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .preprocess import CropPreprocessor


def union_boxes(boxes_h: np.ndarray, boxes_o: np.ndarray) -> np.ndarray:
    """[min(x1), min(y1), max(x2), max(y2)] of every pair (pre_images/crop_images.py:207-209)."""
    bh, bo = np.asarray(boxes_h).reshape(-1, 4), np.asarray(boxes_o).reshape(-1, 4)
    return np.concatenate([np.minimum(bh[:, :2], bo[:, :2]), np.maximum(bh[:, 2:], bo[:, 2:])], axis=1)


def pil_box(boxes: np.ndarray) -> np.ndarray:
    """Float boxes -> the integer box PIL's ``image.crop`` uses: each coordinate rounded to the nearest integer
    (ImageCrop: ``int(round(x))``)."""
    return np.rint(np.asarray(boxes, np.float64)).astype(np.int32)


def plan_record_batches(pair_counts: Sequence[int], max_crops: int = 256, max_images: int = 64) -> List[Tuple[int, int]]:
    """Cut images 0 .. len(pair_counts) - 1, in order, into groups [first, last) of at most ``max_images`` images and at most
    ``max_crops`` crops (an image of n pairs has 3 n crops).  An image's crops are never split: an image that alone exceeds
    ``max_crops`` forms a group of its own.  Pure host."""
    if max_crops < 1 or max_images < 1:
        raise ValueError("max_crops and max_images must be >= 1")
    groups, first, crops = [], 0, 0
    for i, n in enumerate(pair_counts):
        if n < 0:
            raise ValueError("negative pair count")
        if i > first and (i - first >= max_images or crops + 3 * n > max_crops):
            groups.append((first, i))
            first, crops = i, 0
        crops += 3 * n
    if len(pair_counts) > first:
        groups.append((first, len(pair_counts)))
    return groups


@torch.no_grad()
def emit_records(clip_model, images, annotations, n_px: int = 224, max_crops: int = 256,
                 preprocessor: CropPreprocessor = None) -> List[Dict[str, np.ndarray]]:
    """The records of a sequence of images, the list ``[emit_record(clip_model, image, **annotation) ...]`` would give, with one
    ``CropPreprocessor.batch`` call, one ``encode_image`` and one device-to-host copy per group of ``plan_record_batches`` instead of per
    image.  ``annotations``: one dict with ``boxes_h``, ``boxes_o``, ``verbs``, ``objects`` per image.  The crops of an image keep the
    order union, object, human; they have the bits of the per-image crops.  (The features of a 6-crop and a 256-crop ``encode_image``
    call differ within the tower's contract: the tower chooses its kernels by the rows of a call.)"""
    images, annotations = list(images), list(annotations)
    if len(images) != len(annotations):
        raise ValueError("one annotation per image")
    pre = preprocessor or CropPreprocessor(n_px)
    recs, crops = [], []
    for a in annotations:
        bh = np.asarray(a["boxes_h"], np.float32).reshape(-1, 4)
        bo = np.asarray(a["boxes_o"], np.float32).reshape(-1, 4)
        n = bh.shape[0]
        if bo.shape[0] != n or len(a["verbs"]) != n or len(a["objects"]) != n:
            raise ValueError("boxes_h, boxes_o, verbs and objects must describe the same pairs")
        recs.append({"boxes_h": bh, "boxes_o": bo, "verbs": np.asarray(a["verbs"], np.int64), "objects": np.asarray(a["objects"], np.int64)})
        crops.append(np.concatenate([pil_box(union_boxes(bh, bo)), pil_box(bo), pil_box(bh)], axis=0).reshape(-1, 4))
    for first, last in plan_record_batches([r["boxes_h"].shape[0] for r in recs], max_crops):
        total = sum(c.shape[0] for c in crops[first:last])
        feats = np.zeros((0, clip_model.visual.output_dim), np.float32)
        if total:
            # One device-to-host copy per group: the per-crop status (0 .. 7, exact in fp32) rides as a last column of the features.
            # A refused crop is NaN and the tower runs on it before the error below is raised: checking first would cost a second copy
            # and a host wait in front of the tower for every group, to be quicker only where the call fails anyway.
            x, status = pre.batch(images[first:last], crops[first:last], check=False)
            both = torch.cat([clip_model.encode_image(x).float(), status.float()[:, None]], dim=1).cpu().numpy()      # the one copy
            feats, st = both[:, :-1], both[:, -1].astype(np.int64)
            if st.any():
                i = int(np.nonzero(st)[0][0])
                why = "; ".join(r for bit, r in CropPreprocessor.STATUS_REASONS if st[i] & bit)
                raise ValueError(f"{why}: crop {i} of the group of images {first} .. {last - 1}")
        at = 0
        for i in range(first, last):
            n = recs[i]["boxes_h"].shape[0]
            f = feats[at:at + 3 * n]
            at += 3 * n
            recs[i].update(union_features=f[:n].copy(), object_features=f[n:2 * n].copy(), huamn_features=f[2 * n:].copy())
    return recs


@torch.no_grad()
def emit_record(clip_model, image_u8: torch.Tensor, boxes_h, boxes_o, verbs, objects, n_px: int = 224,
                preprocessor: CropPreprocessor = None) -> Dict[str, np.ndarray]:
    """One image -> one record.  ``image_u8``: uint8 [H,W,3] on the HIP device; boxes (x1,y1,x2,y2) in pixels."""
    bh = np.asarray(boxes_h, np.float32).reshape(-1, 4)
    bo = np.asarray(boxes_o, np.float32).reshape(-1, 4)
    n = bh.shape[0]
    if bo.shape[0] != n or len(verbs) != n or len(objects) != n:
        raise ValueError("boxes_h, boxes_o, verbs and objects must describe the same pairs")
    pre = preprocessor or CropPreprocessor(n_px)
    rec = {"boxes_h": bh, "boxes_o": bo, "verbs": np.asarray(verbs, np.int64), "objects": np.asarray(objects, np.int64)}
    if n == 0:
        z = np.zeros((0, clip_model.visual.output_dim), np.float32)
        rec.update(union_features=z, object_features=z.copy(), huamn_features=z.copy())
        return rec
    crops = np.concatenate([pil_box(union_boxes(bh, bo)), pil_box(bo), pil_box(bh)], axis=0)
    feats = clip_model.encode_image(pre(image_u8, crops)).float().cpu().numpy()
    rec.update(union_features=feats[:n], object_features=feats[n:2 * n], huamn_features=feats[2 * n:])
    return rec
