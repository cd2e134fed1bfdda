"""Seeded inputs of tests/golden/g15_region_props.npz (generator: make_golden_region_props.py; test: tests/test_region_props_golden.py).
Everything comes from hoigen_amd.synth's generator, so both sides regenerate it bit for bit; only the outputs are stored."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hoigen_amd.synth import hg_normal  # noqa: E402

F = np.float32
E, HIDDEN, OUT, N_CLASSES, HUMAN = 512, 128, 64, 6, 0
PARAMS = dict(human_idx=HUMAN, box_score_thresh=0.2, min_instances=3, max_instances=15, nms_thresh=0.5)
# per image: detections, clusters, mean score (the three profiles leave few, some and many instances), (h, w)
IMAGES = ((40, 8, 0.10, (480.0, 640.0)), (100, 20, 0.35, (427.0, 640.0)), (100, 12, 0.60, (600.0, 500.0)), (3, 3, 0.5, (333.0, 500.0)))


def weights():
    w = dict(w0=hg_normal((HIDDEN, E + 5), 151, 0.05), b0=hg_normal((HIDDEN,), 152, 0.05), w1=hg_normal((HIDDEN, HIDDEN), 153, 0.08),
             b1=hg_normal((HIDDEN,), 154, 0.05), w2=hg_normal((OUT, HIDDEN), 155, 0.08), b2=hg_normal((OUT,), 156, 0.05),
             emb=hg_normal((N_CLASSES, E), 157, 0.2))
    return {k: np.ascontiguousarray(v, F) for k, v in w.items()}


def image(i):
    Q, k, mean, (h, w) = IMAGES[i]
    z = hg_normal((6, max(Q, k)), 200 + i).astype(np.float64)
    cx, cy = w / 2 + w / 5 * z[0, :k], h / 2 + h / 5 * z[1, :k]
    bw, bh = 30 + 50 * np.abs(z[2, :k]), 30 + 50 * np.abs(z[3, :k])
    c = np.arange(Q) % k
    j = hg_normal((4, Q), 300 + i).astype(np.float64)
    x, y = cx[c] + 5 * j[0], cy[c] + 5 * j[1]
    ww, hh = bw[c] * (1 + 0.08 * j[2]), bh[c] * (1 + 0.08 * j[3])
    boxes = np.stack([x - ww / 2, y - hh / 2, x + ww / 2, y + hh / 2], 1).astype(F)
    labels = np.where(c % 3 == 0, HUMAN, 1 + c % (N_CLASSES - 1)).astype(np.int64)
    s = np.abs(mean + 0.25 * z[4, :Q] + 1e-4 * np.arange(Q))      # reflected into (0, 0.99), not clipped: no ties
    scores = np.where(s > 0.99, 1.98 - s, s).astype(F)
    assert len(np.unique(scores)) == Q      # distinct: the reference's argsort leaves ties open
    return scores, labels, boxes


def case():
    """the batch in the layout of tests/props_bound.py's cases"""
    ims = [image(i) for i in range(len(IMAGES))]
    q_off = np.concatenate([[0], np.cumsum([len(s) for s, _, _ in ims])]).astype(np.int64)
    return dict(B=len(ims), q_off=q_off, scores=np.concatenate([s for s, _, _ in ims]), labels=np.concatenate([l for _, l, _ in ims]),
                boxes=np.concatenate([b for _, _, b in ims]), image_sizes=np.array([im[3] for im in IMAGES], F), params=dict(PARAMS),
                weights=weights())
