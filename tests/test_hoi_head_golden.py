"""The test reference of the interaction head (tests/hoi_head_bound.py, with oracle/cache_oracle.py for the branches) against
tests/golden/g14_hoi_head.npz: the outputs of the reference's own statements - pair enumeration and union boxes, normalisation, the
logits expressions, compute_prior_scores, postprocessing - executed on seeded inputs (tests/golden/make_golden_hoi_head.py).  The pooled
means in the fixture are oracle/roi_oracle.py's: that step is pinned to the oracle only (tests/golden/README_hoi_head.md)."""
import os
import sys

import numpy as np

import hoi_head_bound as hb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import hoi_head_cases as hc  # noqa: E402
from oracle import cache_oracle  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_hoi_head.npz"))
SCALE = np.float32(1.0) / (np.float32(hc.IMAGE) / np.float32(hc.H))


def test_pairs_union_boxes_and_objects():
    for i in range(len(hc.SIZES)):
        im = hc.image(i)
        pr = hb.batch_pairs(im["boxes"], im["labels"], [0, hc.SIZES[i]], [hc.HUMANS[i]])
        assert np.array_equal(pr["pair_h"], G[f"x_keep_{i}"]) and np.array_equal(pr["pair_o"], G[f"y_keep_{i}"])
        assert np.array_equal(pr["union_boxes"], G[f"union_boxes_{i}"]) and np.array_equal(pr["objects"], G[f"objects_{i}"])
        assert len(pr["pair_h"]) == hc.HUMANS[i] * (hc.SIZES[i] - 1)


def test_pooled_means_within_both_bounds_of_the_oracle():
    for i in range(len(hc.SIZES)):
        im = hc.image(i)
        rois = np.concatenate([im["boxes"], G[f"union_boxes_{i}"]])
        got = hb.pool(im["feat"], rois, 7, SCALE)
        ref = hb.reference(im["feat"], rois, 7, SCALE)
        want = np.concatenate([G[f"pooled_single_{i}"], G[f"pooled_union_{i}"]])
        assert ref["kept"].all()
        assert (np.abs(got.astype(np.float64) - want) <= ref["E"] + ref["roi_E"]).all()


def test_logits_priors_and_detections():
    w = hc.weights()
    o2t = np.zeros((hc.N_OBJ, hc.NC), np.uint8)
    for o, tar in enumerate(w["obj2target"]):
        o2t[o, tar] = 1
    for i in range(len(hc.SIZES)):
        im = hc.image(i)
        x, y = G[f"x_keep_{i}"], G[f"y_keep_{i}"]
        single, union = G[f"pooled_single_{i}"], G[f"pooled_union_{i}"]
        unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)      # noqa: E731
        h, o, u = unit(single[x]), unit(single[y]), unit(union)
        branches = [cache_oracle.cache_logits(f, w[f"w_{k}"], w[f"b_{k}"], w[f"label_{k}"], w[f"lens_{k}"]) for f, k in ((h, "H"), (o, "O"), (u, "U"))]
        branches.append(cache_oracle.linear_logits(u, w["w_text"]))
        scales = [hc.SCALES[k] for k in ("gen_logit_scale_H", "gen_logit_scale_O", "gen_logit_scale_U", "logit_scale_text")]
        lg, prior, sc = hb.head(branches, scales, im["scores"][x], im["scores"][y], im["labels"][x], im["labels"][y], o2t, hc.HYPER_LAMBDA)
        assert np.allclose(lg, G[f"logits_{i}"], rtol=1e-5, atol=1e-5)
        gp = G[f"prior_{i}"]
        assert gp.shape == prior.shape == (2, len(x), hc.NC) and np.array_equal(gp != 0, prior != 0)
        assert (np.abs(prior.astype(np.float64) - gp) <= 4 * 2.0 ** -23 * np.abs(gp)).all()      # the fixture is torch's fp32 pow: half an ulp here, up to 3 ulp allowed there
        # the detections: nonzero of the product in row-major order, the dense score gathered
        px, py = np.nonzero(prior[0] * prior[1])
        assert np.array_equal(py, G[f"det_labels_{i}"]) and np.array_equal(np.stack([x[px], y[px]]), G[f"det_pairing_{i}"])
        assert np.array_equal(im["labels"][y][px], G[f"det_objects_{i}"])
        assert np.allclose(sc[px, py], G[f"det_scores_{i}"], rtol=2e-5, atol=1e-9)
