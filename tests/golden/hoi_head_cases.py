"""Seeded inputs of the interaction-head fixture (g14_hoi_head.npz): three images with a 64-channel 14 x 14 local map and 2 - 6 boxes
each, humans first (label 0), four cache branches.  make_golden_hoi_head.py and tests/test_hoi_head_golden.py both regenerate them;
only the reference's outputs are stored."""
import numpy as np

C, H, W, NC, S, N_OBJ, IMAGE = 64, 14, 14, 24, 40, 12, 224
SIZES, HUMANS = (5, 2, 6), (2, 1, 3)
SCALES = {"gen_logit_scale_H": 0.7, "gen_logit_scale_O": 1.3, "gen_logit_scale_U": 1.0, "logit_scale_text": 2.1}
HYPER_LAMBDA = 2.8


def image(i):
    rng = np.random.RandomState(1400 + i)
    n, n_h = SIZES[i], HUMANS[i]
    xy = rng.uniform(-10.0, 150.0, size=(n, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(8.0, 90.0, size=(n, 2))], 1).astype(np.float32)
    return {"feat": rng.randn(C, H, W).astype(np.float32), "boxes": boxes, "scores": rng.uniform(0.05, 1.0, size=n).astype(np.float32),
            "labels": np.r_[np.zeros(n_h, np.int64), rng.randint(1, N_OBJ, size=n - n_h)]}


def weights():
    rng = np.random.RandomState(1499)
    out = {}
    for k in "HOU":
        w = rng.randn(S, C).astype(np.float32)
        lab = (rng.uniform(size=(S, NC)) < 0.2).astype(np.float32)
        out[f"w_{k}"], out[f"b_{k}"] = w / np.linalg.norm(w, axis=1, keepdims=True), -np.ones(S, np.float32)
        out[f"label_{k}"], out[f"lens_{k}"] = lab, np.maximum(lab.sum(0), 1.0).astype(np.float32)
    t = rng.randn(NC, C).astype(np.float32)
    out["w_text"] = t / np.linalg.norm(t, axis=1, keepdims=True)
    out["obj2target"] = [sorted(rng.choice(NC, size=rng.randint(1, 6), replace=False).tolist()) for _ in range(N_OBJ)]
    return out
