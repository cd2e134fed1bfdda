"""tests/golden/g18_detr_encoder*.npz (the reference's own TransformerEncoder in fp32, recorded by tests/golden/make_golden_detr_encoder.py)
against the float64 restatement of tests/detr_encoder_cases.py: 1e-5 relative (the reference's fp32 run sits 4.2e-7 from its own fp64
run on this case, as the generator prints).  CPU only."""
import os

import numpy as np
import torch

import detr_encoder_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_restatement_reproduces_the_reference():
    g, cfg = dc.G18, dc.FULL
    sd = dc.weights(cfg, g["wseed"])
    src, pos = dc.inputs(g["B"], g["gh"], g["gw"], cfg["d_model"], g["xseed"])
    mask = dc.rect_mask(g["gh"], g["gw"], g["visible"])
    assert mask[0].sum() == 0 and mask[1].sum() == 221 - 120 and mask[2].sum() == 221 - 20
    streams = dc.encoder_fp64(sd, cfg, src, pos, mask)
    for name, layer in (("g18_detr_encoder_l1.npz", 0), ("g18_detr_encoder.npz", cfg["layers"] - 1)):
        want = np.load(os.path.join(GOLDEN, name))["out"]
        assert want.shape == (221, 3, 256) and want.dtype == np.float32
        w = torch.from_numpy(want).transpose(0, 1).reshape(-1, cfg["d_model"])
        e, r = dc.rel_l2(streams[layer], w)
        print(f"after layer {layer + 1}: restatement vs fixture rel L2 {e:.2e}, worst row {r:.2e}")
        assert e < 1e-5 and r < 1e-5


def test_weights_follow_the_stated_distributions():
    sd = dc.weights(dc.FULL, 18)
    assert len(sd) == 6 * 12
    w = sd["layers.0.self_attn.in_proj_weight"]
    a = np.sqrt(6.0 / (768 + 256))
    assert w.shape == (768, 256) and abs(w).max() <= a and abs(w.std() - a / np.sqrt(3)) < 0.01 * a
    assert abs(sd["layers.3.norm2.weight"].mean() - 1) < 0.05 and abs(sd["layers.3.linear1.bias"].std() - 0.1) < 0.01
    assert not np.array_equal(sd["layers.0.linear1.weight"], sd["layers.1.linear1.weight"])
