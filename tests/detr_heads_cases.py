"""Seeded weights of the DETR heads (detr/models/detr.py:37-38: class_embed = nn.Linear(D, classes + 1), bbox_embed = MLP(D, D, 4, 3)) for
the fixture tests/golden/g20_detr_heads.npz and the tests that use it.  numpy only.  No GPU, no library.

Weights as tests/detr_decoder_cases.py makes them (Xavier-uniform matrices, 0.1 randn biases) under the detector's key names:
`class_embed.weight`, `class_embed.bias`, `bbox_embed.layers.{0,1,2}.weight` / `bias`."""
import numpy as np

import detr_encoder_cases as ec
from hoigen_amd import synth

# the fixture's case (tests/golden/make_golden_detr_heads.py): hs_last of g19_detr_transformer.npz (B = 3, Q = 100, D = 256), 92 logits,
# three images of different sizes as (h, w)
G20 = dict(D=256, C1=92, wseed=20, sizes=((480.0, 640.0), (427.0, 640.0), (375.0, 500.0)))


def weights(D=256, C1=92, seed=20):
    """state dict of the two heads -> float32 numpy arrays"""
    shapes = {"class_embed.weight": (C1, D), "class_embed.bias": (C1,)}
    for i, o in enumerate((D, D, 4)):
        shapes[f"bbox_embed.layers.{i}.weight"], shapes[f"bbox_embed.layers.{i}.bias"] = (o, D), (o,)
    sd = {}
    for name, shape in shapes.items():
        s = synth._seed_of(seed, "heads." + name)
        if len(shape) == 2:
            sd[name] = (np.sqrt(6.0 / (shape[0] + shape[1])) * ec._uniform(shape, s)).astype(np.float32)
        else:
            sd[name] = synth.hg_normal(shape, s, 0.1)
    return sd


def as_case(sd, hs, sizes, class_rows=None):
    """the dict tests/detr_heads_bound.py works on, from a state dict, hs [L, B, Q, D] and the (h, w) of every image"""
    hs = np.ascontiguousarray(hs, np.float32)
    L, B, Q, D = hs.shape
    g = lambda k: np.ascontiguousarray(sd[k], np.float32)
    C1 = g("class_embed.weight").shape[0] if class_rows is None else len(class_rows)
    return dict(hs=hs, wc=g("class_embed.weight"), bc=g("class_embed.bias"), w0=g("bbox_embed.layers.0.weight"), b0=g("bbox_embed.layers.0.bias"),
                w1=g("bbox_embed.layers.1.weight"), b1=g("bbox_embed.layers.1.bias"), w2=g("bbox_embed.layers.2.weight"),
                b2=g("bbox_embed.layers.2.bias"), sizes=np.asarray(sizes, np.float32).reshape(B, 2), family="randn", L=L, B=B, Q=Q, D=D, C1=C1,
                class_rows=None if class_rows is None else list(class_rows))
