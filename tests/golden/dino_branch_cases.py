"""Seeded inputs of the DINO-branch fixture (g24_dino_branch.npz).  The batch is the interaction-head fixture's (hoi_head_cases.py: three
images, a 64-channel 14 x 14 local map, 5 / 2 / 6 boxes, the four cache branches); added here: the DINO network (tests/resnet_cases.
small_resnet(), 512 channels, under a wrapper that adds torchvision's avgpool and an identity fc) with one 64 x 64 view per image,
the DINO and the global cache models, their two logit scales, and the inputs of build_dino_cache_model.  make_golden_dino_branch.py
and the tests both regenerate them; only the reference's outputs are stored."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoi_head_cases as hc  # noqa: E402,F401

B = len(hc.SIZES)
VIEW = 64                      # the DINO view's side: a 2 x 2 map behind small_resnet's layer4
K_DINO, S_DINO, S_GLOBAL = 512, 40, 30
SCALES = dict(hc.SCALES, clip_cache_logit=0.3, dino_cache_logit=0.6)
# build_dino_cache_model: N images of 2048 raw features (the reference draws torch.randn(2048) for a class without samples), classes 4
# and 5 stay empty
N_BUILD, D_BUILD, C_BUILD, SHOT, BATCH, SEED = 12, 2048, 6, 1, 5, 1234


def dino_net():
    """the seeded network and the wrapper the reference's dino_model is a stand-in for: resnet50 with fc = nn.Identity()"""
    import torch
    from torch import nn

    import resnet_cases as rc

    class WithPool(nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net
            self.avgpool, self.fc = nn.AdaptiveAvgPool2d((1, 1)), nn.Identity()

        def forward(self, x):
            return self.fc(torch.flatten(self.avgpool(self.net(x)), 1))

    return WithPool(rc.small_resnet()).eval()


def views():
    """[B, 3, VIEW, VIEW] float32"""
    return (np.random.RandomState(2400).randn(B, 3, VIEW, VIEW) * 1.2).astype(np.float32)


def feat_global():
    """[B, C] float32, NOT normalised (the reference normalises it at :960)"""
    return (np.random.RandomState(2401).randn(B, hc.C) * 3.0).astype(np.float32)


def caches():
    """dino_cache [K_DINO, S] and global_cache [C, S] with unit columns, their biases, multi-hot values [S, NC] and sample lengths [NC]"""
    rng = np.random.RandomState(2402)
    out = {}
    for name, K, S, bias in (("dino", K_DINO, S_DINO, -1.0), ("global", hc.C, S_GLOBAL, -0.5)):
        w = rng.randn(S, K).astype(np.float32)
        lab = (rng.uniform(size=(S, hc.NC)) < 0.2).astype(np.float32)
        out[f"{name}_cache"] = np.ascontiguousarray((w / np.linalg.norm(w, axis=1, keepdims=True)).T)
        out[f"{name}_bias"] = np.full(S, bias, np.float32)
        out[f"{name}_values"], out[f"{name}_len"] = lab, np.maximum(lab.sum(0), 1.0).astype(np.float32)
    return out


def build_inputs():
    """(raw features [N_BUILD, D_BUILD] float32, per-image verb lists)"""
    rng = np.random.RandomState(2403)
    feats = (rng.randn(N_BUILD, D_BUILD) * 4.0 + 0.5).astype(np.float32)
    verbs = [sorted(set(int(v) for v in rng.randint(0, C_BUILD - 2, size=1 + (i % 2)))) for i in range(N_BUILD)]
    return feats, verbs
