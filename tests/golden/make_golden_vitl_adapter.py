#!/usr/bin/env python3
"""Fixture g13: the reference's detector path on its second backbone - ViT-L/14@336px (577 tokens per image) WITH instance adapters in
front of every block - by running the REFERENCE ITSELF (variant C, CLIP_models_adapter_prior2.py) on
``synth.clip_state_dict(synth.VIT_L14_336, 0)`` + ``synth.adapter_state_dict(synth.VIT_L14_336, 1)``.

Runs where the reference is available, on the CPU (half a minute on 16 threads).  Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vitl_adapter.py

  g13_vitl14_336_adapter.npz   visual(x, (priors, mask)) of synth.crops(2, 336, seed=1234) with synth.priors(2, n=14, n_pad=4, seed=99):
                               global rows [2,768], the local map's 768-channel rows at the 64 (y, x) positions of g12
                               (make_golden_vitl.local_positions) [2,64,768], the map's fp64 sum [2]; and visual(x[:1], None) - the
                               adapters with the sequence as their own memory: the same three quantities for crop 0
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden_vitl import local_positions  # noqa: E402
from hoigen_amd import synth  # noqa: E402


def parts(g, l, pos):
    l = l.contiguous().numpy()
    return g.numpy(), np.stack([l[:, :, y, x] for y, x in pos], axis=1), l.astype(np.float64).sum(axis=(1, 2, 3))


@torch.no_grad()
def main():
    torch.set_num_threads(min(os.cpu_count(), 16))
    _, adapter_mod = mg.load_reference()
    cfg = synth.VIT_L14_336
    mC = mg.build_ref_C(adapter_mod, cfg, seed=0, adapter_seed=1)
    assert mC.visual.input_resolution == 336 and len(mC.visual.transformer.resblocks) == 24
    img = torch.from_numpy(synth.crops(2, 336, seed=1234))
    pri, mask = synth.priors(2, n=14, dim=64, n_pad=4, seed=99)
    pos = local_positions()
    res = {"c_local_pos": pos}
    g, l = mC.visual(img, (torch.from_numpy(pri), torch.from_numpy(mask)))
    assert tuple(g.shape) == (2, 768) and tuple(l.shape) == (2, 768, 24, 24)
    res["c_prior_global"], res["c_prior_local_at"], res["c_prior_local_sum"] = parts(g, l, pos)
    g, l = mC.visual(img[:1], None)
    res["c_self_global"], res["c_self_local_at"], res["c_self_local_sum"] = parts(g, l, pos)
    out = f"{HERE}/g13_vitl14_336_adapter.npz"
    np.savez_compressed(out, **res)
    print("g13:", {k: v.shape for k, v in res.items()}, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1 << 20


if __name__ == "__main__":
    main()
