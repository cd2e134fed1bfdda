#!/usr/bin/env python3
"""Fixtures g12 for the reference's second backbone, ViT-L/14@336px, by running the REFERENCE ITSELF on
``synth.clip_state_dict(synth.VIT_L14_336, 0)`` (427.9 M parameters, 577 tokens per image).

Runs where the reference is available, on the CPU (about two minutes on 16 threads).  Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vitl.py

  g12_vitl14_336.npz        encode_image of synth.crops(4, 336, seed=1234); class row after every block; 64 fixed token
                            rows of image 0 after the last block; variant C built with use_adapter=False, prior=None, on
                            the first 2 crops: global rows, the local map's 768-channel rows at 64 fixed (y, x) positions, the map's fp64 sum
  g12_vitl14_336_text.npz   encode_text of the 117 verb sentences and the 81 object prompts of g0_tokens.json (a file of its
                            own so that each stays below 1 MiB)
  g12_vitl14_336_keys.json  names and shapes of the reference model's state dict at this shape
"""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from hoigen_amd import synth  # noqa: E402

TOK_ROWS = (np.arange(64) * 9 + 1) % 577          # 64 token rows of image 0 (1, 10, ... : patch rows all over the grid)
TOK_ROWS[0] = 0                                    # ... and the class row


def local_positions():
    """64 fixed (y, x) positions of the [768, 24, 24] local map (all 768 channels are stored at each)."""
    i = np.arange(64)
    return np.stack([(i * 5 + 3) % 24, (i * 7 + 1) % 24], axis=1).astype(np.int64)


def prompt_ids(g0):
    rows = g0["verb117"]["ids"] + g0["obj81"]["ids"]
    ids = np.zeros((len(rows), 77), np.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    return ids


@torch.no_grad()
def main():
    torch.set_num_threads(min(os.cpu_count(), 16))
    clipnet, adapter_mod = mg.load_reference()
    cfg = synth.VIT_L14_336
    img = torch.from_numpy(synth.crops(4, 336, seed=1234))
    res = {}
    mA = mg.build_ref_A(clipnet, cfg, seed=0)
    assert mA.visual.input_resolution == 336 and len(mA.visual.transformer.resblocks) == 24
    store = []
    hooks = mg.hook_blocks(mA.visual.transformer.resblocks, store)
    res["encode_image"] = mA.encode_image(img).numpy()                          # [4,768]
    keys = {k: list(v.shape) for k, v in mA.state_dict().items()}                # the reference model's own parameter names and shapes
    for h in hooks:
        h.remove()
    res["cls_after_block"] = np.stack([s[:, 0, :] for s in store])              # [24,4,1024]
    res["tok_rows"] = TOK_ROWS.astype(np.int64)
    res["tok_after_block23_img0"] = store[-1][0][TOK_ROWS]                      # [64,1024]
    del store
    g0 = json.load(open(f"{HERE}/g0_tokens.json"))
    ids = torch.from_numpy(prompt_ids(g0))
    txt = torch.cat([mA.encode_text(ids[i:i + 66]) for i in range(0, len(ids), 66)]).numpy()   # [198,768]
    del mA
    sd = mg.t(synth.clip_state_dict(cfg, 0))
    mC = adapter_mod.build_model(sd, use_adapter=False).eval()
    g, l = mC.visual(img[:2], None)
    assert tuple(g.shape) == (2, 768) and tuple(l.shape) == (2, 768, 24, 24)
    l = l.contiguous().numpy()
    pos = local_positions()
    res["c_noprior_global"] = g.numpy()
    res["c_local_pos"] = pos
    res["c_noprior_local_at"] = np.stack([l[:, :, y, x] for y, x in pos], axis=1)                           # [2,64,768]: whole rows
    res["c_noprior_local_sum"] = l.astype(np.float64).sum(axis=(1, 2, 3))                                   # [2] fp64
    np.savez_compressed(f"{HERE}/g12_vitl14_336.npz", **res)
    np.savez_compressed(f"{HERE}/g12_vitl14_336_text.npz", verb117_obj81=txt)
    json.dump(keys, open(f"{HERE}/g12_vitl14_336_keys.json", "w"), separators=(",", ":"))
    print("g12:", {k: v.shape for k, v in res.items()}, txt.shape)


if __name__ == "__main__":
    main()
