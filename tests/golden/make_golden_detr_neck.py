#!/usr/bin/env python3
"""Generates tests/golden/g21_detr_neck.npz: the reference's own statements between the ResNet body and the transformer in fp32 on the
seeded inputs of tests/detr_neck_cases.py (G21: Cin 2048, D 256, three images padded to 200 x 270 with sizes (200, 270), (150, 270),
(200, 181), a 7 x 9 grid):

  * `mask` = F.interpolate(m[None].float(), size=x.shape[-2:]).to(torch.bool)[0]      (detr/models/backbone.py:78), flattened to [B, S]
  * `pos`  = PositionEmbeddingSine(128, normalize=True)(NestedTensor(x, mask))        (detr/models/position_encoding.py:12-48)
  * `src`  = nn.Conv2d(2048, 256, 1)(x)                                               (detr/models/detr.py:40, :65)
    both as `.flatten(2).permute(2, 0, 1)` leaves them (detr/models/transformer.py:50-51), stored batch-first [B, S, C]
  * `src_fp32_vs_fp64_max_abs`, `pos_fp32_vs_fp64_max_abs`: the distance of the reference's fp32 run from its fp64 run.  The
    embedding's cumulative sums and dim_t are fp32 by the reference's own statements whatever the input's dtype, so for `pos` the fp64
    run is the float64 restatement of tests/detr_neck_bound.py

Neither file of the reference can be imported here (util/misc.py imports torchvision), so the statements are read from the reference tree
by line range at run time and executed.  Runs only where the reference is checked out (REFERENCE, default /root/reference), never on the
GPU box:
    python tests/golden/make_golden_detr_neck.py
Nothing of the reference's source is stored: the fixture holds outputs only."""
import math
import os
import sys
import textwrap
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import detr_neck_bound as nb  # noqa: E402
import detr_neck_cases as nc  # noqa: E402

REF = os.environ.get("REFERENCE", "/root/reference")


def reference_lines(path, a, b, ns):
    """exec the 1-based inclusive lines a .. b of a file of the reference"""
    src = f"{REF}/{path}"
    lines = open(src).read().split("\n")
    exec(compile(textwrap.dedent("\n".join(lines[a - 1:b])), f"{src}:{a}-{b}", "exec"), ns)
    return ns


def main():
    c = nc.g21_case()
    NestedTensor = lambda tensors, mask: types.SimpleNamespace(tensors=tensors, mask=mask)
    ns = {"torch": torch, "nn": nn, "math": math, "NestedTensor": NestedTensor}
    reference_lines("detr/models/position_encoding.py", 12, 48, ns)
    sine = ns["PositionEmbeddingSine"](c["D"] // 2, normalize=True)
    conv = nn.Conv2d(c["Cin"], c["D"], kernel_size=1)
    conv.load_state_dict({"weight": torch.from_numpy(c["w"]).reshape(c["D"], c["Cin"], 1, 1), "bias": torch.from_numpy(c["bias"])})
    m_all = torch.from_numpy(c["image_mask"]).to(torch.bool)
    out = {}
    for dt in (torch.float32, torch.float64):
        x = torch.from_numpy(c["x"]).to(dt)
        with torch.no_grad():
            masks = []
            for m in m_all:      # backbone.py:78 for every image of the batch, as BackboneBase.forward runs it on the batched mask
                masks.append(reference_lines("detr/models/backbone.py", 78, 78, {"F": torch.nn.functional, "torch": torch, "m": m[None], "x": x})["mask"][0])
            mask = torch.stack(masks)
            pos_embed = sine(NestedTensor(x, mask)).to(dt)
            t = reference_lines("detr/models/transformer.py", 50, 51, {"src": conv.to(dt)(x), "pos_embed": pos_embed})
        cur = dict(src=t["src"].permute(1, 0, 2).contiguous(), pos=t["pos_embed"].permute(1, 0, 2).contiguous())
        if dt == torch.float64:
            cur["pos"] = torch.from_numpy(nb.reference(c)["pos"])
        if dt == torch.float32:
            out = {k: v.numpy() for k, v in cur.items()}
            out["mask"] = mask.flatten(1).numpy()
        else:
            for k in ("src", "pos"):
                d = torch.from_numpy(out[k]).double() - cur[k]
                out[f"{k}_fp32_vs_fp64_max_abs"] = np.float64(d.abs().max())
                print(f"{k}: the reference's fp32 run against its fp64 run: relative L2 {float(d.norm() / cur[k].norm()):.2e}, "
                      f"max abs {float(d.abs().max()):.2e}")
    S = c["H"] * c["W"]
    assert out["src"].shape == (c["B"], S, c["D"]) and out["pos"].shape == out["src"].shape and out["mask"].shape == (c["B"], S)
    path = os.path.join(HERE, "g21_detr_neck.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
