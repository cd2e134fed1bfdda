#!/usr/bin/env python3
"""Generates tests/golden/g20_detr_heads.npz: the reference's own heads and PostProcess in fp32 on `hs_last` of g19_detr_transformer.npz
(B = 3, Q = 100, D = 256), with the seeded head weights of tests/detr_heads_cases.py (G20: 92 logits) and three image sizes:

  * `logits` = class_embed(hs), `pred_boxes` = bbox_embed(hs).sigmoid()          (detr/models/detr.py:67-68 with :37-38)
  * `scores`, `labels`, `boxes` = PostProcess()({'pred_logits', 'pred_boxes'}, target_sizes)      (detr.py:258-290)

detr/models/detr.py cannot be imported here (util/box_ops.py imports torchvision), so the statements of `PostProcess` (detr.py:258-290),
`MLP` (:293-305) and `box_cxcywh_to_xyxy` (util/box_ops.py:9-13) are read from the reference tree at run time and executed.  Runs only
where the reference is checked out (REFERENCE, default /root/reference), never on the GPU box:
    python tests/golden/make_golden_detr_heads.py
Nothing of the reference's source is stored: the fixture holds outputs only."""
import os
import sys
import textwrap
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import detr_heads_cases as hc  # noqa: E402

REF = os.environ.get("REFERENCE", "/root/reference")


def reference_lines(path, a, b, ns):
    """exec the 1-based inclusive lines a .. b of a file of the reference"""
    src = f"{REF}/{path}"
    lines = open(src).read().split("\n")
    exec(compile(textwrap.dedent("\n".join(lines[a - 1:b])), f"{src}:{a}-{b}", "exec"), ns)
    return ns


def main():
    g = hc.G20
    box_ops = types.SimpleNamespace(**{k: v for k, v in reference_lines("detr/util/box_ops.py", 9, 13, {"torch": torch}).items()
                                       if k == "box_cxcywh_to_xyxy"})
    ns = {"torch": torch, "nn": nn, "F": torch.nn.functional, "box_ops": box_ops}
    reference_lines("detr/models/detr.py", 258, 290, ns)
    reference_lines("detr/models/detr.py", 293, 305, ns)
    class_embed, bbox_embed, post = nn.Linear(g["D"], g["C1"]), ns["MLP"](g["D"], g["D"], 4, 3), ns["PostProcess"]()
    sd = {k: torch.from_numpy(v) for k, v in hc.weights(g["D"], g["C1"], g["wseed"]).items()}
    class_embed.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("class_embed.")}, strict=True)
    bbox_embed.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("bbox_embed.")}, strict=True)
    hs = torch.from_numpy(np.load(os.path.join(HERE, "g19_detr_transformer.npz"))["hs_last"])
    sizes = torch.tensor(g["sizes"], dtype=torch.float32)
    out = {}
    for dt in (torch.float32, torch.float64):
        with torch.no_grad():
            ce, be = class_embed.to(dt), bbox_embed.to(dt)
            logits, pb = ce(hs.to(dt)), be(hs.to(dt)).sigmoid()
            res = post({"pred_logits": logits, "pred_boxes": pb}, sizes.to(dt))
        cur = dict(logits=logits, pred_boxes=pb, scores=torch.stack([r["scores"] for r in res]), labels=torch.stack([r["labels"] for r in res]),
                   boxes=torch.stack([r["boxes"] for r in res]))
        if dt == torch.float32:
            out = {k: v.numpy() for k, v in cur.items()}
        else:
            for k in ("logits", "pred_boxes", "scores", "boxes"):
                d = torch.from_numpy(out[k]).double() - cur[k]
                print(f"{k}: the reference's fp32 run against its fp64 run: relative L2 {float(d.norm() / cur[k].norm()):.2e}, "
                      f"max abs {float(d.abs().max()):.2e}")
            print("labels equal:", bool((torch.from_numpy(out["labels"]) == cur["labels"]).all()))
    assert out["logits"].shape == (3, 100, 92) and out["labels"].dtype == np.int64 and out["boxes"].shape == (3, 100, 4)
    path = os.path.join(HERE, "g20_detr_heads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
