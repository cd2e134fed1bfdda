#!/usr/bin/env python3
"""Generates tests/golden/g18_detr_encoder.npz and g18_detr_encoder_l1.npz by running the reference's own TransformerEncoder
(detr/models/transformer.py, loaded by file path: it imports nothing but torch) in fp32 on the seeded weights and inputs of
tests/detr_encoder_cases.py: B = 3 on a 13 x 17 grid, image 0 unpadded, image 1 visible on 10 x 12, image 2 on 4 x 5.  Recorded:
the encoder's output after layer 6 (g18_detr_encoder.npz) and after layer 1 (g18_detr_encoder_l1.npz), [S, B, C] fp32 - one array a
file, because the two together are 1.4 MB and a committed file stays below 1 MiB.  Outputs only: no weights, no program text.  It also
prints how far the reference's fp32 run is from the same module in fp64.  Run in the build container:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_detr_encoder.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detr_encoder_cases as dc  # noqa: E402

REF = "/root/reference/detr/models/transformer.py"


def main():
    spec = importlib.util.spec_from_file_location("ref_detr_transformer", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cfg, g = dc.FULL, dc.G18
    sd = {k: torch.from_numpy(v) for k, v in dc.weights(cfg, g["wseed"]).items()}
    src, pos = (torch.from_numpy(a) for a in dc.inputs(g["B"], g["gh"], g["gw"], cfg["d_model"], g["xseed"]))
    mask = torch.from_numpy(dc.rect_mask(g["gh"], g["gw"], g["visible"])).bool()
    outs = {}
    for dtype in (torch.float32, torch.float64):
        for n_layers in (1, cfg["layers"]):
            layer = ref.TransformerEncoderLayer(cfg["d_model"], cfg["heads"], cfg["d_ff"], 0.1, "relu", False)
            enc = ref.TransformerEncoder(layer, n_layers, None).to(dtype).eval()
            enc.load_state_dict({k: v.to(dtype) for k, v in sd.items() if int(k.split(".")[1]) < n_layers})
            with torch.no_grad():
                outs[dtype, n_layers] = enc(src.to(dtype), src_key_padding_mask=mask, pos=pos.to(dtype))
    for n_layers in (1, cfg["layers"]):
        a, b = outs[torch.float32, n_layers].double(), outs[torch.float64, n_layers]
        print(f"after layer {n_layers}: the reference's fp32 run is {float((a - b).norm() / b.norm()):.2e} (relative L2) from its fp64 run")
    for name, n_layers in (("g18_detr_encoder.npz", cfg["layers"]), ("g18_detr_encoder_l1.npz", 1)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, out=outs[torch.float32, n_layers].numpy())
        print("wrote", path, os.path.getsize(path) // 1024, "KiB", tuple(outs[torch.float32, n_layers].shape))


if __name__ == "__main__":
    main()
