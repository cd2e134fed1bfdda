#!/usr/bin/env python3
"""Generates tests/golden/g19_detr_decoder.npz and g19_detr_transformer.npz by running the reference's own TransformerDecoder and
Transformer (detr/models/transformer.py, loaded by file path: it imports nothing but torch) in fp32 on the seeded weights and inputs of
tests/detr_decoder_cases.py: the full configuration (256 / 8 / 2048 / 6, return_intermediate), B = 3, Q = 100, a 13 x 17 grid with
G18's rectangle mask, tgt = 0.  Recorded: hs[0] and hs[-1] of the decoder on a seeded memory ([Q, B, C]), and hs[-1] of the whole
Transformer.forward from src ([B, Q, C]; encoder weights of seed 18, decoder weights of seed 19).  Outputs only: no weights, no program
text.  It also prints how far the reference's fp32 run is from the same module in fp64.  Run in the build container:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_detr_decoder.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detr_decoder_cases as dd  # noqa: E402
import detr_encoder_cases as ec  # noqa: E402

REF = "/root/reference/detr/models/transformer.py"


def main():
    spec = importlib.util.spec_from_file_location("ref_detr_transformer", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cfg, g = dd.FULL, dd.G19
    D = cfg["d_model"]
    dsd = {k: torch.from_numpy(v) for k, v in dd.weights(cfg, g["wseed"]).items()}
    esd = {k: torch.from_numpy(v) for k, v in ec.weights(cfg, g["enc_wseed"]).items()}
    qe, memory, pos = (torch.from_numpy(a) for a in dd.inputs(g["B"], g["gh"], g["gw"], g["Q"], D, g["xseed"]))
    src, pos_map = (torch.from_numpy(a) for a in dd.src_map(g["B"], g["gh"], g["gw"], D, g["xseed"]))
    mask = torch.from_numpy(ec.rect_mask(g["gh"], g["gw"], g["visible"])).bool()
    dec_out, tr_out = {}, {}
    for dtype in (torch.float32, torch.float64):
        t = ref.Transformer(D, cfg["heads"], cfg["layers"], cfg["layers"], cfg["d_ff"], 0.1, "relu", False, True).to(dtype).eval()
        t.encoder.load_state_dict({k: v.to(dtype) for k, v in esd.items()})
        t.decoder.load_state_dict({k: v.to(dtype) for k, v in dsd.items()})
        with torch.no_grad():
            qp = qe.to(dtype).unsqueeze(1).repeat(1, g["B"], 1)
            dec_out[dtype] = t.decoder(torch.zeros_like(qp), memory.to(dtype), memory_key_padding_mask=mask, pos=pos.to(dtype), query_pos=qp)
            tr_out[dtype] = t(src.to(dtype), mask.view(g["B"], g["gh"], g["gw"]), qe.to(dtype), pos_map.to(dtype))[0]
    for name, o in (("decoder hs[0]", {k: v[0] for k, v in dec_out.items()}), ("decoder hs[-1]", {k: v[-1] for k, v in dec_out.items()}),
                    ("transformer hs[-1]", {k: v[-1] for k, v in tr_out.items()})):
        a, b = o[torch.float32].double(), o[torch.float64]
        rows = ((a - b).norm(dim=-1) / b.norm(dim=-1)).max()
        print(f"{name}: the reference's fp32 run is {float((a - b).norm() / b.norm()):.2e} (relative L2; worst row {float(rows):.2e}) from its fp64 run")
    path = os.path.join(HERE, "g19_detr_decoder.npz")
    np.savez_compressed(path, hs0=dec_out[torch.float32][0].numpy(), hs_last=dec_out[torch.float32][-1].numpy())
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    path = os.path.join(HERE, "g19_detr_transformer.npz")
    np.savez_compressed(path, hs_last=tr_out[torch.float32][-1].numpy())
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", tuple(tr_out[torch.float32][-1].shape))


if __name__ == "__main__":
    main()
