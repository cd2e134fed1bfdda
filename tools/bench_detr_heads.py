#!/usr/bin/env python3
"""Times the DETR heads and PostProcess on the HIP path (hoigen_amd.detr.DetectionHeads: one hg_detr_heads launch)
against the statements it replaces as torch's own fp32 modules on the same tensors (upt_tip_cache_model_free_finetune_distill3.py:1598-1605:
class_embed(hs), bbox_embed(hs).sigmoid(), PostProcess on the last level).

Shapes: B in {1, 4, 8}, Q = 100, L in {1, 6}, D = 256, C1 = 92.  For each, in turn, round after round, each timed with a pair of events
around `--inner` calls that end in a synchronise; median and min .. max over the rounds:

  * native, every level: `DetectionHeads._run(hs, sizes, True)` - logits and boxes of all L levels and the detections, what the torch
    statements compute;
  * native, detections only: `DetectionHeads.detect(hs, sizes)` - the last level alone, what `UPT.forward` uses;
  * torch: the three statements with torch's modules in fp32.

The figures include the Python of both sides (the list of dicts, the output allocations).  Seeded default-initialised weights (timing
does not depend on their values).  Prints a report, writes it to --out (default profiles/detr_heads.txt) and prints one JSON line.
    python tools/bench_detr_heads.py [--rounds 7] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from hoigen_amd.detr import DetectionHeads  # noqa: E402

D, C1, Q = 256, 92, 100
CASES = [(B, L) for B in (1, 4, 8) for L in (1, 6)]


class MLP(nn.Module):
    def __init__(self, i, h, o, n):
        super().__init__()
        self.num_layers = n
        dims = [h] * (n - 1)
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip([i] + dims, dims + [o]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = torch.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


def post_process(logits, boxes, sizes):
    prob = torch.softmax(logits, -1)
    scores, labels = prob[..., :-1].max(-1)
    cx, cy, w, h = boxes.unbind(-1)
    b = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    ih, iw = sizes.unbind(1)
    b = b * torch.stack([iw, ih, iw, ih], 1)[:, None, :]
    return [{"scores": s, "labels": l, "boxes": x} for s, l, x in zip(scores, labels, b)]


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def in_turn(variants, rounds, inner):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detr_heads.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    ce, be = nn.Linear(D, C1).cuda().eval(), MLP(D, D, 4, 3).cuda().eval()
    heads = DetectionHeads.from_modules(ce, be)
    lines = [f"DETR heads + PostProcess: hg_detr_heads (one launch) against torch's fp32 modules, D = {D}, C1 = {C1}, Q = {Q}; "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} alternating rounds of {args.inner} calls, ms a call"]
    result = {}
    for B, L in CASES:
        hs = torch.randn(L, B, Q, D, device="cuda")
        sizes = [(480.0 + 8 * b, 640.0 - 8 * b) for b in range(B)]
        sizes_dev = torch.tensor(sizes, device="cuda")

        def torch_path():
            oc, ob = ce(hs), be(hs).sigmoid()
            return post_process(oc[-1], ob[-1], sizes_dev)

        t = in_turn({"native_all_levels": lambda: heads._run(hs, sizes, True), "native_detect": lambda: heads.detect(hs, sizes),
                     "torch_fp32": torch_path}, args.rounds, args.inner)
        ratio_all, ratio_det = t["torch_fp32"][0] / t["native_all_levels"][0], t["torch_fp32"][0] / t["native_detect"][0]
        lines.append(f"B = {B}, L = {L} ({L * B * Q} rows): every level {t['native_all_levels'][0]:.4f} ({t['native_all_levels'][1]:.4f} .. "
                     f"{t['native_all_levels'][2]:.4f}); detections only {t['native_detect'][0]:.4f} ({t['native_detect'][1]:.4f} .. "
                     f"{t['native_detect'][2]:.4f}); torch {t['torch_fp32'][0]:.4f} ({t['torch_fp32'][1]:.4f} .. {t['torch_fp32'][2]:.4f}); "
                     f"torch / native {ratio_all:.2f} x (every level), {ratio_det:.2f} x (detections only)"
                     + ("" if min(ratio_all, ratio_det) > 1 else "   <- NOT faster than torch"))
        result[f"B{B}_L{L}"] = {k: [round(x, 5) for x in v] for k, v in t.items()}
    lines.append("Not measured: a 16-row tile, counter profiles, DETR-R50's own weights (timing does not depend on the values).")
    report = "\n".join(lines)
    print(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report + "\n")
    print(json.dumps({"bench": "detr_heads", "ms": result}))


if __name__ == "__main__":
    main()
