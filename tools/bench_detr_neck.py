#!/usr/bin/env python3
"""Times the DETR neck on the HIP path (hoigen_amd.detr.DetectorNeck: one hg_detr_neck call) against the statements
it replaces as torch runs them on the same tensors (upt_tip_cache_model_free_finetune_distill3.py:1594-1597 and the two transposes of
hoigen_amd.detr.Transformer.forward): fp32 Conv2d, an independent torch statement of the sine embedding, F.interpolate for the mask and
`flatten(2).transpose(1, 2).contiguous()` of src and pos.

Shapes: Cin 2048, D 256, (B, grid) in {(1, 25 x 38), (4, 25 x 38), (2, 38 x 38), (8, 25 x 42)}, images 32 times the grid less 11 x 5
pixels, the second and later images padded.  For each, in turn, round after round, each timed with a pair of events around `--inner`
calls that end in a synchronise; median and min .. max over the rounds, the Python of both sides included:

  * the neck: native call against torch;
  * the chain: neck + `Transformer.forward_tokens` against torch's neck statements + `Transformer.forward` (six + six layers, 100 queries);
  * the kernel(s) alone from the project's profiler (HG_PROF_DETR_NECK brackets the launch and, under a split, the launch that adds the
    partial sums) for detr_neck_split = 1, 2, 4, 8, 16, 32: median (min .. max) of 20 calls, and x's bytes over the median.

"Faster" is said only where the gap between the medians exceeds three times the larger spread (max - min).  Seeded default-initialised
weights (timing does not depend on their values).  Prints a report, writes it to --out (default profiles/detr_neck.txt) and prints one
JSON line.
    python tools/bench_detr_neck.py [--rounds 7] [--inner 20]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from hoigen_amd import _lib  # noqa: E402
from hoigen_amd.detr import DetectorNeck, Transformer  # noqa: E402

CIN, D, Q = 2048, 256, 100
CASES = [(1, 25, 38), (4, 25, 38), (2, 38, 38), (8, 25, 42)]
SPLITS = (1, 2, 4, 8, 16, 32)


class Sine(nn.Module):
    """PositionEmbeddingSine's arithmetic written independently in torch (normalize = True)"""

    def __init__(self, num_pos_feats=128, temperature=10000, normalize=True, scale=2 * math.pi):
        super().__init__()
        self.num_pos_feats, self.temperature, self.normalize, self.scale = num_pos_feats, temperature, normalize, scale

    def forward(self, mask):
        free = (~mask).float()
        ys, xs = free.cumsum(1), free.cumsum(2)
        ys = ys / (ys[:, -1:, :] + 1e-6) * self.scale
        xs = xs / (xs[:, :, -1:] + 1e-6) * self.scale
        k = torch.arange(self.num_pos_feats, dtype=torch.float32, device=mask.device)
        t = self.temperature ** (2 * torch.div(k, 2, rounding_mode="floor") / self.num_pos_feats)
        px, py = xs[..., None] / t, ys[..., None] / t
        px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), 4).flatten(3)
        py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), 4).flatten(3)
        return torch.cat((py, px), 3).permute(0, 3, 1, 2)


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


def fmt(v):
    return f"{v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})"


def verdict(native, torch_):
    gap, spread = torch_[0] - native[0], max(native[2] - native[1], torch_[2] - torch_[1])
    if gap > 3 * spread:
        return f"native faster, {torch_[0] / native[0]:.2f} x"
    if -gap > 3 * spread:
        return f"native SLOWER, {torch_[0] / native[0]:.2f} x"
    return f"no difference beyond three spreads (torch / native {torch_[0] / native[0]:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detr_neck.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    conv, sine = nn.Conv2d(CIN, D, 1).cuda().eval(), Sine(D // 2)
    neck = DetectorNeck.from_modules(conv, sine)
    tr = Transformer(D, 8, 6, 6, 2048, True).cuda().eval()
    neck._ctx = tr.encoder._ctx
    query = torch.randn(Q, D, device="cuda")
    lines = [f"DETR neck: hg_detr_neck against torch (fp32 Conv2d + sine embedding + F.interpolate + two transposes), Cin = {CIN}, D = {D}; "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} alternating rounds of {args.inner} calls, ms a call"]
    result = {}
    for B, H, W in CASES:
        Hi, Wi = 32 * H - 11, 32 * W - 5
        x = torch.randn(B, CIN, H, W, device="cuda").relu()
        im = torch.zeros(B, Hi, Wi, dtype=torch.bool, device="cuda")
        for b in range(1, B):
            im[b, Hi - 40 * b:], im[b, :, Wi - 56 * b:] = True, True

        def torch_neck():
            mask = F.interpolate(im[None].float(), size=(H, W)).to(torch.bool)[0]
            pos, src = sine(mask), conv(x)
            return (src.flatten(2).transpose(1, 2).contiguous(), pos.flatten(2).transpose(1, 2).contiguous(), mask.flatten(1))

        def torch_chain():
            mask = F.interpolate(im[None].float(), size=(H, W)).to(torch.bool)[0]
            return tr(conv(x), mask, query, sine(mask))

        def native_chain():
            src, pos, mask, hw = neck(x, im)
            return tr.forward_tokens(src, mask, query, pos, hw)

        neck.set_option("detr_neck_split", 0)
        t = in_turn({"native_neck": lambda: neck(x, im), "torch_neck": torch_neck, "native_chain": native_chain, "torch_chain": torch_chain},
                    args.rounds, args.inner)
        lines.append(f"B = {B}, grid {H} x {W} ({B * H * W} tokens, x {x.numel() * 4 / 1e6:.1f} MB):")
        lines.append(f"  neck   native {fmt(t['native_neck'])}; torch {fmt(t['torch_neck'])}: {verdict(t['native_neck'], t['torch_neck'])}")
        lines.append(f"  chain  neck + forward_tokens {fmt(t['native_chain'])}; torch neck + Transformer.forward {fmt(t['torch_chain'])}: "
                     f"{verdict(t['native_chain'], t['torch_chain'])}")
        result[f"B{B}_{H}x{W}"] = {k: [round(v, 5) for v in val] for k, val in t.items()}
        h = neck._ctx.get(x.device)
        kern = {}
        for sp in SPLITS:
            neck.set_option("detr_neck_split", sp)
            neck(x, im)
            _, recs = _lib.profile(h, _lib.HG_PROF_DETR_NECK, 20, lambda: [neck(x, im) for _ in range(20)])
            ms = [r[4] for r in recs]
            kern[sp] = (statistics.median(ms), min(ms), max(ms))
            lines.append(f"  kernel(s) alone, detr_neck_split = {sp:2d}: {kern[sp][0] * 1e3:7.1f} us ({kern[sp][1] * 1e3:.1f} .. {kern[sp][2] * 1e3:.1f}), "
                         f"x's bytes / time = {x.numel() * 4 / (kern[sp][0] * 1e-3) / 1e12:.2f} TB/s")
        neck.set_option("detr_neck_split", 0)
        neck(x, im)
        _, recs = _lib.profile(h, _lib.HG_PROF_DETR_NECK, 20, lambda: [neck(x, im) for _ in range(20)])
        lines.append(f"  the default rule picks {recs[0][2]} slice(s): {statistics.median(r[4] for r in recs) * 1e3:.1f} us")
        result[f"B{B}_{H}x{W}"]["kernel_us_by_split"] = {sp: [round(v * 1e3, 2) for v in val] for sp, val in kern.items()}
    lines.append("HBM rate the guides quote for this part: about 6.3 TB/s (a guide figure, not measured here).")
    lines.append("Not measured: other token tiles than 32, counter profiles, DETR-R50's own weights (timing does not depend on the values).")
    report = "\n".join(lines)
    print(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report + "\n")
    print(json.dumps({"bench": "detr_neck", "ms": result}))


if __name__ == "__main__":
    main()
