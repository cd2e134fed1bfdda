#!/usr/bin/env python3
"""Times the ResNet stem on the HIP path (hoigen_amd.resnet.ResNetStem: hg_resnet_stem, and NativeBody(native_stem=True): hg_resnet_body;
DESIGN.md section 21) against the paths it replaces, on the same tensors, in turn: 7 rounds of 20 calls, median (min .. max), ms a
call, the Python of both sides included.

(a) the stem alone: hg_resnet_stem against the stand-in's conv1, bn1, relu, maxpool in torch fp32;
(b) the body: NativeBody(native_stem=True) against NativeBody(native_stem=False) - the torch stem in front of the native stages, which
    is the path before the native stem existed.
Shapes: 3 x 800 x 1 333 at B = 1, 4, 8 (the detector's view) and 3 x 224 x 224 at B = 64 (the DINO use).  The stem launch alone: the
project's profiler (HG_PROF_RESNET_STEM, one record per launch) over 5 calls of the body, with the bytes it must move (the fp32 images
read once, the NHWC fp32 + fp16 pair written once) over that time.

Timing does not depend on the weights' values.  Prints a report, writes it to --out (default profiles/resnet_stem.txt) and prints one
JSON line.
    python tools/bench_resnet_stem.py [--rounds 7] [--inner 20] [--cases detr1,detr4,detr8,dino64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
import resnet_cases as rc  # noqa: E402
from bench_resnet_stages import fmt, in_turn, verdict  # noqa: E402
from hoigen_amd import _lib  # noqa: E402
from hoigen_amd.resnet import NativeBody, ResNetStem  # noqa: E402

# name -> (B, Hi, Wi)
CASES = {"detr1": (1, 800, 1333), "detr4": (4, 800, 1333), "detr8": (8, 800, 1333), "dino64": (64, 224, 224)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resnet_stem.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    net = rc.make_resnet().cuda()
    stem = ResNetStem.from_module(net).cuda()
    body_native = NativeBody.from_module(net, native_stem=True).cuda()
    body_parent = NativeBody.from_module(net).cuda()
    lines = [f"ResNet-50 stem: (a) hg_resnet_stem against conv1, bn1, relu, maxpool in torch fp32; (b) the body with the native stem (hg_resnet_body) "
             f"against the torch stem in front of the native stages; {torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} "
             f"alternating rounds of {args.inner} calls, ms a call"]
    result = {}
    for name in args.cases.split(","):
        B, Hi, Wi = CASES[name]
        x = torch.randn(B, 3, Hi, Wi, device="cuda") * 1.2

        def torch_stem():
            return net.maxpool(net.relu(net.bn1(net.conv1(x))))

        got, want = stem(x), torch_stem()
        rel = float((got - want).norm() / want.norm())
        gb, wb = body_native(x)["0"], body_parent(x)["0"]
        rel_b = float((gb - wb).norm() / wb.norm())
        ta = in_turn({"native": lambda: stem(x), "torch_fp32": torch_stem}, args.rounds, args.inner)
        tb = in_turn({"native_stem": lambda: body_native(x), "torch_stem": lambda: body_parent(x)}, args.rounds, args.inner)
        lines.append(f"{name}: B = {B}, 3 x {Hi} x {Wi} -> stem map {tuple(got.shape[1:])}, body map {tuple(gb.shape[1:])}; native stem against torch fp32 "
                     f"rel L2 {rel:.2e}; body against the torch-stem body rel L2 {rel_b:.2e}")
        lines.append(f"  (a) stem alone: native {fmt(ta['native'])}; torch fp32 {fmt(ta['torch_fp32'])}: {verdict(ta['native'], ta['torch_fp32'])}")
        lines.append(f"  (b) body: native stem {fmt(tb['native_stem'])}; torch stem {fmt(tb['torch_stem'])}: {verdict(tb['native_stem'], tb['torch_stem'])}")
        h = body_native.stages._ctx.get(x.device)
        calls = 5
        _, recs = _lib.profile(h, _lib.HG_PROF_RESNET_STEM, calls, lambda: [body_native(x) for _ in range(calls)])
        assert len(recs) == calls, len(recs)
        ms = statistics.median(r[4] for r in recs)
        nbytes = x.numel() * 4 + got.numel() * 6
        flop = 2.0 * got.numel() * 4 * 147      # four conv pixels a pooled pixel, without the halo's recompute
        lines.append(f"  the stem launch alone (HG_PROF_RESNET_STEM, median of {calls}): {ms * 1e3:.0f} us; {nbytes / 1e6:.1f} MB it must move "
                     f"({x.numel() * 4 / 1e6:.1f} read, {got.numel() * 6 / 1e6:.1f} written) = {nbytes / (ms * 1e-3) / 1e9:.0f} GB/s; {flop / 1e9:.1f} GFLOP of the "
                     f"conv map = {flop / (ms * 1e-3) / 1e12:.1f} TFLOP/s")
        result[name] = {"stem": {k: [round(v, 4) for v in val] for k, val in ta.items()}, "body": {k: [round(v, 4) for v in val] for k, val in tb.items()},
                        "rel_l2": rel, "stem_launch_ms": round(ms, 4), "stem_gb_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
        del x, got, want, gb, wb
        torch.cuda.empty_cache()
    lines.append("Not measured: counter profiles of the stem kernel, tile shapes other than 4 x 8 pooled pixels, ResNet-50's own weights (timing does not "
                 "depend on the values), a second box.")
    report = "\n".join(lines)
    print(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report + "\n")
    print(json.dumps({"bench": "resnet_stem", "ms": result}))


if __name__ == "__main__":
    main()
