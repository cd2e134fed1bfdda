#!/usr/bin/env python3
"""Times the ResNet bottleneck stages on the HIP path (hoigen_amd.resnet.ResNetStages: hg_resnet_stages) against
the same stand-in ResNet-50 modules in torch on the same tensors, in turn: 7 rounds of 20 calls, median (min .. max), ms a call, the
Python of both sides included.

Shapes: the stem's map of the 800 x 1 333 view (64 x 200 x 334) at B = 1, 4, 8; the DINO use (64 x 56 x 56) at B = 64; layer4 alone from
a 1024 x 50 x 84 map at B = 4.  Torch side: the stand-in modules of tests/resnet_cases.py (frozen norms, seeded recipe) in fp32 - what
the reference runs, and what the claim is made against; a second, informational row runs them in fp16 channels_last.  Per convolution:
the project's profiler (HG_PROF_RESNET_CONV, one record per launch) over 5 calls, summed per level, with the fraction of the dense fp16
MFMA peak (2 517 TFLOP/s: 16 x the 157.3 TFLOP/s fp32 figure of the hardware guide - a spec figure, not measured here).

Timing does not depend on the weights' values.  Prints a report, writes it to --out (default profiles/resnet_stages.txt) and prints one
JSON line.
    python tools/bench_resnet_stages.py [--rounds 7] [--inner 20] [--cases detr1,detr4,detr8,dino64,layer4]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import resnet_cases as rc  # noqa: E402
from hoigen_amd import _lib  # noqa: E402
from hoigen_amd.resnet import ResNetStages  # noqa: E402

PEAK = 16 * 157.3e12
# name -> (B, C, H, W, levels)
CASES = {"detr1": (1, 64, 200, 334, (1, 4)), "detr4": (4, 64, 200, 334, (1, 4)), "detr8": (8, 64, 200, 334, (1, 4)),
         "dino64": (64, 64, 56, 56, (1, 4)), "layer4": (4, 1024, 50, 84, (4, 4))}


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
    return f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"


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
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resnet_stages.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    net = rc.make_resnet().cuda()
    net16 = rc.make_resnet().cuda().half().to(memory_format=torch.channels_last)
    lines = [f"ResNet-50 bottleneck stages: hg_resnet_stages against the same modules in torch (fp32: the claim; fp16 channels_last: informational); "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} alternating rounds of {args.inner} calls, ms a call"]
    result = {}
    for name in args.cases.split(","):
        B, Cc, H, W, levels = CASES[name]
        m = ResNetStages.from_module(net, levels=levels).cuda()
        layers = [getattr(net, f"layer{i}") for i in range(levels[0], levels[1] + 1)]
        layers16 = [getattr(net16, f"layer{i}") for i in range(levels[0], levels[1] + 1)]
        x = torch.randn(B, Cc, H, W, device="cuda").relu()
        x16 = x.half().contiguous(memory_format=torch.channels_last)

        def torch32():
            t = x
            for l in layers:
                t = l(t)
            return t

        def torch16():
            t = x16
            for l in layers16:
                t = l(t)
            return t

        got, want = m(x), torch32()
        rel = float((got - want).norm() / want.norm())
        t = in_turn({"native": lambda: m(x), "torch_fp32": torch32, "torch_fp16_cl": torch16}, args.rounds, args.inner)
        lines.append(f"{name}: B = {B}, {Cc} x {H} x {W}, layer{levels[0]} .. layer{levels[1]} -> {tuple(got.shape[1:])}; native against torch fp32 rel L2 {rel:.2e}")
        lines.append(f"  native {fmt(t['native'])}; torch fp32 {fmt(t['torch_fp32'])}: {verdict(t['native'], t['torch_fp32'])}")
        lines.append(f"  torch fp16 channels_last {fmt(t['torch_fp16_cl'])} (informational): {verdict(t['native'], t['torch_fp16_cl'])}")
        result[name] = {k: [round(v, 4) for v in val] for k, val in t.items()}
        result[name]["rel_l2"] = rel
        # per convolution, summed per level
        h = m._ctx.get(x.device)
        n_conv = sum(4 if b.downsample is not None else 3 for b in m.blocks())
        calls = 5
        _, recs = _lib.profile(h, _lib.HG_PROF_RESNET_CONV, n_conv * calls, lambda: [m(x) for _ in range(calls)])
        assert len(recs) == n_conv * calls, (len(recs), n_conv)
        per = [statistics.median(recs[i + n_conv * c][4] for c in range(calls)) for i in range(n_conv)]
        i, total_ms, total_fl = 0, 0.0, 0.0
        worst = None
        for lname in m.level_names:
            ms = fl = 0.0
            for b in getattr(m, lname):
                for _ in range(4 if b.downsample is not None else 3):
                    _, M, N, K, _ = recs[i]
                    f = 2.0 * M * N * K
                    ms, fl = ms + per[i], fl + f
                    share = f / (per[i] * 1e-3) / PEAK
                    if worst is None or per[i] > worst[0]:
                        worst = (per[i], lname, M, N, K, share)
                    i += 1
            lines.append(f"  {lname}: convolutions {ms:.3f} ms, {fl / 1e9:.1f} GFLOP, {fl / (ms * 1e-3) / 1e12:.1f} TFLOP/s = {fl / (ms * 1e-3) / PEAK:.1%} of the dense fp16 peak")
            total_ms, total_fl = total_ms + ms, total_fl + fl
        lines.append(f"  all {n_conv} convolutions {total_ms:.3f} ms ({total_fl / 1e9:.1f} GFLOP, {total_fl / (total_ms * 1e-3) / PEAK:.1%} of peak) of the call's "
                     f"{t['native'][0]:.3f} ms; the slowest launch: {worst[0] * 1e3:.0f} us in {worst[1]}, M {worst[2]} N {worst[3]} K {worst[4]}, {worst[5]:.1%} of peak")
        result[name]["conv_ms"] = round(total_ms, 4)
        del m
        torch.cuda.empty_cache()
    lines.append("Not measured: counter profiles of the convolution kernel, tile shapes other than 32 / 128 x 64, ResNet-50's own weights (timing does not depend on the values).")
    report = "\n".join(lines)
    print(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report + "\n")
    print(json.dumps({"bench": "resnet_stages", "ms": result}))


if __name__ == "__main__":
    main()
