#!/usr/bin/env python3
"""Generates tests/golden/g22_resnet_stages.npz: one two-block bottleneck stage with stride 2 and a downsample, 64 -> 256 channels, on
2 x 64 x 9 x 7, in fp32 - `F.conv2d` and the reference's own `FrozenBatchNorm2d.forward` (detr/models/backbone.py:19-55) on the seeded
recipe of tests/resnet_cases.py (`g22_stage`).  Stored: the input `x`, every parameter under its state-dict key (`layer1.0.conv1.weight`,
`layer1.0.bn1.running_var`, ..), every block's output `out0`, `out1`, and `out{i}_fp32_vs_fp64_max_abs`, the distance of the fp32 run from
the same statements in fp64.

The reference's backbone.py cannot be imported here (it imports torchvision), so the class is read from the reference tree by line range
at run time and executed.  Runs only where the reference is checked out (REFERENCE, default /root/reference), never on the GPU box:
    python tests/golden/make_golden_resnet.py
Nothing of the reference's source is stored: the fixture holds data only."""
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import resnet_cases as rc  # noqa: E402

REF = os.environ.get("REFERENCE", "/root/reference")


def reference_lines(path, a, b, ns):
    """exec the 1-based inclusive lines a .. b of a file of the reference"""
    src = f"{REF}/{path}"
    lines = open(src).read().split("\n")
    exec(compile(textwrap.dedent("\n".join(lines[a - 1:b])), f"{src}:{a}-{b}", "exec"), ns)
    return ns


def main():
    frozen = reference_lines("detr/models/backbone.py", 19, 55, {"torch": torch})["FrozenBatchNorm2d"]
    stage, x = rc.g22_stage(norm=frozen)
    out = {"x": x.numpy()}
    out.update({k: v.numpy() for k, v in stage.state_dict().items()})
    with torch.no_grad():
        t32, t64 = x, x.double()
        stage64 = rc.g22_stage(norm=frozen)[0].double()
        for i, (b32, b64) in enumerate(zip(stage.layer1, stage64.layer1)):
            t32, t64 = b32(t32), b64(t64)
            out[f"out{i}"] = t32.numpy()
            d = t32.double() - t64
            out[f"out{i}_fp32_vs_fp64_max_abs"] = np.float64(d.abs().max())
            print(f"block {i}: {tuple(t32.shape)}, the fp32 run against the fp64 run: relative L2 {float(d.norm() / t64.norm()):.2e}, "
                  f"max abs {float(d.abs().max()):.2e}; positive {float((t64 > 0).double().mean()):.2f}, rms {float(t64.pow(2).mean().sqrt()):.2f}")
    path = os.path.join(HERE, "g22_resnet_stages.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
