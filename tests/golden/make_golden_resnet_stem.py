#!/usr/bin/env python3
"""Generates tests/golden/g23_resnet_stem.npz: the stem of the seeded ResNet of tests/resnet_cases.py (`make_resnet`) on 2 x 3 x 37 x 45
(tests/stem_cases.py `g23_input`), in fp32 - `F.conv2d` -> the reference's own `FrozenBatchNorm2d.forward` (detr/models/backbone.py:19-55)
-> ReLU -> `F.max_pool2d`.  Stored: the input `x`, `conv1.weight`, `bn1.weight` / `bias` / `running_mean` / `running_var`, the output
`out` [2, 64, 10, 12], and `out_fp32_vs_fp64_max_abs`, the distance of the fp32 run from the same statements in fp64.

The reference's backbone.py cannot be imported here (it imports torchvision), so the class is read from the reference tree by line range
at run time and executed.  Runs only where the reference is checked out (REFERENCE, default /root/reference), never on the GPU box:
    python tests/golden/make_golden_resnet_stem.py
Nothing of the reference's source is stored: the fixture holds data only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import resnet_cases as rc  # noqa: E402
import stem_bound as sb  # noqa: E402
import stem_cases as sc  # noqa: E402
from make_golden_resnet import reference_lines  # noqa: E402


def main():
    frozen = reference_lines("detr/models/backbone.py", 19, 55, {"torch": torch})["FrozenBatchNorm2d"]
    net = rc.make_resnet(norm=frozen)
    x = sc.g23_input()
    out = {"x": x.numpy(), "conv1.weight": net.conv1.weight.detach().numpy()}
    out.update({f"bn1.{k}": v.numpy() for k, v in net.bn1.state_dict().items()})
    with torch.no_grad():
        o32 = sb.reference_fp32(x, net.conv1.weight, net.bn1)
        bn64 = frozen(64).double()
        bn64.load_state_dict({k: v.double() for k, v in net.bn1.state_dict().items()})
        o64 = sb.reference_fp32(x.double(), net.conv1.weight.double(), bn64)
    d = o32.double() - o64
    out["out"] = o32.numpy()
    out["out_fp32_vs_fp64_max_abs"] = np.float64(d.abs().max())
    print(f"stem: {tuple(o32.shape)}, the fp32 run against the fp64 run: relative L2 {float(d.norm() / o64.norm()):.2e}, max abs {float(d.abs().max()):.2e}; "
          f"positive {float((o64 > 0).double().mean()):.2f}, rms {float(o64.pow(2).mean().sqrt()):.2f}")
    path = os.path.join(HERE, "g23_resnet_stem.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
