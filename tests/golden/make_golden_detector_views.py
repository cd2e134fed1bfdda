#!/usr/bin/env python3
"""Generates tests/golden/g17_detector_views.npz: the detector's two views of the cases of tests/detector_views_cases.py at the setting
`a` (size 40, max_size 66, clip_px 16), made by Pillow itself and by the reference's own lines:

  * the output size of every image: get_size_with_aspect_ratio, detr/datasets/transforms_clip.py:142-161, executed from the reference;
  * the resized image: `Image.resize((ow, oh), Image.BICUBIC)` - what F.resize(image, size, interpolation=Image.BICUBIC) calls for a
    PIL image (transforms_clip.py:170; torchvision is not installed here) - and the CLIP view, the same call on THAT image
    (IResize([n, n]), transforms_clip.py:279-288);
  * the targets: boxes scaled and `size` set by transforms_clip.py:175-204, executed from the reference on seeded fp32 boxes.

Runs only where the reference is checked out (REFERENCE, default /root/reference), never on the GPU box:
    python tests/golden/make_golden_detector_views.py
Nothing of the reference's source is stored: the fixture holds data only.  The inputs are not stored either: they are the seeded images
of detector_views_cases.image."""
import os
import sys
import textwrap

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import detector_views_cases as dc  # noqa: E402

REF = os.environ.get("REFERENCE", "/root/reference")
SRC = f"{REF}/detr/datasets/transforms_clip.py"


def reference_lines(a, b, ns):
    """exec the 1-based inclusive lines a .. b of transforms_clip.py (the body of `resize`, which cannot be imported without torchvision)"""
    lines = open(SRC).read().split("\n")
    exec(compile(textwrap.dedent("\n".join(lines[a - 1:b])), f"{SRC}:{a}-{b}", "exec"), ns)
    return ns


def main():
    size, max_size, n = dc.SETTINGS["a"]
    rule = reference_lines(142, 161, {})["get_size_with_aspect_ratio"]
    rng = np.random.RandomState(20241117)
    out = {"setting": np.asarray([size, max_size, n], np.int32)}
    for name in dc.NAMES:
        img = dc.image("a", name)
        pil = Image.fromarray(img)
        oh, ow = rule(pil.size, size, max_size)
        resized = pil.resize((ow, oh), Image.BICUBIC)
        h, w = img.shape[:2]
        boxes = (rng.rand(3, 4) * [w, h, w, h]).astype(np.float32)
        target = {"boxes": torch.from_numpy(boxes.copy()), "boxes_h": torch.from_numpy(boxes[:2].copy()), "boxes_o": torch.from_numpy(boxes[1:].copy())}
        ns = reference_lines(175, 204, {"torch": torch, "rescaled_image": resized, "image": pil, "target": target, "size": (oh, ow)})
        assert ns["target"] is not target and tuple(ns["target"]["size"].tolist()) == (oh, ow)
        out[f"{name}_size"] = np.asarray([oh, ow], np.int32)
        out[f"{name}_u8"] = np.asarray(resized.convert("RGB"), np.uint8)
        out[f"{name}_clip_u8"] = np.asarray(resized.resize((n, n), Image.BICUBIC).convert("RGB"), np.uint8)
        out[f"{name}_boxes_in"] = boxes
        for k in ("boxes", "boxes_h", "boxes_o"):
            assert ns["target"][k].dtype == torch.float32
            out[f"{name}_{k}"] = ns["target"][k].numpy()
        out[f"{name}_target_size"] = ns["target"]["size"].numpy()
    path = os.path.join(HERE, "g17_detector_views.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
