#!/usr/bin/env python3
"""Times hg_detector_views on one MI355X and writes the table of profiles/detector_views.txt.

    python tools/bench_detector_views.py [--rounds 60] [--out profiles/detector_views.txt]

Legs alternate inside every round; median (minimum) of `--rounds` rounds after warm-up of every shape:

  * 480 x 640 images at B = 1, 4, 8, 64, at (800, 1333, 224): the C call between device events, the façade's wall clock (ending in a
    device synchronise), the CLIP leg alone as CropPreprocessor.batch on the same resized images, and - where Pillow imports - the CPU
    pipeline the call replaces, per image: two PIL resizes, two normalisations in torch, the pad copy;
  * the C call without the CLIP view (clip_px 0: the two kernels of hg_detector_views.hip alone) and its output bytes per second - the
    resized bytes, the fp32 planes and the mask - against the HBM roofline (8 TB/s spec, 6.3 TB/s achievable: a float4 copy);
  * one row each at a downscale of 4 and of 12 (B = 8).
There is no CPU fallback: without a HIP device this fails."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from hoigen_amd import _lib, detector_views, preprocess  # noqa: E402

MEAN, STD = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


def image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def cpu_pipeline(imgs, size, max_size, n):
    """the reference's host path for these images: two PIL resizes, two normalisations, the pad copy"""
    from PIL import Image
    sizes, hm, wm, _ = detector_views.view_shapes([i.shape[0] for i in imgs], [i.shape[1] for i in imgs], size, max_size)
    out = torch.zeros(len(imgs), 3, hm, wm)
    mask = torch.ones(len(imgs), hm, wm, dtype=torch.bool)
    clips = []
    for b, (im, (oh, ow)) in enumerate(zip(imgs, sizes)):
        r = Image.fromarray(im).resize((ow, oh), Image.BICUBIC)
        c = r.resize((n, n), Image.BICUBIC)
        t = (torch.from_numpy(np.array(r)).permute(2, 0, 1).float().div(255) - MEAN) / STD
        clips.append((torch.from_numpy(np.array(c)).permute(2, 0, 1).float().div(255) - MEAN) / STD)
        out[b, :, :oh, :ow].copy_(t)
        mask[b, :oh, :ow] = False
    return out, mask, torch.stack(clips)


def fmt(xs):
    return f"{statistics.median(xs):9.1f} ({min(xs):8.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_views: needs a HIP device (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    size, max_size, n = 800, 1333, 224
    rows = [("480x640", 480, 640, B, size, max_size) for B in (1, 4, 8, 64)] + [("down 4: 1600x2132 -> 400x533", 1600, 2132, 8, 400, 0),
                                                                                ("down 12: 1920x2560 -> 160x213", 1920, 2560, 8, 160, 0)]
    lib, handle = _lib.lib(), _lib.ctx(0)
    lines = [f"hg_detector_views, clip_px {n}; microseconds, median (minimum) of {args.rounds} rounds after warm-up, legs alternating", "",
             f"{'images':32s} {'B':>3s} | {'C call (device events)':>22s} | {'same, clip_px 0':>22s} | {'facade (wall)':>20s} | {'CLIP leg: CropPreprocessor.batch':>32s} | "
             f"{'CPU pipeline / image':>22s} | clip_px 0 call: out GB/s (of 6300)"]
    for name, h, w, B, sz, mx in rows:
        host = [image(h, w, 10 + b) for b in range(B)]
        imgs = [torch.from_numpy(i).to(dev) for i in host]
        dv = detector_views.DetectorViews(sz, mx, n)
        sizes, hm, wm, off = detector_views.view_shapes([h] * B, [w] * B, sz, mx)
        t = torch.empty(B, 3, hm, wm, device=dev)
        m = torch.empty(B, hm, wm, dtype=torch.uint8, device=dev)
        c = torch.empty(B, 3, n, n, device=dev)
        u = torch.empty(int(off[B]), dtype=torch.uint8, device=dev)
        a = _lib.hg_detector_views_args((ctypes.c_void_p * B)(*[i.data_ptr() for i in imgs]), (ctypes.c_int32 * B)(*[h] * B),
                                        (ctypes.c_int32 * B)(*[w] * B), B, sz, mx, n, 0, 0, u.data_ptr(), t.data_ptr(), m.data_ptr(), c.data_ptr())
        a0 = _lib.hg_detector_views_args((ctypes.c_void_p * B)(*[i.data_ptr() for i in imgs]), (ctypes.c_int32 * B)(*[h] * B),
                                         (ctypes.c_int32 * B)(*[w] * B), B, sz, mx, 0, 0, 0, u.data_ptr(), t.data_ptr(), m.data_ptr(), None)
        stream = torch.cuda.current_stream().cuda_stream
        resized = [u[int(off[b]):int(off[b]) + oh * ow * 3].view(oh, ow, 3) for b, (oh, ow) in enumerate(sizes)]
        crop = preprocess.CropPreprocessor(n, stretch=True, imagenet_norm=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def c_call(args=a):
            e0.record()
            _lib.check(0, lib.hg_detector_views(handle, ctypes.byref(args), stream), "hg_detector_views")
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6

        legs = {"c": c_call, "c0": lambda: c_call(a0), "facade": lambda: wall(lambda: dv(imgs)), "clip": lambda: wall(lambda: crop.batch(resized, check=False))}
        cpu_rounds = max(3, min(args.rounds, 200 // B)) if have_pil else 0
        for _ in range(5):
            for f in legs.values():
                f()
        got = {k: [] for k in legs}
        cpu = []
        for r in range(args.rounds):
            for k, f in legs.items():
                got[k].append(f())
            if r < cpu_rounds:
                t0 = time.perf_counter()
                cpu_pipeline(host, sz, mx, n)
                cpu.append((time.perf_counter() - t0) * 1e6 / B)
        out_bytes = sum(oh * ow * 3 for oh, ow in sizes) + B * hm * wm * (12 + 1)      # resized bytes, fp32 planes, mask: the clip_px 0 call
        gbs = out_bytes / (statistics.median(got["c0"]) * 1e-6) / 1e9
        lines.append(f"{name:32s} {B:3d} | {fmt(got['c']):>22s} | {fmt(got['c0']):>22s} | {fmt(got['facade']):>20s} | {fmt(got['clip']):>32s} | "
                     f"{(fmt(cpu) if cpu else 'Pillow not installed'):>22s} | {gbs:8.1f} ({100 * gbs / 6300:4.1f} %)")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
