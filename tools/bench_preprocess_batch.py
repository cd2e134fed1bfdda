#!/usr/bin/env python
"""Time hg_preprocess_batch (one call for the crops of a batch of images) against what exists without it.

    python tools/bench_preprocess_batch.py [--reps 60] [--out profiles/preprocess_batch.txt]

(a) one CropPreprocessor.batch() call (check=False: nothing is copied back) against the loop of per-image CropPreprocessor calls
    (hg_preprocess_crops: host geometry, an upload and a host wait per image), 4 / 16 / 64 images of 480 x 640 with 3 and 12 crops each:
    wall clock from the first call to the end of a device synchronise, the loop's host waits included; and the two launches of the
    batch call alone (the C call with every input already on the device) by device events.
(b) the 256 boxes of one 480 x 640 image of tools/bench_preprocess.py: the two launches of hg_preprocess_batch against the three of
    hg_preprocess_crops on the same boxes, by device events (the per-image call's upload and host wait sit inside its events).
(d) larger downscales, where the bands of the fused kernel shrink: 64 square boxes of 896, 1792 and 3584 pixels (downscales 4, 8, 16: bands
    of 14, 5 and 1 output rows) of one 3584 x 3584 image, the same two legs as (b).
(c) records.emit_records against the loop of records.emit_record on the synthetic ViT-B/16, 20 images x 4 pairs, end to end, wall clock.

Legs alternating, median and minimum over --reps rounds after 5 warm-up rounds; 1 GPU.

--trace N runs nothing but the two legs of (b) N times each, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_preprocess_batch.py --trace 50
gives the three kernels of hg_preprocess_crops and the two of hg_preprocess_batch without the host part of either call."""
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

from hoigen_amd import _lib, preprocess, records   # noqa: E402

torch.set_grad_enabled(False)
DEV = torch.device("cuda:0")
H, W = 480, 640


def boxes_of(rng, n):
    out = []
    for _ in range(n):
        x0, y0 = rng.randint(0, W - 60), rng.randint(0, H - 60)
        out.append((x0, y0, min(W, x0 + rng.randint(40, 320)), min(H, y0 + rng.randint(40, 280))))
    return np.asarray(out, np.int32)


def timed(legs, reps, wall, warmup=5):
    """wall: host clock around fn() + synchronise (ms); else device events around fn()"""
    out = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            if wall:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            if r >= warmup:
                out[k].append(ms)
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def c_call(images, boxes_d, owner_d, n, n_px, out, status):
    """the C call alone, every input resident"""
    nb = len(images)
    a = _lib.hg_preprocess_batch_args(
        (ctypes.c_void_p * nb)(*[im.data_ptr() for im in images]), (ctypes.c_int32 * nb)(*[im.shape[0] for im in images]),
        (ctypes.c_int32 * nb)(*[im.shape[1] for im in images]), nb, boxes_d.data_ptr(), owner_d.data_ptr(), n, n_px, 0, 0, out.data_ptr(), None,
        status.data_ptr())
    lib, handle, stream = _lib.lib(), _lib.ctx(0), torch.cuda.current_stream().cuda_stream

    def fn():
        rc = lib.hg_preprocess_batch(handle, ctypes.byref(a), stream)
        assert rc == 0, rc
    return fn


def fmt(p):
    return f"{p[0]:8.3f} ({p[1]:7.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    pre = preprocess.CropPreprocessor(224)
    prop = torch.cuda.get_device_properties(0)
    lines = [f"1 x {prop.name} ({getattr(prop, 'gcnArchName', '?').split(':')[0]}, {prop.multi_processor_count} CUs), python tools/bench_preprocess_batch.py --reps {args.reps}",
             f"median (min) of {args.reps} alternating rounds after 5 warm-up rounds; 480 x 640 images, n_px 224",
             "", "(a) one batch() call against the loop of per-image calls: wall clock ms, host waits included; launches: the C call alone, device events",
             "images crops/img crops |        batch() ms             loop ms loop/batch |    2 launches ms"]
    images = [torch.from_numpy(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).to(DEV) for _ in range(64)]
    for B in (() if args.trace else (4, 16, 64)):
        for per in (3, 12):
            bx = [boxes_of(rng, per) for _ in range(B)]
            imgs = images[:B]
            want = torch.cat([pre(i, b) for i, b in zip(imgs, bx)])
            got, status = pre.batch(imgs, bx, check=False)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not status.any()
            n = B * per
            out = torch.empty(n, 3, 224, 224, device=DEV)
            st = torch.zeros(n, dtype=torch.int32, device=DEV)
            bd = torch.from_numpy(np.concatenate(bx)).to(DEV)
            od = torch.from_numpy(np.repeat(np.arange(B), per).astype(np.int32)).to(DEV)
            w = timed({"batch": lambda: pre.batch(imgs, bx, check=False), "loop": lambda: [pre(i, b) for i, b in zip(imgs, bx)]}, args.reps, True)
            d = timed({"launches": c_call(imgs, bd, od, n, 224, out, st)}, args.reps, False)
            assert torch.equal(out.view(torch.int32), want.view(torch.int32))
            lines.append(f"{B:6d} {per:9d} {n:5d} | {fmt(w['batch'])}  {fmt(w['loop'])} {w['loop'][0] / w['batch'][0]:10.2f} | {fmt(d['launches'])}")
    # (b)
    rng = np.random.RandomState(0)
    img = torch.from_numpy(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).to(DEV)
    boxes = boxes_of(rng, 256)
    want = pre(img, boxes)
    out = torch.empty(256, 3, 224, 224, device=DEV)
    st = torch.zeros(256, dtype=torch.int32, device=DEV)
    if args.trace:
        fn = c_call([img], torch.from_numpy(boxes).to(DEV), torch.zeros(256, dtype=torch.int32, device=DEV), 256, 224, out, st)
        for _ in range(args.trace):
            fn()
            pre(img, boxes)
        torch.cuda.synchronize()
        return
    d = timed({"batch": c_call([img], torch.from_numpy(boxes).to(DEV), torch.zeros(256, dtype=torch.int32, device=DEV), 256, 224, out, st),
               "crops": lambda: pre(img, boxes)}, args.reps, False)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    lines += ["", "(b) the 256 boxes of one 480 x 640 image (tools/bench_preprocess.py): device events, ms",
              " hg_preprocess_batch (2 launches)   hg_preprocess_crops (upload, wait, 3 launches)   batch/crops",
              f"        {fmt(d['batch'])}                  {fmt(d['crops'])}               {d['batch'][0] / d['crops'][0]:8.2f}"]
    # (d)
    big = torch.from_numpy(rng.randint(0, 256, size=(3584, 3584, 3)).astype(np.uint8)).to(DEV)
    lines += ["", "(d) 64 square boxes of one 3584 x 3584 image at larger downscales (shrunk bands): device events, ms",
              " side  scale | hg_preprocess_batch   hg_preprocess_crops   batch/crops"]
    out64, st64, zero64 = torch.empty(64, 3, 224, 224, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV)
    for side in (896, 1792, 3584):
        x0, y0 = rng.randint(0, 3584 - side + 1, 64), rng.randint(0, 3584 - side + 1, 64)
        bx = np.stack([x0, y0, x0 + side, y0 + side], 1).astype(np.int32)
        want = pre(big, bx)
        d = timed({"batch": c_call([big], torch.from_numpy(bx).to(DEV), zero64, 64, 224, out64, st64), "crops": lambda: pre(big, bx)}, args.reps, False)
        assert torch.equal(out64.view(torch.int32), want.view(torch.int32)) and not st64.any()
        lines.append(f"{side:5d} {side / 224:6.1f} |   {fmt(d['batch'])}    {fmt(d['crops'])}   {d['batch'][0] / d['crops'][0]:11.2f}")
    # (c)
    from hoigen_amd import synth
    from hoigen_amd.model import build_model
    m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).float().to(DEV)
    imgs = images[:20]
    ann = []
    for _ in imgs:
        bh, bo = boxes_of(rng, 4).astype(np.float32), boxes_of(rng, 4).astype(np.float32)
        ann.append(dict(boxes_h=bh, boxes_o=bo, verbs=[1, 2, 3, 4], objects=[5, 6, 7, 8]))
    w = timed({"emit_records": lambda: records.emit_records(m, imgs, ann), "loop": lambda: [records.emit_record(m, i, **a) for i, a in zip(imgs, ann)]},
              args.reps, True)
    lines += ["", f"(c) records of 20 images x 4 pairs (240 crops) on the synthetic ViT-B/16, end to end: wall clock ms, median (min) of {args.reps} rounds",
              "      emit_records ms   loop of emit_record ms   loop/emit_records",
              f"   {fmt(w['emit_records'])}        {fmt(w['loop'])}   {w['loop'][0] / w['emit_records'][0]:17.2f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
