#!/usr/bin/env python
"""Time the DINO branch in one process: ResNetFeatures (hg_resnet_features: stem, stages, pool + normalise) against the same stand-in
modules in torch fp32 on the device, and hg_hoi_head with and without the per-image branch.

    python tools/bench_dino_branch.py [--reps 50] [--out profiles/dino_branch.txt] [--parent-lib PATH/libhoigen_amd.so]

features  ResNetFeatures.normalized(images) against avgpool(net(images)).flatten(1) normalised, net = tests/resnet_cases.make_resnet()
          (a seeded ResNet-50 under the frozen norm), at B = 8 and B = 64 of 3 x 224 x 224
head      one hg_hoi_head call with five branches (human|object, union, text, human, global) at a detector-sized batch, the same call
          with an image branch (K_img = 2048, S = 1170 cached rows) as the sixth, and - with --parent-lib, the library of the commit
          before the image source, loaded beside this one - the five-branch call through that library on the same tensors

Device events around each arm, arms alternating within a round, every shape warmed up for 5 rounds, median and range (min .. max) over
--reps rounds.  The events bracket the Python call, so a figure includes the host's time to enqueue the call's launches; for the head
call (about 25 short launches through ctypes) that may be most of the figure - it is the same for every arm.

--parent-lib: libhoigen_amd.so of the parent commit, built from an export of that commit with its own hoigen_amd/csrc/build.sh
(git archive PARENT | tar -x -C DIR; bash DIR/hoigen_amd/csrc/build.sh).  It is loaded beside this tree's library with a context and
cache slots of its own and timed twice per round: the difference of its two arms is the spread a no-change shows."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import hoi_head_bound as hb      # noqa: E402
import resnet_cases as rc        # noqa: E402
import roi_bound as rb           # noqa: E402
from hoigen_amd import _lib      # noqa: E402
from hoigen_amd.cache_model import CacheLogits  # noqa: E402
from hoigen_amd.resnet import ResNetFeatures    # noqa: E402

NC, S, P = 117, 1170, 7


def timed(arms, reps, warmup=5):
    out = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[k].append(a.elapsed_time(b))
    return out


def cell(v):
    return f"{statistics.median(v):8.3f} ({min(v):7.3f} .. {max(v):7.3f})"


def features_lines(reps, dev):
    net = rc.make_resnet()
    net.avgpool, net.fc = nn.AdaptiveAvgPool2d((1, 1)), nn.Identity()
    native = ResNetFeatures.from_module(net).to(dev)
    net = net.to(dev)
    lines = [f"ResNetFeatures.normalized against torch fp32 on the device (seeded ResNet-50, 3 x 224 x 224): ms, median (min .. max) of {reps}",
             f"{'B':>3} | {'native':>30} {'torch':>30} {'torch/native':>12}"]
    for B in (8, 64):
        x = torch.randn(B, 3, 224, 224, device=dev)

        def torch_arm():
            with torch.no_grad():
                f = net.avgpool(net(x)).flatten(1)
                return f / f.norm(dim=-1, keepdim=True)

        t = timed({"native": lambda: native.normalized(x), "torch": torch_arm}, reps)
        lines.append(f"{B:>3} | {cell(t['native'])} {cell(t['torch'])} {statistics.median(t['torch']) / statistics.median(t['native']):>12.2f}")
        print(lines[-1], flush=True)
    return lines


class ParentLib:
    """the library of the commit before HG_HOI_SRC_IMAGE, beside this one: its own context and cache slots; hg_hoi_head_args is the same
    struct in both"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.hg_create.restype = C.c_void_p
        self.lib.hg_create.argtypes = [C.c_int]
        self.lib.hg_load_cache.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.hg_cache_weights)]
        self.lib.hg_hoi_head.argtypes = [C.c_void_p, C.POINTER(_lib.hg_hoi_head_args), C.c_void_p]
        self.lib.hg_last_error.restype = C.c_char_p
        self.lib.hg_last_error.argtypes = [C.c_void_p]
        self.ctx = self.lib.hg_create(0)
        assert self.ctx

    def load_cache(self, slot, weight, bias, labels, lens, post_div):
        keep = [t.detach().float().contiguous() if t is not None else None for t in (weight, bias, labels, lens)]
        w = _lib.hg_cache_weights()
        w.weight, w.bias, w.labels, w.sample_lens = (_lib.tensor(t) for t in keep)
        w.S, w.K, w.C, w.post_div = weight.shape[0], weight.shape[1], labels.shape[1] if labels is not None else 0, post_div
        rc = self.lib.hg_load_cache(self.ctx, slot, C.byref(w))
        assert rc == 0, self.lib.hg_last_error(self.ctx)


def head_lines(reps, dev, parent):
    B, H, Cc, size, n = 8, 24, 768, 336, 12
    n_h = n // 2
    g = torch.Generator().manual_seed(Cc)
    specs = (("human_object", 2 * Cc, 2.0), ("union", Cc, 1.0), ("text", Cc, 1.0), ("human", Cc, 1.0), ("global", Cc, 1.0), ("image", 2048, 1.0))
    branches = []
    for slot, (src, K, post_div) in enumerate(specs):
        w = torch.randn(NC if src == "text" else S, K, generator=g)
        w = (w / w.norm(dim=1, keepdim=True)).to(dev)
        if src == "text":
            t = (w, None, None, None)
        else:
            lab = torch.zeros(S, NC)
            lab[torch.arange(S), torch.arange(S) % NC] = 1
            t = (w, -torch.ones(S, device=dev), lab.to(dev), lab.sum(0).to(dev))
        cache = CacheLogits(*t, post_div)
        if parent is not None and src != "image":
            parent.load_cache(cache.slot, *t, post_div)      # the same slot number in the parent's context
        branches.append(("union" if src == "text" else src, cache, 0.5))
    rng = np.random.RandomState(1)
    feat, fg, fi = torch.randn(B, Cc, H, H, device=dev), torch.randn(B, Cc, device=dev), torch.randn(B, 2048, device=dev)
    fi = fi / fi.norm(dim=1, keepdim=True)
    boxes = np.concatenate([rb.random_boxes(n, size, 100 + b) for b in range(B)])
    labels = np.concatenate([np.r_[np.zeros(n_h, np.int32), rng.randint(1, 80, size=n - n_h).astype(np.int32)] for _ in range(B)])
    box_off = np.arange(B + 1) * n
    Pt = len(hb.batch_pairs(boxes, labels, box_off, [n_h] * B)["pair_h"])
    t_boxes, t_scores, t_labels = torch.from_numpy(boxes).to(dev), torch.rand(B * n, device=dev), torch.from_numpy(labels).to(dev)
    o2t = (torch.rand(80, NC, device=dev) < 0.1).to(torch.uint8)
    logits, prior, scores = torch.empty(Pt, NC, device=dev), torch.empty(2, Pt, NC, device=dev), torch.empty(Pt, NC, device=dev)
    off_c, nh_c = (C.c_int32 * (B + 1))(*box_off.tolist()), (C.c_int32 * B)(*([n_h] * B))

    def args(brs):
        a = _lib.hg_hoi_head_args()
        a.feat_local, a.feat_global, a.boxes, a.scores, a.labels = feat.data_ptr(), fg.data_ptr(), t_boxes.data_ptr(), t_scores.data_ptr(), t_labels.data_ptr()
        a.box_off, a.n_human = off_c, nh_c
        a.B, a.C, a.H, a.W, a.P, a.spatial_scale = B, Cc, H, H, P, float(np.float32(H) / np.float32(size))
        a.n_branch = len(brs)
        for i, (src, cache, w) in enumerate(brs):
            a.branch[i].source, a.branch[i].slot, a.branch[i].scale = _lib.HG_HOI_SRC[src], cache.slot, w
        a.obj2target, a.n_obj_classes, a.num_classes, a.score_pow = o2t.data_ptr(), 80, NC, 2.8
        a.logits, a.prior, a.scores_out = logits.data_ptr(), prior.data_ptr(), scores.data_ptr()
        return a

    a5, a6 = args(branches[:5]), args(branches)
    lib, ctx = _lib.lib(), _lib.ctx(0)

    im = _lib.hg_hoi_image_args(fi.data_ptr(), 2048, None)

    def run(l, c, a):
        rc = l.hg_hoi_head(c, C.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, l.hg_last_error(c)

    def run_image():
        rc = lib.hg_hoi_head_image(ctx, C.byref(a6), C.byref(im), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.hg_last_error(ctx)

    arms = {"five": lambda: run(lib, ctx, a5), "five + image": run_image}
    if parent is not None:      # twice per round: the spread of repeated parent runs in this same process
        arms["parent five"] = lambda: run(parent.lib, parent.ctx, a5)
        arms["parent five (again)"] = lambda: run(parent.lib, parent.ctx, a5)
    t = timed(arms, reps)
    lines = ["figures include the host's time to enqueue each call (device events around the Python call); 'parent' = the parent commit's library, "
             "built from an export of that commit with its own build.sh, loaded beside this one",
             f"hg_hoi_head, B = {B}, map {H} x {H} x {Cc}, {n} boxes an image, {Pt} pairs, {NC} classes, S = {S}: ms, median (min .. max) of {reps}"]
    lines += [f"  {k:<22} {cell(v)}" for k, v in t.items()]
    lines.append(f"  the image branch (K_img 2048: conversion, padding rows, two GEMMs of {B} rows on 256-row tiles, copy) costs "
                 f"{statistics.median(t['five + image']) - statistics.median(t['five']):.3f} ms a call (difference of the medians)")
    for _, c, _ in branches:
        c.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    o = ap.parse_args()
    dev = torch.device("cuda:0")
    parent = ParentLib(o.parent_lib) if o.parent_lib else None
    lines = head_lines(o.reps, dev, parent) + [""] + features_lines(o.reps, dev)
    text = "\n".join(lines) + "\n"
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
