#!/usr/bin/env python
"""Time hg_hoi_head (one call per batch) against the per-image loop built from the entry points that existed before it, and its
pooling kernel alone against roi_align_kernel over the same RoIs.

    python tools/bench_hoi_head.py [--reps 60] [--out profiles/hoi_head.txt]

batched   one hg_hoi_head call: pairs, union boxes, pooled means, normalised rows, four branches (human, object, union with labels;
          union as the linear text map), logits, priors at p = 2.8, scores
loop      per image: roi_align x 2 (boxes, union boxes; reduce_mean), the gathers single[x], single[y], l2_normalize x 3,
          CacheLogits x 4, the scaled sum in torch.  The pair indices and union boxes are built ONCE outside the timed region (the
          reference's meshgrid / nonzero / .item() glue is not charged to the loop), and priors and scores are left out of it.
pool      hg_hoi_head with no branch and no feats (set-up kernel + pooling kernel) against ONE roi_align launch per image over its
          boxes and union boxes together

Device events around each leg, legs alternating, median and minimum over --reps rounds after 5 warm-up rounds; random maps and
seeded uniform boxes (tests/roi_bound.random_boxes), half of an image's boxes humans."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import hoi_head_bound as hb      # noqa: E402
import roi_bound as rb           # noqa: E402
from hoigen_amd import _lib, vae  # noqa: E402
from hoigen_amd.cache_model import CacheLogits  # noqa: E402
from hoigen_amd.roi import roi_align  # noqa: E402

NC, S, P = 117, 1170, 7


def timed(legs, reps, warmup=5):
    """legs: name -> callable; alternating; -> name -> list of ms"""
    out = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[k].append(a.elapsed_time(b))
    return out


def config(B, H, C, size, n, dev, caches):
    n_h = n // 2
    rng = np.random.RandomState(B * 1000 + H * 10 + n)
    feat = torch.randn(B, C, H, H, device=dev)
    boxes = np.concatenate([rb.random_boxes(n, size, 100 + b) for b in range(B)])
    labels = np.concatenate([np.r_[np.zeros(n_h, np.int32), rng.randint(1, 80, size=n - n_h).astype(np.int32)] for _ in range(B)])
    box_off = np.arange(B + 1) * n
    pr = hb.batch_pairs(boxes, labels, box_off, [n_h] * B)
    Pt = len(pr["pair_h"])
    t_boxes, t_scores = torch.from_numpy(boxes).to(dev), torch.rand(B * n, device=dev)
    t_labels = torch.from_numpy(labels).to(dev)
    o2t = (torch.rand(80, NC, device=dev) < 0.1).to(torch.uint8)
    scale = float(np.float32(H) / np.float32(size))
    logits, prior, scores = torch.empty(Pt, NC, device=dev), torch.empty(2, Pt, NC, device=dev), torch.empty(Pt, NC, device=dev)
    ps, pu = torch.empty(B * n, C, device=dev), torch.empty(Pt, C, device=dev)
    off_c, nh_c = (_lib.C.c_int32 * (B + 1))(*box_off.tolist()), (_lib.C.c_int32 * B)(*([n_h] * B))

    def args(branches):
        a = _lib.hg_hoi_head_args()
        a.feat_local, a.boxes, a.scores, a.labels = feat.data_ptr(), t_boxes.data_ptr(), t_scores.data_ptr(), t_labels.data_ptr()
        a.box_off, a.n_human = off_c, nh_c
        a.B, a.C, a.H, a.W, a.P, a.spatial_scale = B, C, H, H, P, scale
        a.n_branch = len(branches)
        for i, (src, cache, w) in enumerate(branches):
            a.branch[i].source, a.branch[i].slot, a.branch[i].scale = _lib.HG_HOI_SRC[src], cache.slot, w
        a.obj2target, a.n_obj_classes, a.num_classes, a.score_pow = o2t.data_ptr(), 80, NC, 2.8
        if branches:
            a.logits, a.prior, a.scores_out = logits.data_ptr(), prior.data_ptr(), scores.data_ptr()
        else:
            a.pooled_single, a.pooled_union = ps.data_ptr(), pu.data_ptr()
        return a

    branches = [("human", caches[0], 0.5), ("object", caches[1], 0.5), ("union", caches[2], 1.0), ("union", caches[3], 2.0)]
    a_full, a_pool = args(branches), args([])
    lib, ctx = _lib.lib(), _lib.ctx(0)

    def batched(a=a_full):
        rc = lib.hg_hoi_head(ctx, _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.hg_last_error(ctx)

    per_image = []
    for b in range(B):
        lo, hi = pr["pair_off"][b], pr["pair_off"][b + 1]
        per_image.append((feat[b], t_boxes[b * n:(b + 1) * n], torch.from_numpy(pr["union_boxes"][lo:hi]).to(dev),
                          torch.from_numpy(pr["pair_h"][lo:hi]).long().to(dev), torch.from_numpy(pr["pair_o"][lo:hi]).long().to(dev)))
    both = [torch.cat([bx, ub]) for _, bx, ub, _, _ in per_image]

    def loop():
        out = []
        for f, bx, ub, x, y in per_image:
            single = roi_align(f, bx, P, scale, reduce_mean=True)
            union = vae.l2_normalize(roi_align(f, ub, P, scale, reduce_mean=True))
            human, obj = vae.l2_normalize(single[x]), vae.l2_normalize(single[y])
            out.append(caches[0](human) * 0.5 + caches[1](obj) * 0.5 + caches[2](union) * 1.0 + caches[3](union) * 2.0)
        return out

    def roi_only():
        return [roi_align(f, r, P, scale, reduce_mean=True) for (f, *_), r in zip(per_image, both)]

    return {"batched": batched, "loop": loop}, {"pool": lambda: batched(a_pool), "roi_align": roi_only}, Pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    assert o.reps >= 50, "median of at least 50"
    dev = torch.device("cuda:0")
    lines = [f"hg_hoi_head against the per-image loop, and its pooling against roi_align_kernel: ms, median (min) of {o.reps} alternating rounds",
             f"{'B':>2} {'map':>12} {'boxes':>5} {'pairs':>6} | {'batched':>15} {'loop':>15} {'loop/batched':>12} | {'pool':>15} {'roi_align':>15} {'roi/pool':>8}"]
    for H, C, size in ((14, 512, 224), (24, 768, 336)):
        g = torch.Generator().manual_seed(C)
        caches = []
        for i in range(4):
            w = torch.randn(S if i < 3 else NC, C, generator=g)
            w = (w / w.norm(dim=1, keepdim=True)).to(dev)
            if i == 3:
                caches.append(CacheLogits(w))
            else:
                lab = torch.zeros(S, NC)
                lab[torch.arange(S), torch.arange(S) % NC] = 1
                caches.append(CacheLogits(w, -torch.ones(S, device=dev), lab.to(dev), lab.sum(0).to(dev)))
        for B in (4, 8):
            for n in (6, 12, 30):
                head, pool, Pt = config(B, H, C, size, n, dev, caches)
                t, tp = timed(head, o.reps), timed(pool, o.reps)
                med = {k: statistics.median(v) for k, v in {**t, **tp}.items()}
                mn = {k: min(v) for k, v in {**t, **tp}.items()}
                cell = lambda k: f"{med[k]:7.3f} ({mn[k]:6.3f})"      # noqa: E731
                lines.append(f"{B:>2} {f'{H}x{H}x{C}':>12} {n:>5} {Pt:>6} | {cell('batched')} {cell('loop')} {med['loop'] / med['batched']:>12.1f} | "
                             f"{cell('pool')} {cell('roi_align')} {med['roi_align'] / med['pool']:>8.2f}")
                print(lines[-1], flush=True)
        for c in caches:
            c.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
