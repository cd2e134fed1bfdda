#!/usr/bin/env python
"""Time hg_region_priors (one call per batch) against the per-image loop it replaces.

    python tools/bench_region_priors.py [--reps 60] [--out profiles/region_priors.txt]

one call  hoigen_amd.proposals.DetectorFrontEnd: the concatenation of the inputs, hg_region_priors, the one device-to-host copy of
          the counts, the output lists
loop      the reference's steps in torch on the GPU, per image: the gathers behind the NMS, four nonzero, the threshold and
          minimum / maximum rules with their host comparisons, two argsort where a rule needs them; then get_prior's padded
          [B, max_n, E + 5] tensor with the embedding indexed by labels.cpu(), and three linears.  The NMS result is handed to the loop
          PRECOMPUTED (there is no torchvision kernel to time): that is in the loop's favour.
select    hg_region_priors with prior_slot = -1 (props_select_kernel alone), C ABI, no host copy
select+mlp  the full C call (props_select_kernel + prior_mlp_kernel), no host copy; mlp = the difference

Device events around each leg, legs alternating, median and minimum over --reps rounds after 5 warm-up rounds.  Cases: B = 4 and 8,
Q = 100 detections an image, 80 object classes, three score profiles that leave about 6, 12 and 30 instances an image
(tests/props_bound.random_image; the scores raised to a power chosen per profile)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import props_bound as pb                     # noqa: E402
from hoigen_amd import _lib, proposals      # noqa: E402

Q, N_CLASSES, E, HIDDEN, HUMAN = 100, 80, 512, 128, 0
PARAMS = dict(pb.PARAMS, human_idx=HUMAN)


def timed(legs, reps, warmup=5):
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


def make_case(B, target, weights):
    """B images whose selection leaves about `target` instances each: the power of the scores is the one of a fixed list that comes closest"""
    r = np.random.RandomState(B * 100 + target)
    sizes = [(480.0, 640.0)] * B
    images = [pb.random_image(r, Q, N_CLASSES, HUMAN, 480.0, 640.0) for _ in range(B)]
    best = None
    for g in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 1, 1.5, 2, 3, 4, 6, 8, 12, 16, 24):
        ims = [((s.astype(np.float64) ** g).astype(np.float32), lb, bx) for s, lb, bx in images]
        n = []
        for s, lb, bx in ims:
            surv = pb.nms(s, lb, bx, PARAMS["nms_thresh"])
            n.append(len(pb.select_rule(s, lb, surv, HUMAN, PARAMS["box_score_thresh"], PARAMS["min_instances"], PARAMS["max_instances"])[0]))
        if best is None or abs(np.mean(n) - target) < abs(best[0] - target):
            best = (float(np.mean(n)), ims)
    return pb.pack(best[1], sizes, PARAMS, weights), best[0]


def loop_leg(case, dev, lin, emb):
    """the per-image loop as a callable; the NMS survivors are computed here, once, outside the timed region"""
    p = case["params"]
    thr, human, mn, mx = p["box_score_thresh"], p["human_idx"], p["min_instances"], p["max_instances"]
    results, survivors = [], []
    for b in range(case["B"]):
        lo, hi = case["q_off"][b], case["q_off"][b + 1]
        sc, lb, bx = case["scores"][lo:hi], case["labels"][lo:hi], case["boxes"][lo:hi]
        results.append((torch.from_numpy(sc).to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(bx).to(dev)))
        survivors.append(torch.from_numpy(pb.nms(sc, lb, bx, p["nms_thresh"])).to(dev))
    image_size = torch.from_numpy(case["image_sizes"]).to(dev)

    def of_kind(kind, sc, keep, n):      # one kind's instances by the threshold, minimum and maximum rules (host comparisons, as there)
        idx = torch.nonzero(kind).squeeze(1)
        if n < mn:
            return idx[sc[idx].argsort(descending=True, stable=True)[:mn]]
        if n > mx:
            return idx[sc[idx].argsort(descending=True, stable=True)[:mx]]
        return keep[torch.nonzero(kind[keep]).squeeze(1)]

    def loop():
        props = []
        for (sc, lb, bx), surv in zip(results, survivors):
            sc, lb, bx = sc[surv].view(-1), lb[surv].view(-1), bx[surv].view(-1, 4)
            keep = torch.nonzero(sc >= thr).squeeze(1)
            is_human = lb == human
            n_human = is_human[keep].sum()
            n_object = len(keep) - n_human
            keep = torch.cat([of_kind(is_human, sc, keep, n_human), of_kind(is_human == 0, sc, keep, n_object)])
            props.append((bx[keep], sc[keep], lb[keep]))
        max_n = max(len(s) for _, s, _ in props)
        mask = torch.ones((len(props), max_n), dtype=torch.bool, device=dev)
        priors = torch.zeros((len(props), max_n, E + 5), device=dev)
        img_h, img_w = image_size.unbind(-1)
        scale = torch.stack([img_w, img_h, img_w, img_h], dim=1)
        for b, (bx, sc, lb) in enumerate(props):
            n = len(bx)
            mask[b, :n] = False
            priors[b, :n, :5] = torch.cat((sc.unsqueeze(-1), bx / scale[b][None, :]), dim=-1)
            priors[b, :n, 5:] = emb[lb.cpu()]
        x = priors
        for i, (w, bias) in enumerate(lin):
            x = F.linear(x, w, bias)
            if i < 2:
                x = F.relu(x)
        return props, (x, mask)

    return loop


def c_leg(case, slot, dev):
    """the raw C call on preallocated buffers (no host copy)"""
    B, cap = case["B"], 2 * case["params"]["max_instances"]
    p = case["params"]
    keepalive = [torch.from_numpy(case["scores"]).to(dev), torch.from_numpy(case["labels"].astype(np.int32)).to(dev), torch.from_numpy(case["boxes"]).to(dev)]
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    outs = [torch.empty(B, 4, **i32), torch.empty(B, cap, **i32), torch.empty(B, cap, 4, **f32), torch.empty(B, cap, **f32), torch.empty(B, cap, **i32),
            torch.empty(B, cap, 64, **f32), torch.empty(B, cap, dtype=torch.uint8, device=dev)]
    a = _lib.hg_region_priors_args()
    a.scores, a.labels, a.boxes = (t.data_ptr() for t in keepalive)
    off_c = (_lib.C.c_int32 * (B + 1))(*[int(v) for v in case["q_off"]])
    size_c = (_lib.C.c_float * (2 * B))(*[float(v) for v in case["image_sizes"].reshape(-1)])
    a.q_off, a.image_sizes, a.B = off_c, size_c, B
    a.box_score_thresh, a.nms_thresh = p["box_score_thresh"], p["nms_thresh"]
    a.human_idx, a.min_instances, a.max_instances, a.prior_slot = p["human_idx"], p["min_instances"], p["max_instances"], slot
    a.counts, a.keep, a.out_boxes, a.out_scores, a.out_labels = (t.data_ptr() for t in outs[:5])
    if slot >= 0:
        a.priors, a.mask = outs[5].data_ptr(), outs[6].data_ptr()
    lib, ctx = _lib.lib(), _lib.ctx(0)

    def run(keep=(keepalive, outs, off_c, size_c)):
        rc = lib.hg_region_priors(ctx, _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.hg_last_error(ctx)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    assert o.reps >= 50, "median of at least 50"
    dev = torch.device("cuda:0")
    weights = pb.make_weights(E, HIDDEN, N_CLASSES, 5)
    t = lambda k: torch.from_numpy(weights[k]).to(dev)      # noqa: E731
    sd = {f"layers.{i}.{k}": t(f"{'w' if k == 'weight' else 'b'}{i}") for i in range(3) for k in ("weight", "bias")}
    emb = t("emb")
    lin = [(sd[f"layers.{i}.weight"], sd[f"layers.{i}.bias"]) for i in range(3)]
    pri = proposals.InstancePriors(sd, emb)
    lines = [f"hg_region_priors against the per-image torch loop (NMS precomputed for the loop): median (min) of {o.reps} alternating rounds; "
             f"Q = {Q}, {N_CLASSES} classes, E = {E}",
             f"{'B':>2} {'inst/img':>8} | {'one call ms':>17} {'loop ms':>17} {'loop/call':>9} | {'select us':>15} {'select+mlp us':>15} {'mlp us':>7}"]
    try:
        for B in (4, 8):
            for target in (6, 12, 30):
                case, n_mean = make_case(B, target, weights)
                front = proposals.DetectorFrontEnd(proposals.RegionProposals(**case["params"]), pri)
                results = []
                for b in range(B):
                    lo, hi = case["q_off"][b], case["q_off"][b + 1]
                    results.append(dict(scores=torch.from_numpy(case["scores"][lo:hi]).to(dev), labels=torch.from_numpy(case["labels"][lo:hi]).to(dev),
                                        boxes=torch.from_numpy(case["boxes"][lo:hi]).to(dev)))
                sizes = torch.from_numpy(case["image_sizes"])
                loop = loop_leg(case, dev, lin, emb)
                # the two legs agree before they are timed
                rp, (pr_a, mask_a) = front(results, sizes)
                props, (pr_b, mask_b) = loop()
                assert all(torch.equal(a["boxes"], b[0]) for a, b in zip(rp, props)) and torch.equal(mask_a, mask_b)
                assert (pr_a - pr_b).abs().max().item() < 1e-4
                tm = timed({"call": lambda: front(results, sizes), "loop": loop}, o.reps)
                tk = timed({"select": c_leg(case, -1, dev), "full": c_leg(case, pri.slot, dev)}, o.reps)
                med = {k: statistics.median(v) for k, v in {**tm, **tk}.items()}
                mn = {k: min(v) for k, v in {**tm, **tk}.items()}
                lines.append(f"{B:>2} {n_mean:>8.1f} | {med['call']:8.3f} ({mn['call']:6.3f}) {med['loop']:8.3f} ({mn['loop']:6.3f}) {med['loop'] / med['call']:>9.1f} | "
                             f"{1e3 * med['select']:7.1f} ({1e3 * mn['select']:5.1f}) {1e3 * med['full']:7.1f} ({1e3 * mn['full']:5.1f}) "
                             f"{1e3 * (med['full'] - med['select']):>7.1f}")
                print(lines[-1], flush=True)
    finally:
        pri.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
