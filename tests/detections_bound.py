"""Test infrastructure for hg_hoi_detections (hoigen_amd/csrc/hg_detections.hip), in the manner of props_bound.py.

  restate(case, flaw)   every stage in the kernels' own arithmetic (numpy float32, one rounding per operation): nonzero(prior[0] * prior[1])
                        in row-major order, the entry fields, recover_boxes, box_iou, min over the two boxes, iou.max(0) over the
                        ground-truth pairs of the detection's class, the winner of every ground-truth pair.  Expected bit for bit.  `flaw`
                        turns it into one of the wrong kernels of FLAWS (tests/test_detections_model.py).
  literal(case)         the reference's own statements (postprocessing, upt_tip_cache_model_free_finetune_distill3.py:1408-1427;
                        test_hico, utils_tip_cache_and_union_finetune.py:376-409; BoxAssociation.__call__,
                        pocket/pocket/utils/association.py:66-90) executed statement by statement in torch, per image and per class, on top
                        of the restated IoU (torchvision is not installed: box_iou is the restatement's).
  definition(case)      the same association in float64 (recover_boxes and box_iou in float64 from the same fp32 inputs).
  screened(case, b)     image b is set aside from the INTEGER comparison with the definition when, in some same-class pair, the IoU lies
                        within the fp32 chain's error of min_iou, or a detection's two best IoUs lie within that error of each other.  The
                        error comes from interval arithmetic with half an ulp per operation: a recovered ground-truth coordinate carries
                        (cx -+ 0.5 w) and the scaling, two roundings (none with gt_format 0; detection boxes are inputs, exact); a length two
                        coordinates and its own rounding; then the product, the sum, the difference and the quotient.
  judge(...)            the rules of tests/test_gpu_detections.py as one function: rule 1 everything bit for bit against restate, rule 3
                        labels and det_gt equal the definition's but on screened images.

A NaN IoU is written as the one pattern 0x7FC00000 (the sign and payload of 0 / 0 are the platform's); a class without ground truth gives
det_gt = -1 and det_max_iou = 0.
"""
import functools

import numpy as np

F = np.float32
U = 2.0 ** -24
NAN_BITS = 0x7FC00000
ENTRY_INT = ("pair", "verb", "h", "o", "object", "interaction")
FLAWS = ("iou_ge", "argmax_last", "no_class_filter", "every_gt_candidate", "tp_per_detection", "rank_by_iou", "score_ties_high", "human_only",
         "product", "union_no_inter", "column_major", "nan_zero", "conversion_transposed", "cx_minus_w", "gt_unscaled", "hw_swapped")


# ---- compaction ------------------------------------------------------------------------------------------------------------------------
def compact(case, flaw=None):
    """det_off [B + 1] and the seven entry arrays, image by image, (x, y) row-major"""
    B, NC = case["B"], case["NC"]
    with np.errstate(all="ignore"):
        prod = case["prior"][0] * case["prior"][1]      # ONE fp32 multiply
    nz = prod != 0                                      # NaN != 0
    if flaw == "nan_zero":
        nz &= ~np.isnan(prod)
    conv = case.get("conversion")
    out = {k: [] for k in ENTRY_INT + ("score",)}
    det_off, status = [0], np.zeros(B, np.int32)
    for b in range(B):
        lo, hi = case["pair_off"][b], case["pair_off"][b + 1]
        if flaw == "column_major":
            y, x = np.nonzero(nz[lo:hi].T)
        else:
            x, y = np.nonzero(nz[lo:hi])
        obj = case["objects"][lo:hi][x]
        if conv is None:
            inter = y.astype(np.int32)
        else:
            ok = (obj >= 0) & (obj < conv.shape[0])
            o_ = np.where(ok, obj, 0)
            tab = conv.reshape(-1).reshape(NC, conv.shape[0])[y, o_] if flaw == "conversion_transposed" else conv[o_, y]
            inter = np.where(ok & (tab >= 0), tab, -1).astype(np.int32)
            if (inter < 0).any():
                status[b] |= 1
        out["pair"].append(x.astype(np.int32))
        out["verb"].append(y.astype(np.int32))
        out["h"].append(case["pair_h"][lo:hi][x])
        out["o"].append(case["pair_o"][lo:hi][x])
        out["object"].append(obj)
        out["score"].append(case["scores"][lo:hi][x, y])
        out["interaction"].append(inter)
        det_off.append(det_off[-1] + len(x))
    res = {k: np.concatenate(v) if v else np.zeros(0, np.int32) for k, v in out.items()}
    res["score"] = res["score"].astype(F)
    res["det_off"] = np.asarray(det_off, np.int32)
    res["status"] = status
    return res


# ---- ground truth and IoU ---------------------------------------------------------------------------------------------------------------
def recover(case, b, dtype=F, flaw=None):
    """image b's ground-truth boxes [2, G, 4] as x1, y1, x2, y2 in pixels"""
    lo, hi = case["gt_off"][b], case["gt_off"][b + 1]
    g = np.stack([case["gt_h"][lo:hi], case["gt_o"][lo:hi]]).astype(dtype)
    if case["gt_format"] == 0:
        return g
    h, w = case["gt_sizes"][b]
    if flaw == "hw_swapped":
        h, w = w, h
    half = dtype(0.5) if flaw != "cx_minus_w" else dtype(1.0)
    cx, cy, bw, bh = g[..., 0], g[..., 1], g[..., 2], g[..., 3]
    with np.errstate(all="ignore"):
        out = np.stack([cx - half * bw, cy - half * bh, cx + half * bw, cy + half * bh], -1)
        if flaw != "gt_unscaled":
            out = out * np.asarray([w, h, w, h], dtype)
    return out.astype(dtype)


def box_iou(g, d, flaw=None):
    """torchvision's box_iou [G, D] in the boxes' dtype, one rounding per operation; minimum, maximum and the clamp hand a NaN on"""
    with np.errstate(all="ignore"):
        ag = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        ad = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
        w = np.maximum(np.minimum(g[:, None, 2], d[None, :, 2]) - np.maximum(g[:, None, 0], d[None, :, 0]), 0)
        h = np.maximum(np.minimum(g[:, None, 3], d[None, :, 3]) - np.maximum(g[:, None, 1], d[None, :, 1]), 0)
        inter = w * h
        union = ag[:, None] + ad[None, :]
        if flaw != "union_no_inter":
            union = union - inter
        return (inter / union).astype(g.dtype)


def pair_iou(gt, boxes_h, boxes_o, flaw=None):
    ih = box_iou(gt[0], boxes_h, flaw)
    if flaw == "human_only":
        return ih
    io = box_iou(gt[1], boxes_o, flaw)
    with np.errstate(all="ignore"):
        return (ih * io).astype(ih.dtype) if flaw == "product" else np.minimum(ih, io)


def max0(iou, mask, last=False):
    """iou.max(0) over the rows mask admits -> (max_iou [D], max_idx [D]): the first index of the maximum, a NaN is the maximum from
    its first index on; no admitted row: (0, -1)"""
    G, D = iou.shape
    best, idx = np.zeros(D, iou.dtype), np.full(D, -1, np.int32)
    if G == 0 or D == 0:
        return best, idx
    nan = mask & np.isnan(iou)
    v = np.where(mask & ~nan, iou, -np.inf)
    if last:
        i = G - 1 - np.argmax(v[::-1], 0)
    else:
        i = np.argmax(v, 0)
    cols = np.arange(D)
    off = ~mask[i, cols]                    # the maximum is a filler: every admitted value is -inf, the first admitted row wins
    i = np.where(off, np.argmax(mask, 0), i)
    has = mask.any(0)
    best = np.where(has, iou[i, cols], 0).astype(iou.dtype)
    idx = np.where(has, i, -1).astype(np.int32)
    anynan = nan.any(0)
    idx = np.where(anynan, np.argmax(nan, 0), idx).astype(np.int32)
    best = np.where(anynan, np.nan, best).astype(iou.dtype)
    return best, idx


def winners(cand, rank, ties_high=False):
    """label [D]: per row of cand [G, D] the admitted column with the highest rank value (NaN above every number, ties to the lowest -
    or, for the flaw, the highest - column)"""
    label = np.zeros(cand.shape[1], F)
    for g in np.nonzero(cand.any(1))[0]:
        idx = np.nonzero(cand[g])[0]
        s = rank[g][idx] if rank.ndim == 2 else rank[idx]
        nan = np.isnan(s)
        if nan.any():
            pick = np.nonzero(nan)[0]
        else:
            pick = np.nonzero(s == s.max())[0]
        label[idx[pick[-1] if ties_high else pick[0]]] = 1
    return label


def associate_image(case, b, ent, dtype=F, flaw=None):
    """-> (label [D] float32, det_gt [D] int32, max_iou [D] dtype, gt boxes [2, G, 4] dtype) of image b"""
    lo, hi = ent["det_off"][b], ent["det_off"][b + 1]
    gt = recover(case, b, dtype, flaw)
    G, D = gt.shape[1], hi - lo
    bx = case["boxes"][case["box_off"][b]:case["box_off"][b + 1]].astype(dtype)
    inter = ent["interaction"][lo:hi]
    hoi = case["gt_hoi"][case["gt_off"][b]:case["gt_off"][b + 1]]
    if D == 0 or G == 0:
        return np.zeros(D, F), np.full(D, -1, np.int32), np.zeros(D, dtype), gt
    iou = pair_iou(gt, bx[ent["h"][lo:hi]], bx[ent["o"][lo:hi]], flaw)
    mask = (hoi[:, None] == inter[None, :]) & (inter[None, :] >= 0)
    if flaw == "no_class_filter":
        mask = np.ones_like(mask)
    best, idx = max0(iou, mask, last=flaw == "argmax_last")
    thr = dtype(F(case["min_iou"]))
    with np.errstate(invalid="ignore"):
        over = best >= thr if flaw == "iou_ge" else best > thr
        cand = (np.arange(G)[:, None] == idx[None, :]) & over[None, :]
        if flaw == "every_gt_candidate":
            cand = mask & (iou > thr)
    sc = ent["score"][lo:hi]
    if flaw == "tp_per_detection":
        label = cand.any(0).astype(F)
    else:
        label = winners(cand, iou if flaw == "rank_by_iou" else sc, ties_high=flaw == "score_ties_high")
    return label, idx, best, gt


def canonical(a):
    """float32 with every NaN as the pattern 0x7FC00000"""
    a = np.ascontiguousarray(a, F).copy()
    a.view(np.uint32)[np.isnan(a)] = NAN_BITS
    return a


def restate(case, flaw=None, dtype=F):
    ent = compact(case, flaw)
    if case.get("gt_off") is None:
        return ent
    B = case["B"]
    lab, gts, ious, boxes = [], [], [], []
    for b in range(B):
        l, g, m, bx = associate_image(case, b, ent, dtype, flaw)
        lab.append(l); gts.append(g); ious.append(m); boxes.append(bx)
        if not np.isfinite(bx).all():
            ent["status"][b] |= 2
    ent["label"] = np.concatenate(lab).astype(F) if lab else np.zeros(0, F)
    ent["gt"] = np.concatenate(gts).astype(np.int32) if gts else np.zeros(0, np.int32)
    mi = np.concatenate(ious) if ious else np.zeros(0, dtype)
    ent["max_iou"] = canonical(mi) if dtype is F else mi
    gb = np.concatenate(boxes, 1) if boxes else np.zeros((2, 0, 4), dtype)
    ent["gt_boxes"] = gb.astype(F) if dtype is F else gb
    return ent


def definition(case):
    return restate(case, dtype=np.float64)


def apply_cap(exp, cap):
    """what a call with `cap` slots leaves of restate's answer: the entries below cap, bit 2 where an image ends behind it"""
    out = dict(exp)
    for k in ENTRY_INT + ("score", "label", "gt", "max_iou"):
        if k in out:
            out[k] = out[k][:cap]
    out["status"] = exp["status"] | np.where(exp["det_off"][1:] > cap, 4, 0).astype(np.int32)
    return out


# ---- the reference's statements --------------------------------------------------------------------------------------------------------
def literal(case):
    """per image: postprocessing's nonzero / gathers, test_hico's conversion and per-class loop, BoxAssociation.__call__ - in torch, on the
    restated IoU.  -> the dict restate gives (max_iou / gt are the last association's per detection, as BoxAssociation keeps them)"""
    import torch

    B, NC = case["B"], case["NC"]
    conv = case.get("conversion")
    keys = ENTRY_INT + ("score", "label", "gt", "max_iou")
    out = {k: [] for k in keys}
    det_off, status, boxes_out = [0], np.zeros(B, np.int32), []
    min_iou = float(F(case["min_iou"])) if case.get("gt_off") is not None else None
    for b in range(B):
        lo, hi = case["pair_off"][b], case["pair_off"][b + 1]
        pr = torch.from_numpy(case["prior"][:, lo:hi])
        bh, bo = torch.from_numpy(case["pair_h"][lo:hi]).long(), torch.from_numpy(case["pair_o"][lo:hi]).long()
        objects = torch.from_numpy(case["objects"][lo:hi]).long()
        dense = torch.from_numpy(case["scores"][lo:hi])
        x, y = torch.nonzero(pr.prod(0)).unbind(1)                                                        # :1418
        pairing, scores, verbs, objs = torch.stack([bh[x], bo[x]]), dense[x, y], y, objects[x]            # :1419-1424
        if conv is not None:
            table = torch.from_numpy(conv.astype(np.float64))
            ok = (objs >= 0) & (objs < conv.shape[0])
            interactions = torch.where(ok, table[torch.where(ok, objs, 0), verbs], torch.tensor(-1.0, dtype=torch.float64))   # :386
            if bool((interactions < 0).any()):
                status[b] |= 1
        else:
            interactions = verbs                                                                          # :388
        out["pair"].append(x.numpy().astype(np.int32)); out["verb"].append(y.numpy().astype(np.int32))
        out["h"].append(pairing[0].numpy().astype(np.int32)); out["o"].append(pairing[1].numpy().astype(np.int32))
        out["object"].append(objs.numpy().astype(np.int32)); out["score"].append(scores.numpy())
        out["interaction"].append(interactions.numpy().astype(np.int32))
        det_off.append(det_off[-1] + len(x))
        if min_iou is None:
            continue
        gt = recover(case, b)                                                                              # :391-392
        boxes_out.append(gt)
        if not np.isfinite(gt).all():
            status[b] |= 2
        bx = case["boxes"][case["box_off"][b]:case["box_off"][b + 1]]
        boxes_h, boxes_o = bx[pairing[0].numpy()], bx[pairing[1].numpy()]                                  # :380
        hoi = torch.from_numpy(case["gt_hoi"][case["gt_off"][b]:case["gt_off"][b + 1]]).to(interactions.dtype)
        labels = torch.zeros_like(scores)                                                                  # :394
        max_iou_all, max_idx_all = torch.zeros_like(scores), torch.full_like(verbs, -1)
        for hoi_idx in interactions.unique():                                                              # :397
            if hoi_idx < 0:
                continue
            gt_idx = torch.nonzero(hoi == hoi_idx).squeeze(1)                                              # :398
            det_idx = torch.nonzero(interactions == hoi_idx).squeeze(1)                                    # :399
            if len(gt_idx):                                                                                # :400
                iou = torch.from_numpy(pair_iou(gt[:, gt_idx.numpy()], boxes_h[det_idx.numpy()], boxes_o[det_idx.numpy()]))
                sc = scores[det_idx].view(-1)
                max_iou, max_idx = iou.max(0)                                                              # association.py:68
                match = torch.zeros_like(iou)                                                              # :76
                match[max_idx, torch.arange(iou.shape[1])] = max_iou                                       # :77
                match = match > min_iou                                                                    # :79
                lab = torch.zeros_like(sc)                                                                 # :81
                for i, m in enumerate(match):                                                              # :83
                    match_idx = torch.nonzero(m).squeeze(1)
                    if len(match_idx) == 0:
                        continue
                    match_scores = sc[match_idx]
                    lab[match_idx[match_scores.argmax()]] = 1                                              # :88
                labels[det_idx] = lab                                                                      # :401
                max_iou_all[det_idx] = max_iou
                max_idx_all[det_idx] = gt_idx[max_idx]
        out["label"].append(labels.numpy()); out["gt"].append(max_idx_all.numpy().astype(np.int32)); out["max_iou"].append(max_iou_all.numpy())
    res = {k: (np.concatenate(v) if v else np.zeros(0, F if k in ("score", "label", "max_iou") else np.int32)) for k, v in out.items()
           if min_iou is not None or k not in ("label", "gt", "max_iou")}
    res["det_off"], res["status"] = np.asarray(det_off, np.int32), status
    if min_iou is not None:
        res["max_iou"] = canonical(res["max_iou"])
        res["gt_boxes"] = np.concatenate(boxes_out, 1) if boxes_out else np.zeros((2, 0, 4), F)
    return res


# ---- the screen ------------------------------------------------------------------------------------------------------------------------
def _iou_interval(g, d, dg):
    """[G, D] lower and upper ends of box_iou under the fp32 chain's error; dg [G] = absolute error of a ground-truth coordinate"""
    dx = np.minimum(g[:, None, 2], d[None, :, 2]) - np.maximum(g[:, None, 0], d[None, :, 0])
    dy = np.minimum(g[:, None, 3], d[None, :, 3]) - np.maximum(g[:, None, 1], d[None, :, 1])
    e = lambda v, c: 2 * c + U * np.abs(v)          # a length: two coordinates and its own rounding
    r = 1 + 4 * U                                   # the product, the sum and the difference around it
    i_lo = np.maximum(dx - e(dx, dg[:, None]), 0) * np.maximum(dy - e(dy, dg[:, None]), 0) / r
    i_hi = np.maximum(dx + e(dx, dg[:, None]), 0) * np.maximum(dy + e(dy, dg[:, None]), 0) * r
    gw, gh, dw, dh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1], d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
    ag_lo, ag_hi = np.maximum(gw - e(gw, dg), 0) * np.maximum(gh - e(gh, dg), 0) / r, (gw + e(gw, dg)) * (gh + e(gh, dg)) * r
    ad_lo, ad_hi = np.maximum(dw - e(dw, 0), 0) * np.maximum(dh - e(dh, 0), 0) / r, (dw + e(dw, 0)) * (dh + e(dh, 0)) * r
    u_lo, u_hi = (ag_lo[:, None] + ad_lo[None] - i_hi) / r, (ag_hi[:, None] + ad_hi[None] - i_lo) * r
    with np.errstate(invalid="ignore", divide="ignore"):
        q_lo = np.where(u_hi > 0, i_lo / u_hi / r, 0)
        q_hi = np.where(i_hi <= 0, 0, np.where(u_lo > 0, i_hi / u_lo * r, np.inf))
    return q_lo, q_hi


def screened(case, b, ent=None):
    ent = ent if ent is not None else compact(case)
    lo, hi = ent["det_off"][b], ent["det_off"][b + 1]
    gt = recover(case, b, np.float64)
    G, D = gt.shape[1], hi - lo
    if G == 0 or D == 0:
        return False
    bx = case["boxes"][case["box_off"][b]:case["box_off"][b + 1]].astype(np.float64)
    if not (np.isfinite(gt).all() and np.isfinite(bx).all()):
        return True
    # a recovered coordinate: the difference cx -+ 0.5 w and the scaling, half an ulp of the result each
    dg = np.zeros(G) if case["gt_format"] == 0 else 2 * U * (1 + 2 * U) * np.abs(gt).max(axis=(0, 2))
    hl, hh = _iou_interval(gt[0], bx[ent["h"][lo:hi]], dg)
    ol, oh = _iou_interval(gt[1], bx[ent["o"][lo:hi]], dg)
    q_lo, q_hi = np.minimum(hl, ol), np.minimum(hh, oh)
    inter = ent["interaction"][lo:hi]
    hoi = case["gt_hoi"][case["gt_off"][b]:case["gt_off"][b + 1]]
    mask = (hoi[:, None] == inter[None, :]) & (inter[None, :] >= 0)
    thr = np.float64(F(case["min_iou"]))
    if (mask & (q_lo <= thr) & (thr <= q_hi) & (q_hi > q_lo)).any():
        return True
    lo_m = np.where(mask, q_lo, -1.0)
    star = np.argmax(lo_m, 0)
    best_lo = lo_m[star, np.arange(D)]
    rival = mask & (q_hi >= best_lo[None, :]) & (q_hi > 0)
    rival[star, np.arange(D)] = False
    return bool(rival.any())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


def judge(got, case, expected=None, defn=None, skip_rule3=()):
    """the rules of the GPU test on one set of outputs (the dict restate gives); raises AssertionError with the first thing that is off,
    returns the number of screened images"""
    exp = expected if expected is not None else restate(case)
    for k in ("det_off", "status") + ENTRY_INT:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), exp[k].astype(np.int64)), f"rule 1: {k}"
    assert same_bits(np.asarray(got["score"], F), exp["score"]), "rule 1: score"
    if case.get("gt_off") is None:
        return 0
    assert np.array_equal(np.asarray(got["gt"]).astype(np.int64), exp["gt"].astype(np.int64)), "rule 1: gt"
    for k in ("label", "max_iou", "gt_boxes"):
        assert same_bits(np.asarray(got[k], F), exp[k]), f"rule 1: {k}"
    defn = defn if defn is not None else definition(case)
    n_screened = 0
    for b in range(case["B"]):
        if b in skip_rule3:
            continue
        if screened(case, b, exp):
            n_screened += 1
            continue
        lo, hi = exp["det_off"][b], exp["det_off"][b + 1]
        assert np.array_equal(np.asarray(got["label"][lo:hi]), defn["label"][lo:hi]), f"rule 3: labels of image {b}"
        assert np.array_equal(np.asarray(got["gt"][lo:hi]), defn["gt"][lo:hi]), f"rule 3: det_gt of image {b}"
    return n_screened


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def split_pairs(P):
    """(n_h, n) with n_h (n - 1) == P and the fewest boxes (P == 0: one lone human)"""
    if P == 0:
        return 1, 1
    best = None
    for n_h in range(1, P + 1):
        if P % n_h == 0:
            n = P // n_h + 1
            if n_h <= n and (best is None or n < best[1]):
                best = (n_h, n)
    return best


def pair_rows(n_h, n):
    """hg_hoi_head's pairs of an image: (x, y), x < n_h, y != x, row-major"""
    x, y = np.meshgrid(np.arange(n_h), np.arange(n), indexing="ij")
    keep = x != y
    return x[keep].astype(np.int32), y[keep].astype(np.int32)


def random_boxes(r, n):
    """continuous coordinates: corners uniform in [0, 500), sides 8 - 300"""
    xy = r.uniform(0, 500, (n, 2))
    wh = r.uniform(8, 300, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(F)


def random_case(seed, NC, pairs, gts, gt_format=0, n_obj=None, targets=3, min_iou=0.5, p_set=1.0):
    """B = len(pairs) images; image b has pairs[b] pairs and gts[b] ground-truth pairs, each a detection's two boxes plus N(0, 12) jitter
    with that detection's class (where the image has detections).  n_obj: a conversion table of that many object classes (else none,
    and 8 object classes)."""
    r = np.random.RandomState(seed)
    B = len(pairs)
    n_cls = n_obj or 8
    k = min(targets, NC)
    obj2target = np.zeros((n_cls, NC), bool)
    for o in range(n_cls):
        obj2target[o, r.choice(NC, k, replace=False)] = True
    conv = None
    if n_obj:
        conv = np.full((n_cls, NC), -1, np.int32)
        conv[obj2target] = r.permutation(int(obj2target.sum())).astype(np.int32)      # every valid (object, verb) its own interaction
    box_off, pair_off, gt_off = [0], [0], [0]
    boxes, ph, po, objs, prior, scores, gh, go, ghoi, sizes = [], [], [], [], [], [], [], [], [], []
    for b in range(B):
        n_h, n = split_pairs(pairs[b])
        x, y = pair_rows(n_h, n)
        assert len(x) == pairs[b]
        bx = random_boxes(r, n)
        lab = np.concatenate([np.zeros(n_h, np.int32), r.randint(1, n_cls, n - n_h).astype(np.int32)])
        s = r.uniform(0.05, 1.0, n)
        obj = lab[y]
        on = obj2target[obj] & (r.rand(len(x), NC) < p_set)
        p0 = np.where(on, (s[x] ** 2.8)[:, None], 0).astype(F)
        p1 = np.where(on, (s[y] ** 2.8)[:, None], 0).astype(F)
        sc = (r.uniform(0.01, 1.0, (len(x), NC)).astype(F) * (p0 * p1)).astype(F)
        h, w = int(r.randint(400, 800)), int(r.randint(801, 1200))
        G = gts[b]
        rows, cols = np.nonzero((p0 * p1) != 0)
        if len(rows):
            pick = r.randint(0, len(rows), G)
            g_h = bx[x[rows[pick]]].astype(np.float64) + r.normal(0, 12, (G, 4))
            g_o = bx[y[rows[pick]]].astype(np.float64) + r.normal(0, 12, (G, 4))
            cls = conv[obj[rows[pick]], cols[pick]] if conv is not None else cols[pick]
        else:
            g_h, g_o = random_boxes(r, G).astype(np.float64), random_boxes(r, G).astype(np.float64)
            cls = r.randint(0, NC, G)
        if gt_format == 1:
            to_c = lambda g: np.stack([(g[:, 0] + g[:, 2]) / 2 / w, (g[:, 1] + g[:, 3]) / 2 / h, (g[:, 2] - g[:, 0]) / w, (g[:, 3] - g[:, 1]) / h], 1)
            g_h, g_o = to_c(g_h), to_c(g_o)
        boxes.append(bx); ph.append(x); po.append(y); objs.append(obj); prior.append(np.stack([p0, p1])); scores.append(sc)
        gh.append(g_h.astype(F).reshape(G, 4)); go.append(g_o.astype(F).reshape(G, 4)); ghoi.append(np.asarray(cls, np.int32).reshape(G))
        sizes.append((h, w))
        box_off.append(box_off[-1] + n); pair_off.append(pair_off[-1] + len(x)); gt_off.append(gt_off[-1] + G)
    return dict(B=B, NC=NC, pair_off=np.asarray(pair_off, np.int32), box_off=np.asarray(box_off, np.int32), gt_off=np.asarray(gt_off, np.int32),
                prior=np.concatenate(prior, 1), scores=np.concatenate(scores), pair_h=np.concatenate(ph), pair_o=np.concatenate(po),
                objects=np.concatenate(objs), boxes=np.concatenate(boxes), conversion=conv, gt_h=np.concatenate(gh), gt_o=np.concatenate(go),
                gt_hoi=np.concatenate(ghoi), gt_sizes=np.asarray(sizes, np.int32), gt_format=gt_format, min_iou=min_iou)


PAIR_EDGES = (0, 1, 2, 63, 64, 65)
GT_EDGES = (0, 1, 2, 63, 64, 65)
# name -> arguments of random_case.  Between them: NC = 1, 24, 63, 64, 65, 117, 600; pairs an image 0, 1, 2, 63, 64, 65 and 2 016 ragged in one
# call; B = 1, 3, 8, 64; ground-truth pairs an image 0, 1, 2, 63, 64, 65, 256; both gt_formats; with and without conversion.  b64_scan has
# 64 x 2 016 rows = 2 016 workgroups of det_count_kernel: det_scan_kernel's loop crosses its 256-sum block boundary seven times.
FAMILIES = {
    "b1_nc1": dict(seed=1, NC=1, pairs=(2,), gts=(1,)),
    "b3_nc24_conv": dict(seed=2, NC=24, pairs=(0, 1, 65), gts=(0, 2, 63), gt_format=1, n_obj=12),
    "b8_nc63": dict(seed=3, NC=63, pairs=(63, 64, 65, 0, 2, 1, 64, 2), gts=(1, 2, 5, 64, 0, 2, 65, 3)),
    "b3_nc64": dict(seed=4, NC=64, pairs=(64, 0, 63), gts=(2, 1, 64), gt_format=1, targets=64, p_set=0.5),
    "b3_nc65": dict(seed=5, NC=65, pairs=(65, 2, 1), gts=(63, 0, 1), targets=65, p_set=0.7),
    "b8_nc117_conv": dict(seed=6, NC=117, pairs=(63, 64, 65, 0, 2, 1, 2016, 64), gts=(1, 2, 63, 64, 65, 0, 256, 5), gt_format=1, n_obj=80, targets=6),
    "b64_nc600": dict(seed=7, NC=600, pairs=tuple(PAIR_EDGES[i % 6] for i in range(63)) + (2016,), gts=tuple(GT_EDGES[(i // 6) % 6] for i in range(63)) + (256,),
                      gt_format=1, targets=4),
    "b64_scan": dict(seed=8, NC=1, pairs=(2016,) * 64, gts=(2,) * 64, targets=1, p_set=0.5),
}


@functools.lru_cache(maxsize=None)
def family(name):
    """Cached: leave unchanged."""
    return random_case(**FAMILIES[name])


# ---- constructed images: hand-derived answers, every number exactly representable ---------------------------------------------------------
def constructed():
    """-> (case, index name -> image, known name -> (labels, det_gt) of the image's detections).  One human (box 0) and one or more
    objects per image unless said otherwise; NC = 4, conversion with one -1 entry, gt_format 0, min_iou 0.5."""
    NC, n_obj = 4, 3
    conv = np.arange(n_obj * NC, dtype=np.int32).reshape(n_obj, NC)
    conv[2, 3] = -1
    images, index, known = [], {}, {}

    def image(name, boxes, n_h, labels, rows, gt, answer=None):
        """rows: per pair (in hg_hoi_head's order) a dict verb -> (prior0, prior1, score); gt: list of (box_h, box_o, class)"""
        index[name] = len(images)
        images.append((np.asarray(boxes, F).reshape(-1, 4), n_h, np.asarray(labels, np.int32), rows, gt))
        if answer is not None:
            known[name] = answer

    H, O, FAR = [0, 0, 1, 1], [10, 10, 12, 12], [100, 100, 101, 101]
    one = lambda s=0.5, v=0: {v: (1.0, 1.0, s)}
    # IoU exactly 0.5 is not above min_iou: ground truth [0, 0, 2, 1] against the detection [0, 0, 1, 1]; the object boxes coincide
    image("iou_exactly_half", [H, O], 1, [0, 1], [one()], [([0, 0, 2, 1], O, 4)], ([0], [0]))
    # two detections of one ground-truth pair (two humans at the same place, one object): only the higher score is a TP
    image("two_dets_higher_score", [H, H, O], 2, [0, 0, 1], [{}, one(0.25), {}, one(0.75)], [(H, O, 4)], ([0, 1], [0, 0]))
    image("two_dets_equal_score", [H, H, O], 2, [0, 0, 1], [{}, one(0.5), {}, one(0.5)], [(H, O, 4)], ([1, 0], [0, 0]))
    # a detection equally over two ground-truth pairs goes to the first
    image("equal_over_two_gt", [H, O], 1, [0, 1], [one()], [(H, O, 4), (H, O, 4)], ([1], [0]))
    # detection 0 = [0, 0, 4, 4] (score 0.75) and detection 1 = [0, 0, 4, 3] (0.25) both have their maximum on ground truth 0 = [0, 0, 4, 4]
    # (IoU 1 and 3 / 4), which detection 0 takes; ground truth 1 = [0, 1, 4, 3] overlaps detection 1 with 8 / 12 > 0.5 (and detection 0 with
    # 8 / 16, not above) but is not its max_idx: label 0
    image("max_idx_taken", [[0, 0, 4, 4], [0, 0, 4, 3], O], 2, [0, 0, 1], [{}, one(0.75), {}, one(0.25)],
          [([0, 0, 4, 4], O, 4), ([0, 1, 4, 3], O, 4)], ([1, 0], [0, 0]))
    # human IoU 1 above, object IoU below the threshold (ground truth [10, 10, 18, 12] of area 16 over the detection's 4: 4 / 16): no match
    image("object_below", [H, O], 1, [0, 1], [one()], [(H, [10, 10, 18, 12], 4)], ([0], [0]))
    # ground truth of another class is ignored: det_gt -1
    image("other_class", [H, O], 1, [0, 1], [one()], [(H, O, 5)], ([0], [-1]))
    image("no_ground_truth", [H, O], 1, [0, 1], [one()], [], ([0], [-1]))
    image("no_detections", [H, O], 1, [0, 1], [{}], [(H, O, 4)], ([], []))
    image("no_pairs", [H], 1, [0], [], [(H, O, 4)], ([], []))
    # a zero-area detection over a zero-area ground truth: 0 / 0 = NaN, and the maximum is NaN even beside an IoU of 1 (ground truth 0)
    Z = [5, 5, 5, 5]
    image("nan_iou", [Z, Z], 1, [0, 1], [one()], [([5, 5, 5, 5], [5, 5, 5, 5], 4), ([5, 5, 5, 5], [5, 5, 5, 5], 4)], ([0], [0]))
    # the detection (H, Z): human IoU 1 with every ground truth, object IoU 0, NaN (0 / 0 on the zero-area ground truth), 0: the maximum is NaN
    image("nan_beside_one", [H, O, Z], 1, [0, 1, 1], [{}, one()], [(H, [4, 4, 6, 6], 4), (H, Z, 4), (H, [4, 4, 6, 6], 4)], None)
    # a NaN prior column counts as a detection; a product that underflows to 0 does not (1e-30 * 1e-30), a denormal product does
    image("nan_prior", [H, O], 1, [0, 1], [{0: (np.nan, 1.0, 0.5), 1: (1e-30, 1e-30, 0.5), 2: (1e-20, 1e-20, 0.5)}], [(H, O, 4)], ([1, 0], [0, -1]))
    # a fully zero row and a fully set row
    image("zero_and_full_rows", [H, O, FAR], 1, [0, 1, 1], [{}, {v: (1.0, 1.0, 0.5) for v in range(NC)}], [(H, FAR, 4)], ([1, 0, 0, 0], [0, -1, -1, -1]))
    # a conversion entry of -1: object class 2, verb 3 (status bit 0; its label stays 0 though a ground truth of class -1 lies on it)
    image("conversion_minus_one", [H, O], 1, [0, 2], [{3: (1.0, 1.0, 0.5)}], [(H, O, -1)], ([0], [-1]))
    box_off, pair_off, gt_off = [0], [0], [0]
    boxes, ph, po, objs, prior, scores, gh, go, ghoi = [], [], [], [], [], [], [], [], []
    for bx, n_h, lab, rows, gt in images:
        n = len(bx)
        x, y = pair_rows(n_h, n) if n > 1 else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert len(rows) == len(x), (len(rows), len(x))
        p, s = np.zeros((2, len(x), NC), F), np.zeros((len(x), NC), F)
        for i, row in enumerate(rows):
            for v, (a, b_, sc) in row.items():
                p[0, i, v], p[1, i, v], s[i, v] = a, b_, sc
        boxes.append(bx); ph.append(x); po.append(y); objs.append(lab[y]); prior.append(p); scores.append(s)
        gh.append(np.asarray([g[0] for g in gt], F).reshape(-1, 4)); go.append(np.asarray([g[1] for g in gt], F).reshape(-1, 4))
        ghoi.append(np.asarray([g[2] for g in gt], np.int32))
        box_off.append(box_off[-1] + n); pair_off.append(pair_off[-1] + len(x)); gt_off.append(gt_off[-1] + len(gt))
    B = len(images)
    case = dict(B=B, NC=NC, pair_off=np.asarray(pair_off, np.int32), box_off=np.asarray(box_off, np.int32), gt_off=np.asarray(gt_off, np.int32),
                prior=np.concatenate(prior, 1), scores=np.concatenate(scores), pair_h=np.concatenate(ph), pair_o=np.concatenate(po),
                objects=np.concatenate(objs), boxes=np.concatenate(boxes), conversion=conv, gt_h=np.concatenate(gh), gt_o=np.concatenate(go),
                gt_hoi=np.concatenate(ghoi), gt_sizes=np.full((B, 2), 1, np.int32), gt_format=0, min_iou=0.5)
    return case, index, known


def check_known(got, case, index, known):
    for name, (labels, gts) in known.items():
        b = index[name]
        lo, hi = got["det_off"][b], got["det_off"][b + 1]
        assert list(np.asarray(got["label"][lo:hi])) == labels, f"{name}: labels {list(got['label'][lo:hi])}"
        assert list(np.asarray(got["gt"][lo:hi])) == gts, f"{name}: det_gt {list(got['gt'][lo:hi])}"
    b = index["nan_iou"]
    assert np.isnan(got["max_iou"][got["det_off"][b]])
    b = index["nan_beside_one"]
    lo = got["det_off"][b]
    assert np.isnan(got["max_iou"][lo]) and got["gt"][lo] == 1 and got["label"][lo] == 0
    assert got["status"][index["conversion_minus_one"]] & 1 and not got["status"][index["other_class"]]
