"""Test infrastructure for hg_region_priors (hoigen_amd/csrc/hg_region_props.hip), in the manner of hoi_head_bound.py.

  restate(...)        every stage in the kernels' own fp32 arithmetic, one rounding per operation (numpy float32): NMS with the coordinate
                      trick, the selection RULE, the prior row, the table T and the three layers in the kernel's order.  Expected bit for
                      bit.  `flaw` turns it into one of the wrong kernels of FLAWS (tests/test_props_model.py).
  select_literal(...) the reference's own statements (upt_tip_cache_model_free_finetune_distill3.py:1371-1398) on top of the restated
                      NMS, statement by statement in numpy; its argsort is made stable (the reference leaves ties open).
  definition(...)     float64: NMS on the float64 offset boxes, the literal selection, the literal get_prior row of E + 5 columns
                      (:1445-1488) through three float64 linears - no fold, no table.
  prior_bound(...)    per element, from the formats alone (u = 2^-24, gamma(k) = k u / (1 - k u)); per layer
                          e_out <= gamma(K + 1) (|b| + sum |x| |w|) + sum |w| e_in               (ReLU is 1-Lipschitz)
                      layer 0's e_in: the division's half ulp u |x_j| on the four box columns and gamma(E) sum |emb| |w| for T; its own
                      chain is 6 additions and 5 multiplies deep.  |x| is taken as |float64 activation| + e_in.
  screened(...)       an image is set aside from the INTEGER comparison with the float64 definition when some pair's IoU lies within the
                      fp32 arithmetic's error of the threshold: the offset coordinates carry half an ulp of c + off each (same-label boxes
                      share the offset, other pairs do not overlap), a length two of those plus its own rounding, and so on through the
                      quotient by interval arithmetic.  (A tie of the maximum coordinate leaves the maximum what it is: nothing to screen.)
  judge(...)          the three rules tests/test_gpu_region_props.py applies to a set of outputs, as one function, so that
                      tests/test_props_model.py can show that each wrong kernel of FLAWS fails them.

Order of the sums, fixed here and in the kernel: T and layers 1, 2 run over k ascending into one accumulator per (row, n); T starts
from 0, layers 1 and 2 from b[n]; layer 0 is ((((((T + b0) + s w0) + x1 w1) + y1 w2) + x2 w3) + y2 w4).  relu(v) = 0 where v < 0, else v.
"""
import functools

import numpy as np

F = np.float32
U = 2.0 ** -24
OUT = 64
FLAWS = ("score_gt", "iou_ge", "no_offset", "offset_no_plus1", "ties_reverse", "suppressed_suppresses", "min_from_prefix",
         "objects_first", "wh_swapped", "unnormalised", "pad_zeros", "relu_last", "missing_relu", "emb_input_position",
         "mask_inverted", "table_drops_col5")


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
def stable_order(scores, flaw=None):
    """descending score, ties to the lower input index (the kernel's rank by counting)"""
    idx = np.arange(len(scores))
    if flaw == "ties_reverse":
        return np.lexsort((-idx, -scores.astype(np.float64)))
    return np.lexsort((idx, -scores.astype(np.float64)))


def offset_boxes(boxes, labels, dtype=F, flaw=None):
    if len(boxes) == 0:
        return boxes.astype(dtype)
    m = dtype(boxes.max())
    t = m + dtype(1.0) if flaw != "offset_no_plus1" else m
    off = labels.astype(dtype) * dtype(t)
    if flaw == "no_offset":
        off = off * dtype(0)
    return boxes.astype(dtype) + off[:, None]


def iou_matrix(ob):
    """[Q, Q] of inter / ((area_i + area_j) - inter) in ob's dtype, one rounding per operation"""
    x1, y1, x2, y2 = ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3]
    area = (x2 - x1) * (y2 - y1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dx = np.where(x2[:, None] < x2[None, :], x2[:, None], x2[None, :]) - np.where(x1[:, None] > x1[None, :], x1[:, None], x1[None, :])
        dy = np.where(y2[:, None] < y2[None, :], y2[:, None], y2[None, :]) - np.where(y1[:, None] > y1[None, :], y1[:, None], y1[None, :])
        inter = np.where(dx > 0, dx, 0).astype(ob.dtype) * np.where(dy > 0, dy, 0).astype(ob.dtype)
        return inter / ((area[:, None] + area[None, :]) - inter)


def nms(scores, labels, boxes, thr, dtype=F, flaw=None):
    """indices of the survivors in descending-score order"""
    Q = len(scores)
    if Q == 0:
        return np.zeros(0, np.int64)
    order = stable_order(scores, flaw)
    iou = iou_matrix(offset_boxes(boxes, labels, dtype, flaw)[order])
    with np.errstate(invalid="ignore"):
        hit = iou >= dtype(thr) if flaw == "iou_ge" else iou > dtype(thr)
    removed = np.zeros(Q, bool)
    for i in range(Q):
        if removed[i] and flaw != "suppressed_suppresses":
            continue
        removed[i + 1:] |= hit[i, i + 1:]
    return order[~removed]


# ---- selection -----------------------------------------------------------------------------------------------------------------------
def select_rule(scores, labels, surv, human_idx, thr, mn, mx, flaw=None):
    """(keep: indices into the input list, humans first; n_human) by the rule of the header"""
    sc, lb = scores[surv], labels[surv]
    pre = sc > F(thr) if flaw == "score_gt" else sc >= F(thr)
    out = []
    for kind in (lb == human_idx, lb != human_idx):
        of_kind = np.nonzero(kind)[0]
        c = int((kind & pre).sum())
        if c < mn:
            k = min(mn, c if flaw == "min_from_prefix" else len(of_kind))
        elif c > mx:
            k = mx
        else:
            k = c
        out.append(surv[of_kind[:k]])
    if flaw == "objects_first":
        return np.concatenate(out[::-1]), len(out[0])
    return np.concatenate(out), len(out[0])


def select_literal(scores, labels, surv, human_idx, thr, mn, mx):
    """the reference's statements :1371-1398 on sc = scores[keep], lb = labels[keep] after the NMS; argsort made stable"""
    sc, lb = scores[surv], labels[surv]
    keep = np.nonzero(sc >= F(thr))[0]
    is_human = lb == human_idx
    hum, obj = np.nonzero(is_human)[0], np.nonzero(is_human == 0)[0]
    n_human = int(is_human[keep].sum())
    n_object = len(keep) - n_human
    desc = lambda v: np.argsort(-v.astype(np.float64), kind="stable")
    if n_human < mn:
        keep_h = hum[desc(sc[hum])[:mn]]
    elif n_human > mx:
        keep_h = hum[desc(sc[hum])[:mx]]
    else:
        keep_h = keep[np.nonzero(is_human[keep])[0]]
    if n_object < mn:
        keep_o = obj[desc(sc[obj])[:mn]]
    elif n_object > mx:
        keep_o = obj[desc(sc[obj])[:mx]]
    else:
        keep_o = keep[np.nonzero(is_human[keep] == 0)[0]]
    return surv[np.concatenate([keep_h, keep_o])], len(keep_h)


# ---- priors ---------------------------------------------------------------------------------------------------------------------------
def relu(v):
    return np.where(v < 0, v.dtype.type(0), v)


def table(emb, w0, flaw=None):
    """T [n_classes, hid] fp32: acc = 0; k ascending: acc = acc + emb[c][k] * w0[n][5 + k]"""
    emb, w0 = emb.astype(F), w0.astype(F)
    acc = np.zeros((emb.shape[0], w0.shape[0]), F)
    for k in range(1 if flaw == "table_drops_col5" else 0, emb.shape[1]):
        acc = acc + emb[:, k:k + 1] * w0[None, :, 5 + k]
    return acc


def linear_chain(x, w, b):
    """fp32 [rows, N]: acc = b[n]; k ascending: acc = acc + x[r][k] * w[n][k]"""
    acc = np.broadcast_to(b.astype(F), (x.shape[0], w.shape[0])).copy()
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * w[None, :, k].astype(F)
    return acc


def prior_rows(scores, boxes, labels, h, w, cap, wt, T, flaw=None, emb_labels=None):
    """priors [cap, 64] fp32 and mask [cap] of one image from its selected instances (n = len(scores) of them)"""
    n = len(scores)
    x = np.zeros((cap, 5), F)
    t = np.zeros((cap, T.shape[1]), F)
    if n:
        h, w = (F(w), F(h)) if flaw == "wh_swapped" else (F(h), F(w))
        if flaw == "unnormalised":
            h = w = F(1)
        x[:n, 0] = scores
        x[:n, 1], x[:n, 2], x[:n, 3], x[:n, 4] = boxes[:, 0] / w, boxes[:, 1] / h, boxes[:, 2] / w, boxes[:, 3] / h
        t[:n] = T[labels if emb_labels is None else emb_labels]
    w0 = wt["w0"].astype(F)
    v = t + wt["b0"].astype(F)[None]
    for j in range(5):
        v = v + x[:, j:j + 1] * w0[None, :, j]
    h0 = relu(v)
    h1 = linear_chain(h0, wt["w1"], wt["b1"])
    if flaw != "missing_relu":
        h1 = relu(h1)
    out = linear_chain(h1, wt["w2"], wt["b2"])
    if flaw == "relu_last":
        out = relu(out)
    if flaw == "pad_zeros":
        out[n:] = 0
    mask = np.arange(cap) >= n
    return out, (~mask if flaw == "mask_inverted" else mask)


# ---- a whole call -----------------------------------------------------------------------------------------------------------------------
def restate(case, flaw=None):
    """the outputs of hg_region_priors on `case` (see make_case) as numpy arrays, in the kernels' arithmetic"""
    p, B = case["params"], case["B"]
    cap, wt = 2 * p["max_instances"], case["weights"]
    T = table(wt["emb"], wt["w0"], flaw)
    out = dict(counts=np.zeros((B, 4), np.int32), keep=np.full((B, cap), -1, np.int32), boxes=np.zeros((B, cap, 4), F),
               scores=np.zeros((B, cap), F), labels=np.full((B, cap), -1, np.int32), survivors=[], priors=np.zeros((B, cap, OUT), F),
               mask=np.zeros((B, cap), np.uint8), table=T)
    for b in range(B):
        lo, hi = case["q_off"][b], case["q_off"][b + 1]
        sc, lb, bx = case["scores"][lo:hi], case["labels"][lo:hi], case["boxes"][lo:hi]
        status = 0 if np.isfinite(sc).all() and np.isfinite(bx).all() else 1
        if ((lb < 0) | (lb >= len(wt["emb"]))).any():
            status |= 2
        surv = keep = np.zeros(0, np.int64)
        n_h = 0
        if not status:
            surv = nms(sc, lb, bx, p["nms_thresh"], F, flaw)
            keep, n_h = select_rule(sc, lb, surv, p["human_idx"], p["box_score_thresh"], p["min_instances"], p["max_instances"], flaw)
        n = len(keep)
        out["counts"][b] = (n, n_h, status, len(surv))
        out["keep"][b, :n], out["boxes"][b, :n], out["scores"][b, :n], out["labels"][b, :n] = keep, bx[keep], sc[keep], lb[keep]
        out["survivors"].append(surv.astype(np.int32))
        h, w = case["image_sizes"][b]
        emb_labels = lb[:n] if flaw == "emb_input_position" else None
        out["priors"][b], m = prior_rows(sc[keep], bx[keep], lb[keep], h, w, cap, wt, T, flaw, emb_labels)
        out["mask"][b] = m
    return out


def definition(case):
    """float64: per image (keep, n_human, survivors), priors [B, cap, 64] float64 of the literal get_prior + MLP, and the bound"""
    p, B = case["params"], case["B"]
    cap, wt = 2 * p["max_instances"], {k: v.astype(np.float64) for k, v in case["weights"].items()}
    E = wt["emb"].shape[1]
    ints, priors, bound = [], np.zeros((B, cap, OUT)), np.zeros((B, cap, OUT))
    a0, a1, a2 = np.abs(wt["w0"]), np.abs(wt["w1"]), np.abs(wt["w2"])
    for b in range(B):
        lo, hi = case["q_off"][b], case["q_off"][b + 1]
        sc, lb, bx = case["scores"][lo:hi], case["labels"][lo:hi], case["boxes"][lo:hi]
        ok = np.isfinite(sc).all() and np.isfinite(bx).all()
        surv = nms(sc, lb, bx, F(p["nms_thresh"]), np.float64) if ok else np.zeros(0, np.int64)
        keep, n_h = select_literal(sc, lb, surv, p["human_idx"], p["box_score_thresh"], p["min_instances"], p["max_instances"]) if ok else (surv, 0)
        ints.append((keep, n_h, surv))
        n = len(keep)
        h, w = (np.float64(v) for v in case["image_sizes"][b])
        row = np.zeros((cap, E + 5))
        row[:n, 0] = sc[keep]
        row[:n, 1:5] = bx[keep].astype(np.float64) / np.array([w, h, w, h])
        row[:n, 5:] = wt["emb"][lb[keep]]
        h0 = np.maximum(row @ wt["w0"].T + wt["b0"], 0)
        h1 = np.maximum(h0 @ wt["w1"].T + wt["b1"], 0)
        priors[b] = h1 @ wt["w2"].T + wt["b2"]
        arow = np.abs(row)
        e0 = gamma(E + 7) * (arow @ a0.T + np.abs(wt["b0"])) + U * (arow[:, 1:5] @ a0[:, 1:5].T)
        e1 = gamma(a1.shape[1] + 1) * ((h0 + e0) @ a1.T + np.abs(wt["b1"])) + e0 @ a1.T
        e2 = gamma(a2.shape[1] + 1) * ((h1 + e1) @ a2.T + np.abs(wt["b2"])) + e1 @ a2.T
        bound[b] = e2 * (1 + 1e-9)
    return ints, priors, bound


def screened(case, b):
    """True when some pair of image b has an IoU within the fp32 arithmetic's error of the threshold"""
    lo, hi = case["q_off"][b], case["q_off"][b + 1]
    return near_threshold(case["labels"][lo:hi], case["boxes"][lo:hi], case["params"]["nms_thresh"])


def near_threshold(lb, bx, nms_thresh):
    if len(lb) < 2 or not np.isfinite(bx).all():
        return False
    ob = offset_boxes(bx, lb, np.float64)
    d = U * np.abs(ob).max() * (1 + 2 * U)      # half an ulp of an offset coordinate (the offset's own roundings shift whole labels)
    x1, y1, x2, y2 = ob.T
    dx = np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None])
    dy = np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None])
    e = lambda v: 2 * d + U * np.abs(v)         # a length: two coordinates and its own rounding
    r = 1 + 4 * U                               # the product, the sum and the difference around it
    i_lo = np.maximum(dx - e(dx), 0) * np.maximum(dy - e(dy), 0) / r
    i_hi = np.maximum(dx + e(dx), 0) * np.maximum(dy + e(dy), 0) * r
    bw, bh = x2 - x1, y2 - y1
    a_lo, a_hi = np.maximum(bw - e(bw), 0) * np.maximum(bh - e(bh), 0) / r, (bw + e(bw)) * (bh + e(bh)) * r
    u_lo, u_hi = (a_lo[:, None] + a_lo[None] - i_hi) / r, (a_hi[:, None] + a_hi[None] - i_lo) * r
    with np.errstate(invalid="ignore", divide="ignore"):
        q_lo, q_hi = i_lo / u_hi / r, np.where(u_lo > 0, i_hi / u_lo * r, np.inf)
    thr = np.float64(F(nms_thresh))
    near = (q_lo <= thr) & (thr <= q_hi) & (i_hi > 0)
    np.fill_diagonal(near, False)
    return bool(near.any())


def judge(got, case, expected=None, defn=None, skip_rule3=()):
    """the rules of the GPU test on one set of outputs; raises AssertionError with the first thing that is off"""
    exp = expected if expected is not None else restate(case)
    B = case["B"]
    # rule 1: bit for bit against the restatement
    for k in ("counts", "keep", "labels", "mask"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), exp[k].astype(np.int64)), f"rule 1: {k}"
    for b in range(B):
        assert np.array_equal(np.asarray(got["survivors"][b]), exp["survivors"][b]), f"rule 1: survivors of image {b}"
    for k in ("boxes", "scores", "table", "priors"):
        assert np.array_equal(np.asarray(got[k], F).view(np.uint32), exp[k].view(np.uint32)), f"rule 1: {k}"
    ints, pri, bound = defn if defn is not None else definition(case)
    # rule 2: priors within the derived bound of the float64 definition (images whose integers agree with it: same rows)
    # rule 3: the integers are the definition's, but for the images the screen sets aside
    worst = 0.0
    for b in range(B):
        keep, n_h, surv = ints[b]
        n = int(got["counts"][b][0])
        same = n == len(keep) and np.array_equal(np.asarray(got["keep"][b][:n]), keep)
        assert np.array_equal(np.asarray(got["mask"][b]) != 0, np.arange(len(got["mask"][b])) >= n), f"rule 3: mask of image {b}"
        if b not in skip_rule3 and not screened(case, b):
            assert same and int(got["counts"][b][1]) == n_h, f"rule 3: selection of image {b}"
            assert np.array_equal(np.asarray(got["survivors"][b]), surv), f"rule 3: survivors of image {b}"
        if same:
            err = np.abs(np.asarray(got["priors"][b], np.float64) - pri[b])
            assert (err <= bound[b]).all(), f"rule 2: image {b}: worst |err| / E = {(err / bound[b]).max():.3f}"
            worst = max(worst, float((err / np.maximum(bound[b], 1e-300)).max()))
    return worst


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def make_weights(E, hid, n_classes, seed):
    r = np.random.RandomState(seed)
    lin = lambda o, i: ((r.rand(o, i) * 2 - 1) / np.sqrt(i)).astype(F)
    return dict(w0=lin(hid, E + 5), b0=lin(1, hid)[0], w1=lin(hid, hid), b1=lin(1, hid)[0], w2=lin(OUT, hid), b2=lin(1, OUT)[0],
                emb=(r.randn(n_classes, E) / np.sqrt(E)).astype(F) * F(4))


def random_image(r, Q, n_classes, human_idx, h, w, p_human=0.35):
    """clustered boxes (a handful of centres, jittered copies: many pairs near and over the threshold), distinct scores"""
    k = max(1, Q // 6)
    cx, cy = r.rand(k) * w, r.rand(k) * h
    bw, bh = (0.08 + 0.3 * r.rand(k)) * w, (0.08 + 0.3 * r.rand(k)) * h
    c = r.randint(0, k, Q)
    jit = lambda s: 1 + 0.25 * (r.rand(Q) - 0.5) * s
    x, y, ww, hh = cx[c] + 0.2 * bw[c] * (r.rand(Q) - 0.5), cy[c] + 0.2 * bh[c] * (r.rand(Q) - 0.5), bw[c] * jit(1), bh[c] * jit(1)
    boxes = np.stack([x - ww / 2, y - hh / 2, x + ww / 2, y + hh / 2], 1).clip(0, [w, h, w, h]).astype(F)
    cls_of = np.where(r.rand(k) < p_human, human_idx, r.randint(0, n_classes, k))
    labels = np.where(r.rand(Q) < 0.85, cls_of[c], r.randint(0, n_classes, Q)).astype(np.int64)
    scores = (r.permutation(Q * 4)[:Q].astype(np.float64) / (Q * 4) * 0.98 + 0.01).astype(F)      # distinct
    return scores, labels, boxes


def pack(images, sizes, params, weights):
    q_off = np.concatenate([[0], np.cumsum([len(s) for s, _, _ in images])]).astype(np.int64)
    cat = lambda i, dt, shape: np.concatenate([np.asarray(im[i], dt).reshape(shape) for im in images] + [np.zeros(0, dt).reshape(shape)])
    return dict(B=len(images), q_off=q_off, scores=cat(0, F, (-1,)), labels=cat(1, np.int64, (-1,)), boxes=cat(2, F, (-1, 4)),
                image_sizes=np.asarray(sizes, F).reshape(-1, 2), params=dict(params), weights=weights)


PARAMS = dict(human_idx=0, box_score_thresh=0.2, min_instances=3, max_instances=15, nms_thresh=0.5)
Q_EDGES = (0, 1, 2, 63, 64, 65, 100, 128, 129, 512)
# family: (Q per image, classes, E, hidden, human_idx, parameter overrides)
FAMILIES = {
    "q_edges_81": (Q_EDGES, 81, 512, 128, 1, {}),
    "b1_2cls_e768": ((100,), 2, 768, 128, 0, {}),
    "b3_ragged_2cls": ((37, 5, 90), 2, 512, 96, 0, {}),
    "b8_81": ((100,) * 8, 81, 512, 128, 1, {}),
    "b64_81": (tuple(20 + (7 * i) % 41 for i in range(64)), 81, 512, 128, 1, {}),
    "cap64_hid256": ((200, 130, 64), 81, 512, 256, 1, dict(max_instances=32, box_score_thresh=0.05)),
    "cap8": ((60, 33), 2, 512, 128, 0, dict(max_instances=4, min_instances=2, box_score_thresh=0.5)),
}


@functools.lru_cache(maxsize=None)
def family(name):
    Qs, ncls, E, hid, human, over = FAMILIES[name]
    r = np.random.RandomState(sum(map(ord, name)))
    sizes = [(float(r.randint(300, 700)), float(r.randint(300, 900))) for _ in Qs]
    images = []
    for Q, (h, w) in zip(Qs, sizes):      # an image the screen would set aside is drawn again (test_props_model.py holds the family to its cap)
        for _ in range(40):
            im = random_image(r, Q, ncls, human, h, w)
            if not near_threshold(im[1], im[2], PARAMS["nms_thresh"]):
                break
        images.append(im)
    return pack(images, sizes, dict(PARAMS, human_idx=human, **over), make_weights(E, hid, ncls, 7 + len(Qs)))


def grid_boxes(n, x0=0.0, step=40.0, side=20.0):
    """n boxes that do not touch each other"""
    return np.array([[x0 + step * i, 10.0, x0 + step * i + side, 10.0 + side] for i in range(n)], F).reshape(-1, 4)


def counts_image(n_h, n_o, extra_low=2):
    """n_h humans and n_o objects above the threshold, `extra_low` of each below it, none overlapping; scores distinct, interleaved"""
    lab = np.array([0] * n_h + [1] * n_o + [0] * extra_low + [1] * extra_low, np.int64)
    n = len(lab)
    sc = np.concatenate([0.9 - 0.01 * np.arange(n_h + n_o)[::-1], 0.1 - 0.01 * np.arange(2 * extra_low)]).astype(F)
    return sc, lab, grid_boxes(n)


@functools.lru_cache(maxsize=None)
def constructed():
    """the hand-built images, one call: (case, {name: image index}, known answers {name: keep})"""
    mn, mx = 2, 4
    P = dict(PARAMS, min_instances=mn, max_instances=mx, box_score_thresh=0.5)
    im, known = {}, {}
    box = [10.0, 10.0, 50.0, 50.0]
    im["duplicates"] = ([0.9, 0.8, 0.7, 0.6], [0, 0, 1, 1], [box, box, [60, 60, 90, 90], [60, 60, 90, 90]])
    known["duplicates"] = [0, 2]
    # IoU exactly 0.5: [0,0,2,2] and [0,0,2,1]... inter 2, union 4; exact through the offset (small integers); not > 0.5: both stay
    im["iou_half"] = ([0.9, 0.8, 0.7], [1, 1, 0], [[0, 0, 2, 2], [0, 0, 2, 1], [100, 100, 120, 120]])
    known["iou_half"] = [2, 0, 1]
    im["two_labels"] = ([0.9, 0.8], [0, 1], [box, box])
    known["two_labels"] = [0, 1]
    # no positive coordinate: the maximum is 0 and the `+ 1` alone keeps the labels apart
    im["nonpositive"] = ([0.9, 0.8], [0, 1], [[-1, -1, 0, 0], [-1, -1, 0, 0]])
    known["nonpositive"] = [0, 1]
    # zero-area boxes: two identical ones give 0 / 0 = NaN, not > thr: both stay; one inside a real box has IoU 0
    im["zero_area"] = ([0.9, 0.8, 0.7], [1, 1, 1], [[5, 5, 5, 5], [5, 5, 5, 5], [0, 0, 10, 10]])
    known["zero_area"] = [0, 1, 2]
    # tied scores: the stable order keeps 0 before 1; they overlap, so WHICH of them survives depends on the order
    im["tied"] = ([0.75, 0.75, 0.75, 0.6], [0, 0, 1, 1], [[0, 0, 40, 40], [2, 0, 42, 40], [100, 0, 140, 40], [200, 0, 240, 40]])
    known["tied"] = [0, 2, 3]
    im["at_threshold"] = ([0.9, 0.5, 0.8, 0.7, 0.5, 0.4], [0, 0, 0, 1, 1, 1], grid_boxes(6))      # mn = 2: the 0.5s count (>=): h = 3, o = 2
    known["at_threshold"] = [0, 2, 1, 3, 4]
    im["all_below"] = ([0.4, 0.3, 0.2, 0.1, 0.35], [0, 0, 0, 1, 1], grid_boxes(5))                  # the minimum draws from everything
    known["all_below"] = [0, 1, 4, 3]
    for nh, no in ((mn - 1, mx + 1), (mn, mx), (mx, mn), (mx + 1, mn - 1)):
        im[f"counts_{nh}_{no}"] = counts_image(nh, no)
    im["no_human"] = ([0.9, 0.8, 0.7], [1, 2, 1], grid_boxes(3))
    known["no_human"] = [0, 1, 2]
    im["one_box"] = ([0.9], [0], [box])
    known["one_box"] = [0]
    im["min_exceeds"] = ([0.1, 0.05], [0, 1], grid_boxes(2))                                        # min_instances 2, one of each kind
    known["min_exceeds"] = [0, 1]
    im["empty"] = ([], [], np.zeros((0, 4), F))
    known["empty"] = []
    names = list(im)
    images = [(np.asarray(s, F), np.asarray(l, np.int64), np.asarray(b, F).reshape(-1, 4)) for s, l, b in im.values()]
    sizes = [(480.0, 640.0)] * len(images)
    return pack(images, sizes, P, make_weights(512, 128, 3, 3)), {n: i for i, n in enumerate(names)}, known


def case_images(case, which):
    """the sub-batch of the images `which`"""
    ims = [(case["scores"][case["q_off"][b]:case["q_off"][b + 1]], case["labels"][case["q_off"][b]:case["q_off"][b + 1]],
            case["boxes"][case["q_off"][b]:case["q_off"][b + 1]]) for b in which]
    return pack(ims, case["image_sizes"][list(which)], case["params"], case["weights"])
