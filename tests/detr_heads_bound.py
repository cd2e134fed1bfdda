"""What the DETR heads kernel (hoigen_amd/csrc/hg_detr_heads.hip: class_embed, bbox_embed with its sigmoid and PostProcess in one launch;
the reference's upt_tip_cache_model_free_finetune_distill3.py:1598-1605 over detr/models/detr.py:37-38, :269-282, :293-305) is held to:
the statements in float64 on the CPU from the UNROUNDED operands (hs and the weights as the caller holds them, fp32), and a bound PER
ELEMENT that sums the worst case of every rounding the kernel performs.  A plain module beside the tests: no fixtures, no GPU, no library.

All float64, u = 2^-24.  For one linear y = sum_k a_k W_k + b whose input the kernel holds as a^ with |a^ - a| <= ea and whose weight it
holds as W^ = fp16(W) (eW = |W^ - W|, the ACTUAL rounding: zero for weights that are fp16 numbers):

    E_y = sum_k (ea_k |W_k| + |a_k| eW_k + ea_k eW_k)        the operands' errors through the product
        + D u S,  S = sum_k (|a_k| + ea_k)(|W_k| + eW_k)      fp32 accumulation of D products (D u sum |a| |b|)
        + u (S (1 + D u) + |b|)                               the bias add after the sum

  input        ea = |fp16(hs) - hs|, the actual rounding (round to nearest even)
  logits       E_logit = E_y of class_embed (the rows of class_rows where given)
  hidden       h = relu(y), kept as fp16(relu(y^)): e_h = E_y + 2^-11 (h + E_y) + 2^-25, and 0 where y < -E_y (an exact zero either way)
  t            three layers of that; the last without ReLU and rounding
  pred_box     sigma(t) = 1 / (1 + expf(-t)): E_t times the steepest slope of sigma over [t - E_t, t + E_t], plus the roundings
               sigma ((1 - sigma) EXP + u + DIV) - expf, the add, the division - `sigmoid_rounding`
  score        p_j = exp(l_j) / sum_c exp(l_c) moves with the logits by at most a factor exp(E_j + ln sum_c p_c exp(E_c)); the arithmetic
               adds eta_j + sum_c p_c eta_c + C1 u + DIV with eta_c = u |l_c - m| + EXP (the subtraction, expf), the sum of C1 positive
               terms in any order and the division; 1e-37 absolute for results below fp32's normal range
  boxes        (E_cx + E_w / 2) W (1 + 2 u) + 2 u |x|: the subtraction or addition and the multiplication, rounded one by one

EXP = 8 u (4 ulp) and DIV = 5 u (2.5 ulp) are the ASSUMED figures of tests/elem_bound.py for the device's expf and division; they are
assumptions there and stay assumptions here.

Rule: every element has |got - want| <= bound.  The two exact families hold fp16 numbers whose products and partial sums are exact in
fp32 in any order (`exact_margin` states the condition and the CPU test asserts it): there the logits are compared BIT FOR BIT with
`model()` and with the reference, pred_boxes with sigma(model's t) inside `sigmoid_rounding` alone - t itself does not leave the kernel -,
and the labels exactly, with planted equal foreground maxima (the tie goes to the lower index) and rows whose no-object column is the
greatest.

Labels elsewhere (`check_labels`): a row is AMBIGUOUS if the two greatest foreground logits of the reference are closer than the sum of
their two bounds.  An ambiguous row is not skipped: its label must be one of the classes c with max - l_c < E_max + E_c, and its score
must meet the bound of that class's probability.  Every other row's label must equal the reference's.  At most 15 % of the rows of a
case may be ambiguous (`MAX_AMBIGUOUS`; the CPU test asserts it for every case).

`model()` restates the kernel in fp16 / fp32: x16 = fp16(hs); every linear accumulates fp32 over k in ascending blocks of 32 from zero and
adds the bias after the sum; h1, h2 = fp16(relu(.)), one rounding each; pred_box = 1 / (1 + exp(-t)) in fp32; the softmax as eight
threads a row compute it (thread s sums columns s, s + 8, .. in ascending order, then the xor butterfly 1, 2, 4); the boxes with one
rounding per operation.  numpy's expf is not the device's, so only the logits, t, the labels of unambiguous rows and - given pred_boxes -
the boxes are bit-level statements.

Families (`make_case`; seeded):
    exact_int   hs integers / 4 in [-1, 1], matrices integers / 2 in [-1, 1], biases integers / 8; layers.2 has 16 nonzeros a row,
                integers in [-2, 2] times 2^-7
    exact_pow2  hs, matrices and biases +-2^-e, e in 0 .. 3; layers.2 16 nonzeros a row, +-2^-6 or +-2^-7
                both: channels 0 and 1 of hs select the row's kind by r mod 4 - 0 plain; 1 the foreground pair A boosted by 512 in both
                columns (rows of class_embed equal: a tie at the maximum); 2 the pair B = (0, 8) likewise (the same thread's columns;
                C1 >= 11); 3 the no-object column boosted
    randn       LayerNorm-like rows (normalised randn times 1 +- 0.2, plus 0.1 randn), Xavier-uniform matrices, 0.1 randn biases
    outlier     randn with every 37th channel of hs times 64
    cancel      the second half of hs equal to the first plus 2^-6 randn, hs times 2, the second half of every layers.0 row minus the first
                and of every class_embed row minus the first plus a quarter of a Xavier draw: products thirty times the logits they
                leave; class biases randn
    saturate    layers.2.bias = (24, -24, 30, -30) and 4 x Xavier weights: |t| up to 30 and beyond, the sigmoid meets 0 and 1; one class
                40 above the rest: its score is 1 - tiny
"""
import numpy as np

from elem_bound import DIV, EXP

U = 2.0 ** -24
ROWS = 32
MAX_AMBIGUOUS = 0.15
FAMILIES = ("exact_int", "exact_pow2", "randn", "outlier", "cancel", "saturate")
EXACT_FAMILIES = ("exact_int", "exact_pow2")
MUTANTS = ("softmax_foreground_only", "max_with_no_object", "tie_to_higher", "no_relu_2", "no_sigmoid", "full_width", "hw_swapped",
           "scale_of_image_0", "truncate_f16", "class_rows_ignored", "level_0", "padded_column")
SHAPES = ((1, 1, 1), (1, 1, 31), (1, 2, 33), (2, 1, 257), (6, 3, 100))
C1S = (2, 17, 81, 92, 256)
# the seed of the cases both tests run: the one-row shape is a case of its own, and its single row must not be ambiguous (seeds 20, 23 and
# 24 each draw one such row among the 200 non-exact cases; 21 and 22 draw none and stay below 11 % everywhere) - a property of the
# inputs, computed from the float64 reference and the bound alone, which the CPU test asserts
SEED = 22


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def make_case(family, L, B, Q, D, C1, seed, class_rows=None):
    """class_rows (C1 of them): the head made for the case becomes those rows, in that order, of a larger class_embed of
    max(class_rows) + 3 rows whose other rows are noise - the V-COCO path"""
    r = np.random.default_rng([seed, L, B, Q, D, C1, FAMILIES.index(family)])
    n = lambda *s: r.standard_normal(s)
    xav = lambda o, i: r.uniform(-1, 1, (o, i)) * np.sqrt(6.0 / (o + i))
    M = L * B * Q
    if family == "exact_int":
        x, wc, w0, w1 = r.integers(-4, 5, (M, D)) / 4, r.integers(-2, 3, (C1, D)) / 2, r.integers(-2, 3, (D, D)) / 2, r.integers(-2, 3, (D, D)) / 2
        bc, b0, b1, b2 = r.integers(-8, 9, C1) / 8, r.integers(-8, 9, D) / 8, r.integers(-8, 9, D) / 8, r.integers(-8, 9, 4) / 8
        w2 = np.zeros((4, D))
        for i in range(4):
            w2[i, r.choice(D, 16, replace=False)] = r.integers(-2, 3, 16) * 2.0 ** -7
    elif family == "exact_pow2":
        p2 = lambda *s: r.choice([-1.0, 1.0], s) * 2.0 ** -r.integers(0, 4, s)
        x, wc, w0, w1, bc, b0, b1, b2 = p2(M, D), p2(C1, D), p2(D, D), p2(D, D), p2(C1), p2(D), p2(D), p2(4)
        w2 = np.zeros((4, D))
        for i in range(4):
            w2[i, r.choice(D, 16, replace=False)] = r.choice([-1.0, 1.0], 16) * 2.0 ** -r.integers(6, 8, 16)
    else:
        x = n(M, D)
        x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True) * (1 + 0.2 * n(D)) + 0.1 * n(D)
        wc, w0, w1, w2 = xav(C1, D), xav(D, D), xav(D, D), xav(4, D)
        bc, b0, b1, b2 = 0.1 * n(C1), 0.1 * n(D), 0.1 * n(D), 0.1 * n(4)
        if family == "outlier":
            x[:, ::37] *= 64
        elif family == "cancel":
            x[:, D // 2:] = x[:, :D // 2] + 2.0 ** -6 * n(M, D // 2)
            x *= 2
            wc[:, D // 2:] = -wc[:, :D // 2] + 0.25 * xav(C1, D // 2)
            w0[:, D // 2:] = -w0[:, :D // 2]
            bc = n(C1)
        elif family == "saturate":
            w2, b2 = 4 * w2, np.array([24.0, -24.0, 30.0, -30.0])
            bc[3 % max(C1 - 1, 1)] += 40
    if family in EXACT_FAMILIES:
        kind = np.arange(M) % 4
        x[:, 0], x[:, 1] = np.where(kind == 1, 1.0, np.where(kind == 3, -1.0, 0.0)), np.where(kind == 2, 1.0, 0.0)
        wc[:, :2] = 0
        pairs = []
        if C1 >= 4:
            pairs.append((1, C1 - 2, 0))
        elif C1 == 3:
            pairs.append((0, 1, 0))
        if C1 >= 11:
            pairs.append((0, 8, 1))
        for lo, hi, ch in pairs:
            wc[hi], bc[hi] = wc[lo], bc[lo]
            wc[lo, ch] = wc[hi, ch] = 512.0
        wc[C1 - 1, 0] = -512.0
    sizes = np.array([(480 + 37 * b, 640 - 53 * b) for b in range(B)], np.float64)      # (h, w), different for every image
    c = dict(hs=x.reshape(L, B, Q, D), wc=wc, bc=bc, w0=w0, b0=b0, w1=w1, b1=b1, w2=w2, b2=b2, sizes=sizes)
    c = {k: np.ascontiguousarray(v, np.float32) for k, v in c.items()}
    if class_rows is not None:      # the C1 rows made above become rows class_rows of a larger head; the other rows are noise
        class_rows = list(class_rows)
        assert len(class_rows) == C1
        nl = max(class_rows) + 3
        big_w, big_b = (7 * n(nl, D)).astype(np.float32), (7 * n(nl)).astype(np.float32)
        big_w[class_rows], big_b[class_rows] = c["wc"], c["bc"]
        c["wc"], c["bc"] = big_w, big_b
    return c | dict(family=family, L=L, B=B, Q=Q, D=D, C1=C1, class_rows=None if class_rows is None else list(class_rows))


def class_head(c, ignore_rows=False):
    """(weight [C1, D], bias [C1]) fp32 as the loader gathers them"""
    if c["class_rows"] is None or ignore_rows:
        return c["wc"][:c["C1"]], c["bc"][:c["C1"]]
    return c["wc"][c["class_rows"]], c["bc"][c["class_rows"]]


def _xyxy_scaled(pb, sizes):
    """box_cxcywh_to_xyxy and the scale, in pb's dtype with one rounding per operation; pb [B, Q, 4], sizes [B, 2] = (h, w)"""
    cx, cy, w, h = (pb[..., i] for i in range(4))
    half = pb.dtype.type(0.5)
    hw, hh = half * w, half * h
    W, H = sizes[:, None, 1].astype(pb.dtype), sizes[:, None, 0].astype(pb.dtype)
    return np.stack([(cx - hw) * W, (cy - hh) * H, (cx + hw) * W, (cy + hh) * H], -1)


def boxes_fp32(pred_boxes_last, sizes):
    """the fp32 restatement of the six operations on the returned pred_boxes [B, Q, 4]: what `boxes` must equal bit for bit"""
    return _xyxy_scaled(np.asarray(pred_boxes_last, np.float32), np.asarray(sizes, np.float32))


def reference(c):
    """float64 from the unrounded operands: logits [L, B, Q, C1], t, pred_boxes [L, B, Q, 4], prob [B, Q, C1] (last level), scores,
    labels [B, Q], boxes [B, Q, 4]"""
    d = {k: np.asarray(v, np.float64) for k, v in c.items() if isinstance(v, np.ndarray)}
    wc, bc = (np.asarray(a, np.float64) for a in class_head(c))
    x = d["hs"]
    logits = x @ wc.T + bc
    h = np.maximum(x @ d["w0"].T + d["b0"], 0)
    h = np.maximum(h @ d["w1"].T + d["b1"], 0)
    t = h @ d["w2"].T + d["b2"]
    pb = 1 / (1 + np.exp(-t))
    last = logits[-1]
    e = np.exp(last - last.max(-1, keepdims=True))
    prob = e / e.sum(-1, keepdims=True)
    labels = last[..., :-1].argmax(-1)
    scores = np.take_along_axis(prob, labels[..., None], -1)[..., 0]
    return dict(logits=logits, t=t, pred_boxes=pb, prob=prob, scores=scores, labels=labels, boxes=_xyxy_scaled(pb[-1], d["sizes"]))


def _layer(a, ea, W, b, exact):
    """-> (y, E_y) of y = a W^T + b"""
    W16 = f16(W).astype(np.float64)
    eW = np.abs(W16 - W)
    y = a @ W.T + b
    S = (np.abs(a) + ea) @ (np.abs(W) + eW).T
    E = ea @ np.abs(W).T + np.abs(a) @ eW.T + ea @ eW.T
    if not exact:
        E = E + W.shape[1] * U * S + U * (S * (1 + W.shape[1] * U) + np.abs(b))
    return y, E


def _hidden(y, E):
    h = np.maximum(y, 0)
    return h, np.where(y < -E, 0.0, E + 2.0 ** -11 * (h + E) + 2.0 ** -25)


def sigmoid_rounding(t):
    """the roundings of 1 / (1 + expf(-t)) given t: expf (EXP), the add (u), the division (DIV), 1 % for the second order"""
    s = 1 / (1 + np.exp(-np.asarray(t, np.float64)))
    return 1.01 * s * ((1 - s) * EXP + U + DIV) + 1e-37


def bounds(c):
    """per element, float64: logits, pred_boxes [L, B, Q, .], prob [B, Q, C1] (the bound of every class's probability as a score), boxes"""
    d = {k: np.asarray(v, np.float64) for k, v in c.items() if isinstance(v, np.ndarray)}
    exact = c["family"] in EXACT_FAMILIES
    wc, bc = (np.asarray(a, np.float64) for a in class_head(c))
    x = d["hs"]
    ex = np.abs(f16(c["hs"]).astype(np.float64) - x)
    logits, E_l = _layer(x, ex, wc, bc, exact)
    h, e = _hidden(*_layer(x, ex, d["w0"], d["b0"], exact))
    h, e = _hidden(*_layer(h, e, d["w1"], d["b1"], exact))
    t, E_t = _layer(h, e, d["w2"], d["b2"], exact)
    sig = lambda v: 1 / (1 + np.exp(-v))
    nearest0 = np.where(np.abs(t) <= E_t, 0.0, t - np.sign(t) * E_t)
    pb = sig(t)
    E_pb = E_t * sig(nearest0) * (1 - sig(nearest0)) + np.maximum(sigmoid_rounding(t - E_t), sigmoid_rounding(t + E_t))
    last, El = logits[-1], E_l[-1]
    m = last.max(-1, keepdims=True)
    p = np.exp(last - m)
    p = p / p.sum(-1, keepdims=True)
    eta = U * (np.abs(last - m) + 2 * El.max(-1, keepdims=True)) + EXP
    arith = eta + (p * eta).sum(-1, keepdims=True) + c["C1"] * U + DIV
    E_p = p * np.expm1(El + np.log((p * np.exp(El)).sum(-1, keepdims=True)) + 1.01 * arith) + 1e-37
    bx = _xyxy_scaled(pb[-1], d["sizes"])
    Ecx, Ecy, Ew, Eh = (E_pb[-1][..., i] for i in range(4))
    W, H = d["sizes"][:, None, 1], d["sizes"][:, None, 0]
    E_b = np.stack([(Ecx + Ew / 2) * W, (Ecy + Eh / 2) * H, (Ecx + Ew / 2) * W, (Ecy + Eh / 2) * H], -1) * (1 + 2 * U) + 2 * U * np.abs(bx)
    return dict(logits=E_l, pred_boxes=E_pb, prob=E_p, boxes=E_b)


def exact_margin(c):
    """For an exact family: the greatest sum_k |a_k| |W_k| of every linear over 2^24 quanta of its terms - below 1, every partial sum in any
    order is an integer number of quanta below 2^24, so nothing is rounded in fp32.  -> the worst of the four layers"""
    assert c["family"] in EXACT_FAMILIES
    q = {"exact_int": (2.0 ** -3, 2.0 ** -3, 2.0 ** -4, 2.0 ** -11), "exact_pow2": (2.0 ** -6, 2.0 ** -6, 2.0 ** -9, 2.0 ** -16)}[c["family"]]
    m = model(c)
    x = c["hs"].reshape(-1, c["D"]).astype(np.float64)
    wc, bc = class_head(c)
    sums = [(np.abs(x) @ np.abs(wc.astype(np.float64)).T + np.abs(bc)).max(), (np.abs(x) @ np.abs(c["w0"].astype(np.float64)).T + np.abs(c["b0"])).max(),
            (m["h1"].astype(np.float64) @ np.abs(c["w1"].astype(np.float64)).T + np.abs(c["b1"])).max(),
            (m["h2"].astype(np.float64) @ np.abs(c["w2"].astype(np.float64)).T + np.abs(c["b2"])).max()]
    return max(s / (2.0 ** 24 * qi) for s, qi in zip(sums, q))


# ---- the kernel's arithmetic in fp16 / fp32 --------------------------------------------------------------------------------------------
def _mm_blocks(a, w, step=32):
    """fp32: sum over k in ascending blocks of `step`, accumulated from zero; a [M, K], w [N, K]"""
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(0, a.shape[1], step):
        acc = acc + (a[:, k:k + step].astype(np.float64) @ w[:, k:k + step].astype(np.float64).T).astype(np.float32)
    return acc


def _to_f16(v, truncate=False):
    v = np.asarray(v, np.float32)
    h = v.astype(np.float16)
    if truncate:      # toward zero: the nearest fp16 not above |v|
        over = np.abs(h.astype(np.float32)) > np.abs(v)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def _softmax_rows(lg, n_max):
    """lg [R, C] fp32 -> (m, sum, label): the maximum over all columns, the sum of expf(l - m) as eight threads compute it, the lowest
    index of the greatest of the first n_max columns"""
    R, C = lg.shape
    m = lg.max(-1, keepdims=True)
    e = np.exp(lg - m, dtype=np.float32)
    pad = np.zeros((R, (C + 7) // 8 * 8), np.float32)
    pad[:, :C] = e
    pad = pad.reshape(R, -1, 8)
    p = np.zeros((R, 8), np.float32)
    for i in range(pad.shape[1]):
        p = p + pad[:, i]
    for o in (1, 2, 4):
        p = p + p[:, np.arange(8) ^ o]
    return m[:, 0], p[:, 0], lg[:, :n_max].argmax(-1)


def model(c, mutant=None):
    """fp32 as the kernel computes them: logits [L, B, Q, C1], h1, h2 [M, D], t, pred_boxes [L, B, Q, 4], scores, labels (int64), boxes of
    the last level; `mutant`: one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS
    L, B, Q, D, C1 = c["L"], c["B"], c["Q"], c["D"], c["C1"]
    trunc = mutant == "truncate_f16"
    wc, bc = class_head(c, ignore_rows=mutant == "class_rows_ignored")
    x16 = _to_f16(c["hs"].reshape(-1, D), trunc)
    logits = (_mm_blocks(x16, _to_f16(wc, trunc)) + bc).reshape(L, B, Q, C1)
    h1 = _to_f16(np.maximum(_mm_blocks(x16, _to_f16(c["w0"], trunc)) + c["b0"], np.float32(0)), trunc)
    a2 = _mm_blocks(h1, _to_f16(c["w1"], trunc)) + c["b1"]
    h2 = _to_f16(a2 if mutant == "no_relu_2" else np.maximum(a2, np.float32(0)), trunc)
    t = (_mm_blocks(h2, _to_f16(c["w2"], trunc)) + c["b2"]).reshape(L, B, Q, 4)
    pb = t if mutant == "no_sigmoid" else np.float32(1) / (np.float32(1) + np.exp(-t, dtype=np.float32))
    lvl = 0 if mutant == "level_0" else L - 1
    lg = logits[lvl].reshape(B * Q, C1)
    if mutant == "padded_column" and C1 % 16:      # the loader's zero row behind the last logit takes part
        lg = np.concatenate([lg, np.zeros((B * Q, 1), np.float32)], 1)
    if mutant == "softmax_foreground_only":
        lg = lg[:, :C1 - 1]
    n_max = lg.shape[1] if mutant == "max_with_no_object" else C1 - 1
    m, s, labels = _softmax_rows(lg, n_max)
    if mutant == "tie_to_higher":
        labels = n_max - 1 - lg[:, :n_max][:, ::-1].argmax(-1)
    best = np.take_along_axis(lg, labels[:, None], 1)[:, 0]
    scores = np.exp(best - m, dtype=np.float32) / s
    sizes = c["sizes"].copy()
    if mutant == "hw_swapped":
        sizes = sizes[:, ::-1]
    if mutant == "scale_of_image_0":
        sizes[:] = sizes[0]
    pl = pb[lvl]
    if mutant == "full_width":
        pl = pl * np.array([1, 1, 2, 2], np.float32)
    return dict(logits=logits, h1=h1, h2=h2, t=t, pred_boxes=pb, scores=scores.reshape(B, Q), labels=labels.reshape(B, Q).astype(np.int64),
                boxes=_xyxy_scaled(pl, sizes.astype(np.float32)))


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound (inf where a finite value is missing or a zero bound is missed)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


def verdict(c, got, ref=None, bnd=None):
    """Everything a set of outputs `got` (logits, pred_boxes [L, B, Q, .], scores, labels [B, Q], boxes [B, Q, 4]) of case c is held to.
    -> (list of failures, {output: worst |err| / bound, 'ambiguous': fraction of rows})"""
    ref, bnd = ref or reference(c), bnd or bounds(c)
    fails, stats = [], {}
    for k in ("logits", "pred_boxes", "boxes"):
        stats[k] = worst_ratio(got[k], ref[k], bnd[k])
        if not stats[k] <= 1.0:
            fails.append(f"{k}: worst |err| / bound {stats[k]:.3g}")
    stats["ambiguous"], stats["scores"], lf = check_labels(ref, bnd, got["labels"], got["scores"])
    fails += lf
    if stats["ambiguous"] > MAX_AMBIGUOUS:
        fails.append(f"{stats['ambiguous']:.1%} of the rows are ambiguous")
    want = boxes_fp32(np.asarray(got["pred_boxes"])[-1], c["sizes"])
    if not np.array_equal(want.view(np.int32), np.ascontiguousarray(got["boxes"], np.float32).view(np.int32)):
        fails.append("boxes are not the fp32 restatement on the returned pred_boxes bit for bit")
    if c["family"] in EXACT_FAMILIES:
        m = model(c)
        if not np.array_equal(np.ascontiguousarray(got["logits"], np.float32).view(np.int32), m["logits"].view(np.int32)):
            fails.append("logits differ from the exact ones")
        if not np.array_equal(np.asarray(got["labels"]).astype(np.int64), m["labels"]):
            fails.append("labels differ from the exact ones")
        sig = 1 / (1 + np.exp(-m["t"].astype(np.float64)))
        stats["sigmoid"] = worst_ratio(got["pred_boxes"], sig, sigmoid_rounding(m["t"]))
        if not stats["sigmoid"] <= 1.0:
            fails.append(f"pred_boxes against sigma(exact t): worst |err| / rounding {stats['sigmoid']:.3g}")
    return fails, stats


def check_labels(ref, bnd, labels, scores):
    """The label rule.  -> (fraction of ambiguous rows, worst |score - p| / bound, list of failures)"""
    fg, E = ref["logits"][-1][..., :-1], bnd["logits"][-1][..., :-1]
    fg, E = fg.reshape(-1, fg.shape[-1]), E.reshape(-1, E.shape[-1])
    prob, Ep = ref["prob"].reshape(fg.shape[0], -1), bnd["prob"].reshape(fg.shape[0], -1)
    labels, scores = np.asarray(labels).reshape(-1), np.asarray(scores, np.float64).reshape(-1)
    want = ref["labels"].reshape(-1)
    rows = np.arange(fg.shape[0])
    top, Etop = fg[rows, want], E[rows, want]
    near = (top[:, None] - fg) < (Etop[:, None] + E)      # the classes within the two bounds of the maximum, and the maximum itself
    near[rows, want] = True
    ambiguous = near.sum(-1) > 1
    fails = []
    bad = (labels < 0) | (labels >= fg.shape[1])
    lab = np.where(bad, 0, labels)
    for r in np.nonzero(bad | ~near[rows, lab] | (~ambiguous & (labels != want)))[0][:5]:
        fails.append(f"row {r}: label {labels[r]}, reference {want[r]} ({'ambiguous' if ambiguous[r] else 'unambiguous'})")
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(scores - prob[rows, lab])
        ratio = np.where(err == 0, 0.0, np.where(np.isfinite(err), err, np.inf) / Ep[rows, lab])
    for r in np.nonzero(~(ratio <= 1))[0][:5]:
        fails.append(f"row {r}: score {scores[r]:.9g}, class {lab[r]} has probability {prob[r, lab[r]]:.9g} +- {Ep[r, lab[r]]:.3g}")
    return float(ambiguous.mean()), float(ratio.max()), fails
