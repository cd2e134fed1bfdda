"""What hg_hoi_head (hg_hoi_head.hip, hg_heads.hip) is held to.  A plain module beside the tests (tests/test_hoi_head_model.py,
tests/test_hoi_head_host.py, tests/test_gpu_hoi_head.py import it): no fixtures, no GPU, no library.  It builds on roi_bound (the
float64 definition of an aligned RoI, its coordinate error and its screen) and restates nothing of it.

RULE 1, bits.  `batch_pairs`, `axis_weights` and `pool` restate hoi_setup_kernel and hoi_pool_kernel in fp32, operation for operation:
    pairs        all (x, y), x < n_h, y != x, row-major; objects = labels[y]; union box = min of the low, max of the high corners
    one axis     s = b1 scale - .5; e = b2 scale - .5; r = e - s; bin = r / P; g = ceil(r / P)
                 for ph, i in order: y = (s + ph bin) + ((i + .5) bin) / g; skipped outside [-1, size]; clamped as roi_align_kernel does;
                 ly = y - yl; hy = 1 - ly;  w[yl] = w[yl] + hy, then w[yh] = w[yh] + ly;  support [min yl, max yh]
    contraction  acc = 0; for y in support, x in support: acc = acc + (wy[y] wx[x]) f[y][x];  mean = acc / (max(gy gx, 1) float(P P))
The integer outputs, the union boxes and every pooled mean of EVERY box are expected bit for bit; so are `head`'s logits (products
rounded one by one, summed left to right) and the priors at p = 1.

RULE 2, float64.  The reference is roi_bound.definition's mean.  In exact arithmetic the mean of the P x P bins is
wy^T F wx / (count P^2) with wy[j] = sum over the P gh samples of the tent at j: the kernel's form.  |got - want| <= E, u = 2^-24:
  coordinate   roi_bound's term unchanged: a sample moved by (d_y, d_x) changes the piecewise bilinear function by at most
               d_y SY + d_x SX; summed over the samples, / (count P^2):  E_coord
  rounding     ly is exact (Sterbenz), hy rounds once; an entry of wy receives at most 2 P gh additions of non-negative terms (two
               per sample where the clamp makes yl = yh): relative error gamma(2 P gh + 1); wx likewise; one rounding for wy wx, one
               for (.) f, S - 1 additions over the support of S taps, one rounding for count P^2 (none below 2^24), one for the
               division.  All factors multiply, gamma(a) + gamma(b) <= gamma(a + b):
                   E_round = gamma(2 P (gh + gw) + S + 6) (sum wy wx |f| / (count P^2) + E_coord)
               (the weights in that sum are the exact ones; the computed ones differ by the coordinate error, hence + E_coord)
  E = E_coord + E_round.  Discontinuities are roi_bound's (a sample on y = -1 or y = H, roi / P on an integer): `kept` is its screen,
  at most 5 % of the random boxes may be lost (asserted in tests/test_hoi_head_model.py; the seeded draws lose none).
  Against hg_roi_align's mean the two bounds add: |pool - roi_align| <= E + roi_bound's E_mean.

priors at p = 2.8.  The kernel raises the fp32 score to the fp32 power in DOUBLE and rounds the result once to fp32, so the bound comes
from the number formats and from no single-precision routine's accuracy: float64 pow of the same operands rounded to fp32 is within
half an fp32 ulp, and the device's double pow would have to be wrong by 2^28 of ITS ulps to use up the other half.  POWF_ULP = 1 ulp
(2^-23 |x|) of numpy's float64 pow; no measured value went into it.  score = sigmoid(l) ph po: `score_bound` propagates |d sigmoid| <= |d l| / 4 + 2 u and the three roundings.

Worst |err| / E of rule 2 over the kept boxes: the restatement on the CPU (tests/test_hoi_head_model.py, lines HOI_RATIO) and the
kernel on an MI355X (tests/test_gpu_hoi_head.py; its second figure is |pool - hg_roi_align| over E + roi_bound's E_mean):

    restatement   mixed_14x14 0.073   mixed_24x24 0.062   mixed_5x9 0.033   outlier_24x24 0.017   affine_14x14_p2 0.050   ints 0
    kernel        b3_one_box_between 0.047 / 0.020   b3_no_human_between 0.058 / 0.062   b2_24x24_c768 0.020 / 0.003   b1_435_pairs 0.047 / 0.020
                  b1_5x9_c4 0.024 / 0.007   b2_c257 0.056 / 0.020   b3_24x24_c4 0.062 / 0.004   b1_cuts 0.005 / 0.001
                  b1_26x26_c96 0.022 / 0.008   b2_32x32_c40 0.022 / 0.006
No entry is above 1 (the tests assert <= 1); no measured value is a threshold.  E is mostly its coordinate term, which takes the
steepest slope of twelve neighbouring cells for every sample: a sixteenth of it is used.  What E cannot see - a reordered sum, a
fused multiply-add - rule 1 does, and tests/test_hoi_head_host.py reads the kernels' assembly for fused operations.

Mutants (`MUTANTS`; tests/test_hoi_head_model.py proves each is rejected by a rule on the committed cases):
    no_half_pixel, count_no_max, no_clamp, cutoff_hm1            roi_bound's, on this form
    wy_wx_swapped      wy and wx exchanged                        last_row_dropped   the support ends one row early
    seam_skipped       the channel at a chunk seam (c = 64) left unwritten
    union_swapped      union box from max / min exchanged        pairs_col_major    pairs enumerated y-major
    diag_kept          y == x kept                                prior_from_x       prior columns from labels[x]
    scale_twice        a branch scale applied twice               sigmoid_first      sigmoid of every branch before the sum
"""
import functools

import numpy as np

import roi_bound as rb

U = rb.U
F = np.float32
POWF_ULP = 1.0
POOL_MUTANTS = ("no_half_pixel", "count_no_max", "no_clamp", "cutoff_hm1", "wy_wx_swapped", "last_row_dropped", "seam_skipped")
PAIR_MUTANTS = ("union_swapped", "pairs_col_major", "diag_kept")
HEAD_MUTANTS = ("prior_from_x", "scale_twice", "sigmoid_first")
MUTANTS = POOL_MUTANTS + PAIR_MUTANTS + HEAD_MUTANTS
MAX_GRID = 65536


# ---- rule 1: pairs ------------------------------------------------------------------------------------------------------------------
def pairs(n, n_h, mutant=None):
    """(x [p], y [p]) int32 of one image with humans first"""
    if n_h == 0 or n <= 1:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    xs, ys = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = xs < n_h if mutant == "diag_kept" else (xs != ys) & (xs < n_h)
    if mutant == "pairs_col_major":
        x, y = xs.T[keep.T], ys.T[keep.T]
    else:
        x, y = xs[keep], ys[keep]
    return x.astype(np.int32), y.astype(np.int32)


def union_of(bh, bo, mutant=None):
    lo, hi = (np.maximum, np.minimum) if mutant == "union_swapped" else (np.minimum, np.maximum)
    return np.concatenate([lo(bh[:, :2], bo[:, :2]), hi(bh[:, 2:], bo[:, 2:])], 1).astype(np.float32)


def batch_pairs(boxes, labels, box_off, n_human, mutant=None):
    """-> dict of the batch: pair_h, pair_o, objects (int32 [Pt]), union_boxes [Pt, 4], image [Pt], pair_off [B + 1]"""
    ph, po, ob, ub, im, off = [], [], [], [], [], [0]
    for b in range(len(n_human)):
        lo, hi = box_off[b], box_off[b + 1]
        x, y = pairs(hi - lo, n_human[b], mutant)
        ph.append(x), po.append(y), ob.append(labels[lo:hi][y].astype(np.int32)), im.append(np.full(len(x), b, np.int32))
        ub.append(union_of(boxes[lo:hi][x], boxes[lo:hi][y], mutant))
        off.append(off[-1] + len(x))
    return {"pair_h": np.concatenate(ph), "pair_o": np.concatenate(po), "objects": np.concatenate(ob),
            "union_boxes": np.concatenate(ub).reshape(-1, 4), "image": np.concatenate(im), "pair_off": np.asarray(off)}


# ---- rule 1: the separable weights and the contraction --------------------------------------------------------------------------------
def axis_weights(b1, b2, scale, P, size, mutant=None):
    """-> (w [32] float32, g float32 (NaN = refused), lo, hi) of one axis of one RoI"""
    b1, b2, scale, Pf = F(b1), F(b2), F(scale), F(P)
    off = F(0.0) if mutant == "no_half_pixel" else F(0.5)
    with np.errstate(all="ignore"):
        s1, e1 = b1 * scale - off, b2 * scale - off
        r = e1 - s1
        bn = r / Pf
        gf = np.ceil(r / Pf)
    w = np.zeros(32, np.float32)
    if not gf <= MAX_GRID:
        return w, F(np.nan), 0, -1
    g, lo, hi = int(gf), size, -1
    top = F(size - 1) if mutant == "cutoff_hm1" else F(size)
    for ph in range(P):
        for i in range(max(g, 0)):
            y = (s1 + F(ph) * bn) + ((F(i) + F(0.5)) * bn) / F(g)
            if y < F(-1.0) or y > top:
                continue
            if y <= 0:
                y = F(0.0)
            yl = int(y)
            if mutant == "no_clamp":
                yl = min(yl, size - 1)
                yh = yl + 1
            elif yl >= size - 1:
                yl = yh = size - 1
                y = F(yl)
            else:
                yh = yl + 1
            ly = F(y - F(yl))
            hy = F(1.0) - ly
            w[yl] = w[yl] + hy
            if yh < size:      # (`no_clamp`: the row behind the map reads 0)
                w[yh] = w[yh] + ly
            lo, hi = min(lo, yl), max(hi, min(yh, size - 1))
    if hi < 0:
        lo = 0
    return w, F(gf), lo, hi


def pool(feat, boxes, P, scale, mutant=None):
    """-> mean [n, C] float32 of hoi_setup_kernel + hoi_pool_kernel for the boxes (any RoIs) of ONE image, feat [C, H, W]"""
    assert mutant is None or mutant in POOL_MUTANTS, mutant
    feat = np.asarray(feat, np.float32)
    C, H, W = feat.shape
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    out = np.zeros((len(boxes), C), np.float32)
    with np.errstate(all="ignore"):
        for k, b in enumerate(boxes):
            wy, gy, ylo, yhi = axis_weights(b[1], b[3], scale, P, H, mutant)
            wx, gx, xlo, xhi = axis_weights(b[0], b[2], scale, P, W, mutant)
            if mutant == "wy_wx_swapped":
                m = max(H, W)
                wy, wx, ylo, yhi, xlo, xhi = wx, wy, min(xlo, H - 1), min(xhi, H - 1), min(ylo, W - 1), min(yhi, W - 1)
                assert m <= 32
            if mutant == "last_row_dropped":
                yhi -= 1
            acc = np.zeros(C, np.float32)
            for y in range(ylo, yhi + 1):
                for x in range(xlo, xhi + 1):
                    acc = acc + F(wy[y] * wx[x]) * feat[:, y, x]
            cnt = gy * gx
            if mutant != "count_no_max":
                cnt = F(1.0) if cnt < 1 else cnt
            out[k] = acc / (cnt * F(P * P))
            if mutant == "seam_skipped" and C > 64:
                out[k, 64] = 0.0
    return out


# ---- rule 2 -----------------------------------------------------------------------------------------------------------------------
def _touched(v, size):
    """support [lo, hi] of the samples v (exact coordinates) on an axis of `size` cells, as the kernel tracks it"""
    v = v[(v >= -1.0) & (v <= size)]
    if v.size == 0:
        return 0, -1
    yl = np.minimum(np.clip(v, 0.0, None).astype(np.int64), size - 1)
    return int(yl.min()), int(np.minimum(yl + 1, size - 1).max())


def reference(feat, boxes, P, scale, slopes=None):
    """-> dict: mean, E [n, C] float64, kept [n] (roi_bound's screen), roi_E [n, C] (roi_bound's own bound of hg_roi_align's mean)"""
    f = np.asarray(feat, np.float64)
    C, H, W = f.shape
    fa = np.abs(f)
    slopes = slopes if slopes is not None else rb._slopes(feat)
    SY, SX = slopes
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    d = rb.definition(feat, boxes, P, scale, slopes)
    E = np.zeros((len(boxes), C))
    for b, box in enumerate(boxes):
        y, d_y, _, _, gh = rb._coord_error(box[1], box[3], scale, P, H)
        x, d_x, _, _, gw = rb._coord_error(box[0], box[2], scale, P, W)
        if gh <= 0 or gw <= 0:
            continue
        den = float(gh * gw) * P * P
        yv, xv = y.reshape(-1), x.reshape(-1)
        Wy, Wx = rb._tents(yv, H).sum(0), rb._tents(xv, W).sum(0)
        A = np.einsum("h,chw,w->c", Wy, fa, Wx) / den
        iny, inx = (yv >= -1.0) & (yv <= H), (xv >= -1.0) & (xv <= W)
        yl = np.minimum(np.clip(yv, 0.0, H - 1.0).astype(np.int64), H - 1)
        xl = np.minimum(np.clip(xv, 0.0, W - 1.0).astype(np.int64), W - 1)
        sy = SY[:, yl[:, None], xl[None]] * (d_y.reshape(-1) * iny)[None, :, None] * inx[None, None, :]
        sx = SX[:, yl[:, None], xl[None]] * (d_x.reshape(-1) * inx)[None, None, :] * iny[None, :, None]
        e_coord = (sy + sx).sum((1, 2)) / den
        (ylo, yhi), (xlo, xhi) = _touched(yv, H), _touched(xv, W)
        S = max(yhi - ylo + 1, 0) * max(xhi - xlo + 1, 0)
        E[b] = e_coord + rb.gamma(2 * P * (gh + gw) + S + 6) * (A + e_coord)
    return {"mean": d["mean"], "E": E, "kept": d["kept"], "roi_E": d["E_mean"]}


def worst(got, ref, extra=None):
    """worst |got - mean| / (E [+ extra]) over the kept boxes"""
    return rb.worst(got, ref["mean"], ref["E"] if extra is None else ref["E"] + extra, ref["kept"])


# ---- the head behind the pooling: logits, priors, scores --------------------------------------------------------------------------------
def head(branches, scales, scores_x, scores_y, labels_x, labels_y, obj2target, p, mutant=None):
    """fp32 restatement of hoi_epilogue_kernel on branch logits [nb][Pt, NC] -> (logits, prior [2, Pt, NC], score); powf by float64"""
    assert mutant is None or mutant in HEAD_MUTANTS, mutant
    acc = None
    for br, sc in zip(branches, scales):
        t = np.asarray(br, np.float32) * F(sc)
        if mutant == "scale_twice" and acc is None:
            t = t * F(sc)
        if mutant == "sigmoid_first":
            t = (F(1.0) / (F(1.0) + np.exp(-t))).astype(np.float32)
        acc = t if acc is None else acc + t
    lab = labels_x if mutant == "prior_from_x" else labels_y
    on = np.asarray(obj2target)[lab] != 0
    sh, so = np.asarray(scores_x, np.float32), np.asarray(scores_y, np.float32)
    if p != 1.0:
        sh, so = np.power(sh.astype(np.float64), float(F(p))).astype(np.float32), np.power(so.astype(np.float64), float(F(p))).astype(np.float32)
    prior = np.stack([np.where(on, sh[:, None], F(0.0)), np.where(on, so[:, None], F(0.0))]).astype(np.float32)
    if acc is None:
        return None, prior, None
    sig = acc if mutant == "sigmoid_first" else (F(1.0) / (F(1.0) + np.exp(-acc))).astype(np.float32)
    return acc, prior, (sig * (prior[0] * prior[1])).astype(np.float32)


def prior_bound(prior64):
    """|powf - float64 pow| allowed: POWF_ULP ulp of the value (ulp of an fp32 x <= 2^-23 |x|)"""
    return POWF_ULP * 2.0 ** -23 * np.abs(prior64)


def score_bound(logits, prior64):
    """|score - sigmoid64(logits) ph po| from the RETURNED fp32 logits: expf within 2 ulp and the add and the division of the sigmoid
    (4 u relative in all, sigmoid <= 1), ph and po within prior_bound, two multiplies"""
    sig = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))
    ph, po = prior64
    rel = 8 * U + 2 * POWF_ULP * 2.0 ** -23 + 2 * U
    return sig * ph * po, rel * sig * ph * po * (1 + 1e-6) + 1e-45


# ---- the committed cases ----------------------------------------------------------------------------------------------------------
def sub_bin_boxes(size):
    """boxes smaller than one bin, and one of exactly one cell"""
    s = float(size)
    return rb._boxes([(0.3 * s, 0.4 * s, 0.3 * s + 3.0, 0.4 * s + 2.0), (0.7 * s, 0.1 * s, 0.7 * s + 0.5, 0.1 * s + 9.0), (16.0, 32.0, 32.0, 48.0)])


def beyond_boxes(size):
    """boxes reaching beyond the map by more than one cell on each side in turn, and the whole image"""
    s = float(size)
    return rb._boxes([(-40.0, 0.2 * s, 0.5 * s, 0.8 * s), (0.5 * s, -55.0, 0.9 * s, 0.6 * s), (0.4 * s, 0.3 * s, s + 47.0, 0.9 * s),
                      (0.1 * s, 0.5 * s, 0.6 * s, s + 60.0), (0.0, 0.0, s, s)])


@functools.lru_cache(maxsize=None)
def image_boxes(H, size, n, seed, families=True):
    """n boxes of one image: a seeded uniform draw, with a box of each other family among them when there is room (n >= 6; box 1 is
    the zero-width one)"""
    fam = np.zeros((0, 4), np.float32)
    if families and n >= 6:      # zero width, beyond the left edge, the whole image, smaller than a bin - the second one a human
        fam = np.concatenate([rb.degenerate_boxes(size)[:1], beyond_boxes(size)[[0, 4]], sub_bin_boxes(size)[:1]])
    rnd = rb.random_boxes(n - len(fam), size, seed)
    b = np.concatenate([rnd[:1], fam[:1], rnd[1:], fam[1:]]).astype(np.float32)
    b.setflags(write=False)
    return b


def make_batch(sizes, n_humans, H, W, C, size, seed, n_obj=12, num_classes=24, family="randn"):
    """a seeded batch: feat [B, C, H, W], boxes / scores / labels [N], box_off, n_human, obj2target - numpy, humans first (label 0)"""
    rng = np.random.RandomState(seed)
    B = len(sizes)
    feat = np.stack([rb.make_map(family, C, H, W) * F(1 + b) for b in range(B)]).astype(np.float32)
    box_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    boxes = np.concatenate([image_boxes(H, size, n, seed + 31 * b) for b, n in enumerate(sizes)] + [np.zeros((0, 4), np.float32)])
    scores = rng.uniform(0.05, 1.0, size=int(box_off[-1])).astype(np.float32)
    labels = np.concatenate([np.r_[np.zeros(h, np.int32), rng.randint(1, n_obj, size=n - h).astype(np.int32)] for n, h in zip(sizes, n_humans)]
                            + [np.zeros(0, np.int32)])
    o2t = (rng.uniform(size=(n_obj, num_classes)) < 0.3).astype(np.uint8)
    return {"feat": feat, "boxes": np.ascontiguousarray(boxes, np.float32), "scores": scores, "labels": labels, "box_off": box_off,
            "n_human": np.asarray(n_humans, np.int32), "obj2target": o2t, "H": H, "W": W, "C": C, "B": B, "num_classes": num_classes}
