"""What roi_align_kernel (hg_preproc.hip) is held to.  A plain module beside the tests (tests/test_roi_model.py,
tests/test_gpu_roi_exact.py import it): no fixtures, no GPU, no library.  Two references, two rules.

RULE 1, bits.  `restate()` is the fp32 restatement of the kernel in torchvision's published operation order (the arithmetic of
oracle/roi_oracle.py, vectorised over channels and bins; tests/test_roi_model.py proves the two bit-equal), with `out_mean` as the
kernel computes it: a sequential fp32 sum over the bins in (ph, pw) order divided by float(P * P).  Every pooled element and every mean
of EVERY box - those placed on the discontinuities included - is expected bit for bit.

RULE 2, float64 against the definition.  `definition()` does not follow the kernel: aligned = True, bin grid ceil(roi / P), and the
bilinear sample with the boundary rule written as a tent function - a sample at y is worth sum_j max(0, 1 - |clip(y, 0, H - 1) - j|)
f[j] (nothing outside [-1, H]) - so that a bin is (Ay f Ax^T) / count with two small matrices of summed tents.  float64 throughout, from
the fp32 box and the fp32 spatial_scale as exact numbers.  Every pooled element and mean has |got - want| <= E, u = 2^-24:

  rounding   A sample's value is sum of 4 terms (w f): ly = y - yl is exact (Sterbenz), hy = 1 - ly rounds once, a weight hy * hx
             carries 3 roundings, the product with f a 4th, the three additions of the four-term sum at most 3 more; the bin's
             sequential sum over G = gh gw samples adds at most G more to a term, the division by count one:
                 E_round = gamma(G + 8) sum |w f| / count,      gamma(n) = n u / (1 - n u)
  coordinate y = fl(fl(sh + fl(ph bh)) + fl(fl(fl(iy + .5) bh) / gh)) with sh = fl(fl(b s) - .5), rh = fl(eh - sh), bh = fl(rh / P).
             `_coord_error` propagates u |result| per operation through exactly this expression (a few operations on values up to
             about H: d_y of order 1e-5 on a 24-row map).  The sampled function is continuous and piecewise bilinear, so a sample
             moved by (d_y, d_x) changes by at most d_y SY + d_x SX, SY (SX) the largest |f[j + 1, k] - f[j, k]| (|f[j, k + 1] - f[j, k]|)
             over the sample's cell and its neighbours (rows yl - 1 .. yl + 1, columns xl - 1 .. xl + 2: the moved sample may sit
             in the next cell, and the slope along y is itself interpolated along x).  That is the four corners' slope of the cell,
             widened to be a proof:
                 E_coord = sum over the bin's samples (d_y SY + d_x SX) / count
  mean       sum_bins E / P^2 + gamma(P^2) sum_bins |pooled| / P^2        (P^2 - 1 additions and one division)

  Discontinuities.  The operation jumps where a sample crosses y = -1, y = H, x = -1, x = W and where roi / P crosses an integer (the
  grid count).  `definition` keeps a box for rule 2 (`kept`) only if every sample is further from those four lines than its own d_y (d_x) and
  roi / P is further from an integer than the propagated error of bh (bw): then the fp32 kernel and the exact arithmetic take the same
  branch everywhere.  The margin IS the coordinate error, nothing added.  At most 5 % of the random boxes may be screened out
  (asserted; the seeded draws lose none).

Families (`make_map`): randn; affine (rows of a x + b y + c: the float64 result is the closed form at the bin centre for boxes whose
samples stay inside the map - asserted in tests/test_roi_model.py); ints (integers in [-8, 8] with boxes on a dyadic grid, P in {1, 2}
and grid counts that are powers of two - every weight, product and partial sum is exact in fp32, asserted by `exactness`, and the
float64 result rounded once is expected bit for bit); outlier (randn with one cell of 1e4).

Mutants (`MUTANTS`), each rejected by at least one rule on the committed cases (tests/test_roi_model.py):
    no_half_pixel     no - 0.5 offset                         fixed_grid        2 x 2 samples per bin whatever the box
    count_no_max      count without max(.., 1)                cutoff_hm1        y > H - 1 (x > W - 1) as the cut-off
    no_clamp          the clamp yl >= H - 1 missing (the row behind the map reads 0)
    weights_swapped   hy * lx and ly * hx exchanged           channels_256      the channel loop stops at 256
    mean_pw_ph        the mean walks the bins (pw, ph)        pairwise_mean     numpy's pairwise mean
    fma_sum           the four-term sum contracted to fused multiply-adds
  pairwise_mean and fma_sum pass rule 2 and fail rule 1 only: they are correct arithmetic in another order.

Worst |err| / E of rule 2 over the kept boxes: the restatement on the CPU (tests/test_roi_model.py, lines ROI_RATIO) and the kernel on
an MI355X (tests/test_gpu_roi_exact.py) print the same figures, since the kernel is the restatement bit for bit:

    case               map           C     P   scale  boxes kept   pooled   mean
    vitl_24x24_1024    24 x 24    1024     7   1/14    44 of 45    0.256    0.063
    vitb_14x14_768     14 x 14     768     7   1/16    15 of 16    0.159    0.051
    c257_p14           14 x 14     257    14   1/16    11 of 12    0.217    0.023
    c256_p2            24 x 24     256     2   1/14    10 of 12    0.067    0.042
    c255_p1             5 x 9      255     1   1/16    11 of 12    0.052    0.051
    c4_5x9_p7           5 x 9        4     7   1/14    44 of 45    0.172    0.041
    outlier_24x24      24 x 24       4     7   1/14    44 of 45    0.199    0.022
    affine_14x14       14 x 14       4     7   1/16    24 of 25    0.184    0.070
    affine_5x9_p2       5 x 9        4     2   1/14    22 of 22    0.132    0.071
    one_box            14 x 14     257     7   1/16     1 of 1     0.096    0.008
    ints_p2 / ints_p1  exact                                       0        0

No random box is screened out; the boxes lost are the zero-width box (roi / P = 0 is an integer) and, at P = 2 on the 24 x 24 map, the huge
box (54 cells wide: 27 a bin).  No entry is above 1 (the tests assert <= 1); no measured value is a threshold.  E is a worst
case over 8 + G roundings that in fact add like a random walk, and its coordinate term takes the steepest slope of twelve neighbouring
cells: a quarter of it is used at most.  What E cannot see - a reordered sum, a fused multiply-add - rule 1 does: BEFORE
hg_preproc.hip was compiled with -ffp-contract=off these same ratios read 0.24 / 0.06 on the 24 x 24 x 1024 map while one pooled value
in six (380 617 of 2 257 920) was not the restatement's bits - the backend had fused b * scale - 0.5 and sh + ph * bh whatever the
kernel's `fp contract(off)` pragma said.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
F = np.float32
MUTANTS = ("no_half_pixel", "fixed_grid", "count_no_max", "cutoff_hm1", "no_clamp", "weights_swapped", "channels_256", "mean_pw_ph",
           "pairwise_mean", "fma_sum")
BITS_ONLY = ("pairwise_mean", "fma_sum")
FAMILIES = ("randn", "affine", "ints", "outlier")
SCALES = {"1/16": F(1.0 / 16.0), "1/14": F(1.0 / 14.0)}


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_map(family, C, H, W):
    rng = np.random.RandomState(1000 * FAMILIES.index(family) + 97 * C + 7 * H + W)
    if family == "affine":
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        co = affine_coeffs(C, H, W)
        f = (co[:, 0, None, None] * xx + co[:, 1, None, None] * yy + co[:, 2, None, None]).astype(np.float32)
        f.setflags(write=False)
        return f
    if family == "ints":
        f = rng.randint(-8, 9, size=(C, H, W)).astype(np.float32)
    else:
        f = rng.randn(C, H, W).astype(np.float32)
        if family == "outlier":
            f[:, H // 2, W // 3] = 1e4
    f.setflags(write=False)
    return f


def affine_coeffs(C, H, W):
    """[C, 3] (a, b, c) of the rows a x + b y + c of the affine family: quarters, exact in fp32 on the pixel grid"""
    rng = np.random.RandomState(1000 * FAMILIES.index("affine") + 97 * C + 7 * H + W)
    return rng.randint(-8, 9, size=(C, 3)) / 4.0


def random_boxes(n, size, seed):
    """n uniform boxes in [-40, size + 44] (x1 < x2, y1 < y2) on an image of `size` pixels"""
    rng = np.random.RandomState(seed)
    b = np.sort(rng.uniform(-40.0, size + 44.0, size=(n, 2, 2)), axis=2)          # [box, (x, y), (low, high)]
    return np.ascontiguousarray(np.stack([b[:, 0, 0], b[:, 1, 0], b[:, 0, 1], b[:, 1, 1]], 1).astype(np.float32))


def _boxes(rows):
    return np.asarray(rows, np.float32).reshape(-1, 4)


def degenerate_boxes(size):
    s = float(size)
    return _boxes([(50, 60, 50, 120),                    # zero width: no samples, count 1 -> 0
                   (120, 60, 50, 120),                   # x2 < x1
                   (s + 100, s + 100, s + 200, s + 200), (-300, -300, -100, -50),      # wholly outside the map
                   (-0.6 * s, -0.6 * s, 1.65 * s, 1.65 * s)])  # one huge box: 2.25 maps wide, a grid of 8 x 8 per bin at P = 7


def on_the_cuts(H, P, scale):
    """boxes placed on the discontinuities (scale a power of two, so that the coordinates are exact): the first sample row exactly at
    y = -1; the last exactly at y = H; rh / P exactly 1, 2 and 3"""
    inv = 1.0 / float(scale)
    out = []
    # one sample per bin (rh = P): samples at sh + ph + 0.5;  sh = -1.5 puts the first at -1, sh = H - P + 0.5 the last at H
    for sh in (-1.5, H - P + 0.5):
        out.append((2 * inv, (sh + 0.5) * inv, (2 + P + 0.5) * inv + 0.5 * inv, (sh + 0.5 + P) * inv))
    for k in (1, 2, 3):
        out.append((1 * inv, 1 * inv, (1 + k * P) * inv, (1 + k * P) * inv))
    return _boxes(out)


def dyadic_boxes(scale, P):
    """boxes for the `ints` family at spatial_scale 1/16: corners on multiples of 2 pixels (1/8 of a cell), roi sizes whose grid counts
    ceil(roi / P) are 1, 2 or 4"""
    assert float(scale) == 1.0 / 16.0 and P in (1, 2)
    out = []
    for x1, y1, rw, rh in ((8, 8, 1.0, 2.0), (22, 10, 0.5, 1.0), (34, 6, 2.0, 4.0), (-30, 18, 4.0, 3.5), (50, -26, 3.75, 1.75), (100, 130, 8.0, 7.5),
                           (180, 170, 4.0, 8.0), (6, 200, 1.5, 0.25)):
        rw, rh = rw * P / 2.0, rh * P / 2.0
        out.append((x1, y1, x1 + 16.0 * rw, y1 + 16.0 * rh))
    return _boxes(out)


# ---- rule 1: the fp32 restatement of the kernel -----------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def restate(feat, boxes, P, scale, mutant=None, want_mean=True):
    """-> (pooled [n, C, P, P] float32, mean [n, C] float32) in the kernel's operation order"""
    assert mutant is None or mutant in MUTANTS, mutant
    feat = np.asarray(feat, np.float32)
    C, H, W = feat.shape
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = boxes.shape[0]
    scale, Pf = F(scale), F(P)
    off = F(0.0) if mutant == "no_half_pixel" else F(0.5)
    pooled = np.zeros((n, C, P, P), np.float32)
    mean = np.zeros((n, C), np.float32)
    Cr = min(C, 256) if mutant == "channels_256" else C
    fz = np.zeros((C, H + 1, W + 1), np.float32)          # a row / column of zeros behind the map, read by `no_clamp` only
    fz[:, :H, :W] = feat
    hi_y, hi_x = (F(H - 1), F(W - 1)) if mutant == "cutoff_hm1" else (F(H), F(W))
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(n):
            sw, sh = boxes[b, 0] * scale - off, boxes[b, 1] * scale - off
            ew, eh = boxes[b, 2] * scale - off, boxes[b, 3] * scale - off
            rw, rh = ew - sw, eh - sh
            bh, bw = rh / Pf, rw / Pf
            gh, gw = int(np.ceil(rh / Pf)), int(np.ceil(rw / Pf))
            if mutant == "fixed_grid":
                gh = gw = 2
            count = F(gh * gw) if mutant == "count_no_max" else F(max(gh * gw, 1))
            pidx = np.arange(P, dtype=np.float32)
            acc = np.zeros((Cr, P, P), np.float32)
            for iy in range(max(gh, 0)):
                y = (sh + pidx * bh) + ((F(iy) + F(0.5)) * bh) / F(gh)                      # [P]
                oky = ~((y < F(-1.0)) | (y > hi_y))
                yy = np.where(y <= 0, F(0.0), y).astype(np.float32)
                yl = np.where(oky, yy, 0).astype(np.int64)
                if mutant == "no_clamp":
                    yl = np.minimum(yl, H - 1)
                    yh = yl + 1
                else:
                    top = yl >= H - 1
                    yl = np.where(top, H - 1, yl)
                    yh = np.where(top, H - 1, yl + 1)
                    yy = np.where(top, yl.astype(np.float32), yy)
                ly = (yy - yl.astype(np.float32)).astype(np.float32)
                hy = F(1.0) - ly
                for ix in range(max(gw, 0)):
                    x = (sw + pidx * bw) + ((F(ix) + F(0.5)) * bw) / F(gw)
                    okx = ~((x < F(-1.0)) | (x > hi_x))
                    xx = np.where(x <= 0, F(0.0), x).astype(np.float32)
                    xl = np.where(okx, xx, 0).astype(np.int64)
                    if mutant == "no_clamp":
                        xl = np.minimum(xl, W - 1)
                        xh = xl + 1
                    else:
                        right = xl >= W - 1
                        xl = np.where(right, W - 1, xl)
                        xh = np.where(right, W - 1, xl + 1)
                        xx = np.where(right, xl.astype(np.float32), xx)
                    lx = (xx - xl.astype(np.float32)).astype(np.float32)
                    hx = F(1.0) - lx
                    w1, w2, w3, w4 = hy[:, None] * hx[None], hy[:, None] * lx[None], ly[:, None] * hx[None], ly[:, None] * lx[None]
                    if mutant == "weights_swapped":
                        w2, w3 = w3, w2
                    f1, f2 = fz[:Cr, yl[:, None], xl[None]], fz[:Cr, yl[:, None], xh[None]]
                    f3, f4 = fz[:Cr, yh[:, None], xl[None]], fz[:Cr, yh[:, None], xh[None]]
                    if mutant == "fma_sum":
                        t = _fma(np.broadcast_to(w4, f4.shape), f4, _fma(np.broadcast_to(w3, f3.shape), f3,
                                 _fma(np.broadcast_to(w2, f2.shape), f2, w1 * f1)))
                    else:
                        t = w1 * f1 + w2 * f2 + w3 * f3 + w4 * f4
                    acc = acc + np.where((oky[:, None] & okx[None])[None], t, F(0.0))
            acc = acc / count
            pooled[b, :Cr] = acc
            if want_mean:
                if mutant == "pairwise_mean":
                    mean[b, :Cr] = acc.reshape(Cr, -1).mean(-1, dtype=np.float32)
                else:
                    total = np.zeros(Cr, np.float32)
                    walk = acc.transpose(0, 2, 1) if mutant == "mean_pw_ph" else acc
                    for i in range(P * P):
                        total = total + walk.reshape(Cr, -1)[:, i]
                    mean[b, :Cr] = total / F(P * P)
    return pooled, mean


# ---- rule 2: float64 from the definition, and the bound ---------------------------------------------------------------------------
def _coord_error(b1, b2, scale, P, H):
    """one axis of one box: the exact sample coordinates [P, g] and the propagated fp32 error bound d [P, g] of the kernel's
    expression; the exact roi / P, its error, and g.  u |result| per fp32 operation, results taken at their exact values plus the
    error carried so far."""
    b1, b2, s = float(b1), float(b2), float(scale)

    def start(b):
        p = b * s                                   # fl(b s): u |p|
        e = U * abs(p)
        v = p - 0.5
        return v, e + U * (abs(v) + e)              # fl(. - .5)

    sh, d_sh = start(b1)
    eh, d_eh = start(b2)
    rh = eh - sh
    d_rh = d_sh + d_eh + U * (abs(rh) + d_sh + d_eh)
    bh = rh / P
    d_bh = d_rh / P + U * (abs(bh) + d_rh / P)
    g = int(math.ceil(bh))
    if g <= 0:
        return np.zeros((P, 0)), np.zeros((P, 0)), bh, d_bh, g
    ph = np.arange(P, dtype=np.float64)[:, None]
    iy = np.arange(g, dtype=np.float64)[None]
    t1 = ph * bh
    d_t1 = ph * d_bh + U * (np.abs(t1) + ph * d_bh)
    s1 = sh + t1
    d_s1 = d_sh + d_t1 + U * (np.abs(s1) + d_sh + d_t1)
    t2 = (iy + 0.5) * bh
    d_t2 = (iy + 0.5) * d_bh + U * (np.abs(t2) + (iy + 0.5) * d_bh)
    t3 = t2 / g
    d_t3 = d_t2 / g + U * (np.abs(t3) + d_t2 / g)
    y = s1 + t3
    d_y = d_s1 + d_t3 + U * (np.abs(y) + d_s1 + d_t3)
    return y + np.zeros((P, g)), d_y + np.zeros((P, g)), bh, d_bh, g


def _tents(y, size):
    """[len(y), size] float64: row i is the tent of sample y_i over the indices 0 .. size - 1 (zero outside [-1, size])"""
    inside = (y >= -1.0) & (y <= size)
    yc = np.clip(y, 0.0, size - 1.0)
    t = np.maximum(0.0, 1.0 - np.abs(yc[:, None] - np.arange(size)[None]))
    return t * inside[:, None]


def _slopes(feat):
    """SY, SX [C, H, W]: at cell (yl, xl) the largest |difference along y| (along x) over rows yl - 1 .. yl + 1 and columns
    xl - 1 .. xl + 2 (rows yl - 1 .. yl + 2 and columns xl - 1 .. xl + 1)"""
    f = np.asarray(feat, np.float64)
    C, H, W = f.shape

    def widen(d, lo_r, hi_r, lo_c, hi_c):
        out = np.zeros((C, H, W))
        p = np.zeros((C, H + 6, W + 6))
        p[:, 3:3 + d.shape[1], 3:3 + d.shape[2]] = d
        for dr in range(lo_r, hi_r + 1):
            for dc in range(lo_c, hi_c + 1):
                out = np.maximum(out, p[:, 3 + dr:3 + dr + H, 3 + dc:3 + dc + W])
        return out

    dy = np.abs(f[:, 1:] - f[:, :-1]) if H > 1 else np.zeros((C, 0, W))
    dx = np.abs(f[:, :, 1:] - f[:, :, :-1]) if W > 1 else np.zeros((C, H, 0))
    return widen(dy, -1, 1, -1, 2), widen(dx, -1, 2, -1, 1)


def definition(feat, boxes, P, scale, slopes=None):
    """-> dict: pooled, E [n, C, P, P], mean, E_mean [n, C] (float64), kept [n] bool (`screen`: rule 2 applies)"""
    f = np.asarray(feat, np.float64)
    C, H, W = f.shape
    fa = np.abs(f)
    SY, SX = slopes if slopes is not None else _slopes(feat)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    n = boxes.shape[0]
    pooled, E = np.zeros((n, C, P, P)), np.zeros((n, C, P, P))
    kept = np.ones(n, bool)
    for b in range(n):
        y, d_y, bh, d_bh, gh = _coord_error(boxes[b, 1], boxes[b, 3], scale, P, H)
        x, d_x, bw, d_bw, gw = _coord_error(boxes[b, 0], boxes[b, 2], scale, P, W)
        for r, d in ((bh, d_bh), (bw, d_bw)):
            if abs(r - round(r)) <= d:
                kept[b] = False
        if gh <= 0 or gw <= 0:
            continue
        if (np.minimum(np.abs(y + 1.0), np.abs(y - H)) <= d_y).any() or (np.minimum(np.abs(x + 1.0), np.abs(x - W)) <= d_x).any():
            kept[b] = False
        count = float(gh * gw)
        ty, tx = _tents(y.reshape(-1), H), _tents(x.reshape(-1), W)                       # [P gh, H], [P gw, W]
        Ay, Ax = ty.reshape(P, gh, H).sum(1), tx.reshape(P, gw, W).sum(1)
        pooled[b] = np.einsum("ph,chw,qw->cpq", Ay, f, Ax) / count
        e_round = gamma(gh * gw + 8) * np.einsum("ph,chw,qw->cpq", Ay, fa, Ax) / count
        yv, xv = y.reshape(-1), x.reshape(-1)
        iny, inx = (yv >= -1.0) & (yv <= H), (xv >= -1.0) & (xv <= W)
        yl = np.minimum(np.clip(yv, 0.0, H - 1.0).astype(np.int64), H - 1)
        xl = np.minimum(np.clip(xv, 0.0, W - 1.0).astype(np.int64), W - 1)
        sy = SY[:, yl[:, None], xl[None]] * (d_y.reshape(-1) * iny)[None, :, None] * inx[None, None, :]
        sx = SX[:, yl[:, None], xl[None]] * (d_x.reshape(-1) * inx)[None, None, :] * iny[None, :, None]
        e_coord = (sy + sx).reshape(C, P, gh, P, gw).sum((2, 4)) / count
        E[b] = e_round + e_coord
    mean = pooled.reshape(n, C, -1).mean(-1)
    E_mean = E.reshape(n, C, -1).sum(-1) / (P * P) + gamma(P * P) * np.abs(pooled).reshape(n, C, -1).sum(-1) / (P * P)
    return {"pooled": pooled, "E": E, "mean": mean, "E_mean": E_mean, "kept": kept}


def worst(got, want, E, kept):
    """worst |err| / E over the kept boxes (0 / 0 counts as 0)"""
    got = np.asarray(got, np.float64)[kept]
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want[kept])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / E[kept])
    return float(r.max())


def ratios(ref, pooled=None, mean=None):
    r = {}
    if pooled is not None:
        r["pooled"] = worst(pooled, ref["pooled"], ref["E"], ref["kept"])
    if mean is not None:
        r["mean"] = worst(mean, ref["mean"], ref["E_mean"], ref["kept"])
    return r


def exactness(feat, boxes, P, scale):
    """the `ints` family's precondition: box corners times the scale on a grid of 2^-3, grid counts powers of two up to 4 - sample
    coordinates then sit on a grid of 2^-6, weights on 2^-12; integer |f| <= 8 and at most 16 samples keep every partial sum below 2^24
    units of 2^-12, and count and P^2 are powers of two.  Raises AssertionError otherwise."""
    assert float(scale) == 1.0 / 16.0 and P in (1, 2)
    f = np.asarray(feat)
    assert (f == np.round(f)).all() and np.abs(f).max() <= 8
    for b in np.asarray(boxes, np.float64).reshape(-1, 4):
        c = b * float(scale)
        assert (c * 8 == np.round(c * 8)).all(), b
        for r in ((c[2] - c[0]) / P, (c[3] - c[1]) / P):
            g = math.ceil(r)
            assert g in (1, 2, 4) and (r * 8 == round(r * 8)), (b, r)
            assert ((np.arange(g) + 0.5) * r / g * 64 % 1 == 0).all(), (b, r)
    assert 16 * 8 * 2 ** 12 < 2 ** 24


# ---- the committed cases ------------------------------------------------------------------------------------------------------------
def _case(name, family, C, H, W, P, scale, boxes, rule2=True, n_random=0):
    """n_random: the leading boxes that are a seeded uniform draw (of which `definition` may screen out 5 %)"""
    return {"name": name, "n_random": n_random, "family": family, "C": C, "H": H, "W": W, "P": P, "scale": SCALES[scale], "boxes": boxes, "rule2": rule2}


def _mixed(H, size, n, seed):
    return np.concatenate([random_boxes(n, size, seed), degenerate_boxes(size)])


CASES = [
    _case("vitl_24x24_1024", "randn", 1024, 24, 24, 7, "1/14", _mixed(24, 336, 40, 11), n_random=40),                 # n = 45: the local map of ViT-L/14@336px
    _case("vitb_14x14_768", "randn", 768, 14, 14, 7, "1/16", _mixed(14, 224, 11, 12), n_random=11),
    _case("c257_p14", "randn", 257, 14, 14, 14, "1/16", _mixed(14, 224, 7, 13), n_random=7),
    _case("c256_p2", "randn", 256, 24, 24, 2, "1/14", _mixed(24, 336, 7, 14), n_random=7),
    _case("c255_p1", "randn", 255, 5, 9, 1, "1/16", _mixed(5, 112, 7, 15), n_random=7),
    _case("c4_5x9_p7", "randn", 4, 5, 9, 7, "1/14", _mixed(5, 100, 40, 16), n_random=40),
    _case("outlier_24x24", "outlier", 4, 24, 24, 7, "1/14", _mixed(24, 336, 40, 17), n_random=40),
    _case("affine_14x14", "affine", 4, 14, 14, 7, "1/16", _mixed(14, 224, 20, 18), n_random=20),
    _case("affine_5x9_p2", "affine", 4, 5, 9, 2, "1/14", np.concatenate([random_boxes(20, 100, 19), _boxes([(20, 15, 100, 50), (30.5, 22.25, 60, 49)])]), n_random=20),
    _case("one_box", "randn", 257, 14, 14, 7, "1/16", _boxes([(30.5, 20.25, 180.0, 200.75)])),
    _case("cuts_14x14_p7", "randn", 4, 14, 14, 7, "1/16", on_the_cuts(14, 7, SCALES["1/16"]), rule2=False),
    _case("cuts_24x24_p2", "randn", 257, 24, 24, 2, "1/16", on_the_cuts(24, 2, SCALES["1/16"]), rule2=False),
    _case("ints_p2", "ints", 257, 14, 14, 2, "1/16", dyadic_boxes(SCALES["1/16"], 2)),
    _case("ints_p1", "ints", 4, 24, 24, 1, "1/16", dyadic_boxes(SCALES["1/16"], 1)),
]
BY_NAME = {c["name"]: c for c in CASES}


def feat_of(c):
    return make_map(c["family"], c["C"], c["H"], c["W"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(pooled, mean) float32 of the restatement.  Cached: leave unchanged."""
    c = BY_NAME[name]
    p, m = restate(feat_of(c), c["boxes"], c["P"], c["scale"])
    p.setflags(write=False)
    m.setflags(write=False)
    return p, m


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    return definition(feat_of(c), c["boxes"], c["P"], c["scale"])
