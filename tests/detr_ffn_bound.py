"""What the DETR decoder's FFN (hg_detr_ffn.hip: the split over d_ff; or the two GEMMs) and the layer tail behind it (detr_dec_tail_kernel in
hg_detr_rows.hip) are held to: y = LayerNorm3(x + linear2(relu(linear1(x)))) and out = LayerNorm_final(y) in float64 on the CPU from the
operands the kernel multiplies (x rounded to fp16 for linear1, x itself in the residual; weights are fp16 numbers), and a bound PER
ELEMENT made of the worst case of each rounding the kernel performs.  A plain module beside the tests: no fixtures, no GPU, no library.

All float64, u = 2^-24, slices of 128 hidden units, n_sl = d_ff / 128.

  hidden unit    a = sum_k x16_k W1_uk + b1_u,  S1 = sum_k |x16_k| |W1_uk|,  h = relu(a)
                 e1 = D 2^-23 S1 + u (S1 + |b1|)    fp32 accumulation of D exact products in any order (2^-23, not u: no assumption on how the
                                                    matrix unit rounds its internal adds), and the bias add
                 t = h + e1;  e16 = 2^-11 t (2^-25 absolute where t < 2^-14)      ONE rounding to fp16 after the bias and the ReLU
                 e_h = e1 + e16, and 0 where a < -e1 (the ReLU gives an exact zero either way)
  pre-norm sum   s = x + b2 + sum_u h_u W2_nu,  S2 = sum_u (h_u + e_h,u) |W2_nu|
                 E_s = sum_u e_h,u |W2_nu|                    the hidden value's error times |W2|
                     + 128 2^-23 S2                           fp32 accumulation of each slice's 128 products, summed over the slices
                     + (n_sl + 2) u (|x| + |b2| + S2)         the n_sl + 1 additions of the slice sum ((x + b2) + p_0) + p_1 + ...
                 The two-GEMM path (option detr_ffn = 1; `bounds(c, split=False)`) sums all d_ff products in one K loop and adds the bias and
                 the residual in its epilogue: d_ff 2^-23 S2 + 3 u (|x| + |b2| + S2) instead of the last two lines.
  LayerNorm      with d = s - mean(s), sigma = sqrt(mean(d^2) + 1e-5):  Ed = E + mean(E) + 12 u mean|s| (the row mean moves by at most mean(E);
                 its own fp32 sum is ten additions deep: 3 in a lane, 6 in the butterfly, the division), q = sqrt(mean(Ed^2)): the
                 row's standard deviation moves by at most q, so
                 E_y = |g| (Ed / (sigma - q) + |d| q / (sigma (sigma - q)))  +  20 u |g| |d| / sigma  +  2 u |y|
                 (the second group: the fp32 variance sum, division, add, sqrt and reciprocal - at most 20 roundings of positive terms -, the
                 subtraction, the multiply and the fma).  q >= sigma / 2 makes the bound infinite (no family comes near).
  out            the same propagation of E_y through the final norm.

Rule: every element has |got - want| <= bound.  The families whose operands make every product and partial sum exact in fp32 (`exact`,
`trunc`) have E_s = 0 for the fp32 terms by construction and are compared BIT FOR BIT with `model()` instead - partial sums, stream and out.

`model()` restates the kernels' arithmetic: x16 = fp16(x); phase 1 accumulates fp32 over k in ascending blocks of 32 from zero, adds b1,
applies the ReLU, rounds once to fp16 (nearest even); phase 2 accumulates each slice's 128 units in four ascending blocks of 32 from zero
into partial[slice]; the tail adds ((x + b2) + partial[0]) + partial[1] + ... in ascending slice order, then the LayerNorm as the wave
computes it (lane i holds columns 4 i .. 4 i + 3 and 256 + 4 i ..; (v0 + v1) + (v2 + v3) per piece, the xor butterfly 32, 16, .. 1;
fma chains for the squares; 1 / sqrt(. / D + 1e-5); fma((v - mean) rstd, g, b)), and the final norm the same way without writing it back.

Families (`make_case`; seeded, weights always fp16 numbers):
    exact      x integers / 4 in [-1, 1], W1 and W2 integers / 2 in [-1, 1], biases integers / 8: every product and partial sum is exact in
               fp32 in any order (|s| < 2^19 in units of 2^-4), the hidden value is the exact sum rounded once
    trunc      hidden values 1 + (j + 3/4) 2^-10 exactly (x = e_0 + 3 2^-12 e_1, W1[u] = (1 + j 2^-10, 1, 0 ..)), W2 >= 0 on every 16th
               column: a truncating conversion is 3/4 ulp off in the same direction in every unit, rounding to nearest 1/4
    randn      x ~ randn, W ~ Xavier-uniform, biases 0.1 randn
    outlier    randn with every 37th column of x times 40 and every 29th row of W1 times 8
    cancel     W2 of opposite signs on the unit pairs (u, u + F / 2) with equal W1 rows there, plus 2^-6 randn: |sum| << S2
    subn       randn x times 2^-9 and W1 times 2^-4, b1 = -2^-20: hidden values around and below fp16's smallest normal, half of them negative
"""
import numpy as np

U = 2.0 ** -24
SLICE, ROWS = 128, 32
FAMILIES = ("exact", "trunc", "randn", "outlier", "cancel", "subn")
EXACT_FAMILIES = ("exact", "trunc")
MUTANTS = ("drop_slice", "double_slice", "b1_wrong_slice", "b2_per_slice", "no_relu", "relu_after_flush", "truncate_f16", "tail_rows_neighbour",
           "norms_swapped", "final_norm_written_back")


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def make_case(family, M, D, F, seed):
    r = np.random.default_rng([seed, M, D, F, FAMILIES.index(family)])
    n = lambda *s: r.standard_normal(s)
    xav = lambda o, i: (r.uniform(-1, 1, (o, i)) * np.sqrt(6.0 / (o + i)))
    if family == "exact":
        x, w1, w2 = r.integers(-4, 5, (M, D)) / 4, r.integers(-2, 3, (F, D)) / 2, r.integers(-2, 3, (D, F)) / 2
        b1, b2 = r.integers(-8, 9, F) / 8, r.integers(-8, 9, D) / 8
    elif family == "trunc":
        x = np.zeros((M, D))
        x[:, 0], x[:, 1] = 1.0, 3 * 2.0 ** -12
        w1 = np.zeros((F, D))
        w1[:, 0], w1[:, 1] = 1 + r.integers(0, 64, F) * 2.0 ** -10, 1.0
        w2 = np.zeros((D, F))
        w2[::16] = r.integers(1, 9, (D // 16, F)) / 8
        b1, b2 = np.zeros(F), np.zeros(D)
    else:
        x, w1, w2, b1, b2 = n(M, D), xav(F, D), xav(D, F), 0.1 * n(F), 0.1 * n(D)
        if family == "outlier":
            x[:, ::37] *= 40
            w1[::29] *= 8
        elif family == "cancel":
            w1[F // 2:] = w1[:F // 2]
            b1[F // 2:] = b1[:F // 2]
            w2[:, F // 2:] = -w2[:, :F // 2] + 2.0 ** -6 * xav(D, F // 2)
        elif family == "subn":
            x, w1, b1 = x * 2.0 ** -9, w1 * 2.0 ** -4, np.full(F, -(2.0 ** -20))
    g3, gf = 1 + 0.2 * n(D), 1 + 0.2 * n(D)
    be3, bef = 0.1 * n(D), 0.1 * n(D)
    c = dict(x=x, w1=f16(w1), b1=b1, w2=f16(w2), b2=b2, g3=g3, be3=be3, gf=gf, bef=bef)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in c.items()} | dict(family=family, M=M, D=D, F=F)


def _ln64(s, g, b):
    mu = s.mean(-1, keepdims=True)
    d = s - mu
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5) * g + b


def reference(c):
    """float64: (pre-norm sum s, stream y, out) [M, D] each"""
    d = {k: np.asarray(v, np.float64) for k, v in c.items() if isinstance(v, np.ndarray)}
    a = f16(c["x"]).astype(np.float64) @ d["w1"].T + d["b1"]
    s = d["x"] + d["b2"] + np.maximum(a, 0) @ d["w2"].T
    y = _ln64(s, d["g3"], d["be3"])
    return s, y, _ln64(y, d["gf"], d["bef"])


def ln_bound(s, E, g, y):
    D = s.shape[-1]
    d = s - s.mean(-1, keepdims=True)
    sigma = np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5)
    Ed = E + E.mean(-1, keepdims=True) + 12 * U * np.abs(s).mean(-1, keepdims=True)
    q = np.sqrt((Ed * Ed).mean(-1, keepdims=True))
    ok = q < sigma / 2
    den = np.where(ok, sigma - q, 1.0)
    B = np.abs(g) * (Ed / den + np.abs(d) * q / (sigma * den)) + 20 * U * np.abs(g) * np.abs(d) / sigma + 2 * U * np.abs(y)
    return np.where(ok, B, np.inf)


def bounds(c, split=True):
    """(E_s, E_y, E_out) [M, D] float64 for the split kernel's path, or for the two GEMMs'"""
    d = {k: np.asarray(v, np.float64) for k, v in c.items() if isinstance(v, np.ndarray)}
    D, F = c["D"], c["F"]
    x16 = f16(c["x"]).astype(np.float64)
    a = x16 @ d["w1"].T + d["b1"]
    S1 = np.abs(x16) @ np.abs(d["w1"]).T
    e1 = D * 2.0 ** -23 * S1 + U * (S1 + np.abs(d["b1"]))
    t = np.maximum(a, 0) + e1
    e_h = np.where(a < -e1, 0.0, e1 + np.where(t < 2.0 ** -14, 2.0 ** -25, 2.0 ** -11 * t))
    S2 = (np.maximum(a, 0) + e_h) @ np.abs(d["w2"]).T
    K2, adds = (SLICE, F // SLICE + 2) if split else (F, 3)
    E_s = e_h @ np.abs(d["w2"]).T + K2 * 2.0 ** -23 * S2 + adds * U * (np.abs(d["x"]) + np.abs(d["b2"]) + S2)
    s, y, o = reference(c)
    E_y = ln_bound(s, E_s, d["g3"], y)
    return E_s, E_y, ln_bound(y, E_y, d["gf"], o)


# ---- the kernels' arithmetic in fp32 -------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _mm_blocks(a, w, step=32):
    """fp32: sum over k in ascending blocks of `step`, accumulated from zero; a [M, K], w [N, K]"""
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(0, a.shape[1], step):
        acc = acc + (a[:, k:k + step].astype(np.float64) @ w[:, k:k + step].astype(np.float64).T).astype(np.float32)
    return acc


def _to_f16(v, truncate=False, flush=False):
    v = np.asarray(v, np.float32)
    if truncate:      # toward zero: the nearest fp16 not above |v|
        h = v.astype(np.float16)
        over = np.abs(h.astype(np.float32)) > np.abs(v)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
        return h.astype(np.float32)
    h = v.astype(np.float16)
    if flush:
        sub = (np.abs(h.astype(np.float32)) < 2.0 ** -14) & (h != 0)
        h = np.where(sub, np.copysign(np.float16(0), h), h)
    return h.astype(np.float32)


def _wave_ln(v, g, b):
    """LayerNorm of the rows of v [M, D] fp32 as one wave computes it (D a multiple of 4: two pieces a lane up to 512 - the tail's
    registers -, and as many as detr_postnorm_kernel's `i += 64` loops make trips beyond)"""
    M, D = v.shape
    n4 = D // 4
    P = max(2, -(-n4 // 64))
    lanes = np.zeros((M, P, 64, 4), np.float32)      # [row, piece t, lane, e]: column 4 (lane + 64 t) + e
    lanes.reshape(M, P * 64, 4)[:, :n4] = v.reshape(M, n4, 4)
    have = (np.arange(P * 64) < n4).reshape(P, 64)

    def wsum(x):
        for o in (32, 16, 8, 4, 2, 1):
            x = x + x[:, np.arange(64) ^ o]
        return x[:, :1]

    s = np.zeros((M, 64), np.float32)
    for t in range(P):
        p = (lanes[:, t, :, 0] + lanes[:, t, :, 1]) + (lanes[:, t, :, 2] + lanes[:, t, :, 3])
        s = np.where(have[t], s + p, s)
    mean = wsum(s) / np.float32(D)
    sq = np.zeros((M, 64), np.float32)
    for t in range(P):
        for e in range(4):
            dd = lanes[:, t, :, e] - mean
            sq = np.where(have[t], _fma(dd, dd, sq), sq)
    rstd = np.float32(1.0) / np.sqrt(wsum(sq) / np.float32(D) + np.float32(1e-5))
    return _fma((v - mean) * rstd, np.broadcast_to(g, v.shape), np.broadcast_to(b, v.shape))


def model(c, mutant=None):
    """(partial [n_sl, M, D], pre-norm sum s, stream y, out [M, D]) fp32 as the kernels compute them; `mutant`: one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS
    M, D, F = c["M"], c["D"], c["F"]
    x, n_sl = c["x"], F // SLICE
    x16 = f16(x)
    if mutant == "tail_rows_neighbour" and M > ROWS:      # the last row tile reads the tile before it
        m0 = (M - 1) // ROWS * ROWS
        x16 = x16.copy()
        x16[m0:] = x16[m0 - ROWS:m0 - ROWS + (M - m0)]
    part = np.zeros((n_sl, M, D), np.float32)
    for sl in range(n_sl):
        u = slice(sl * SLICE, (sl + 1) * SLICE)
        ub = slice(((sl + 1) % n_sl) * SLICE, ((sl + 1) % n_sl + 1) * SLICE) if mutant == "b1_wrong_slice" else u
        a = _mm_blocks(x16, c["w1"][u]) + c["b1"][ub]
        if mutant == "relu_after_flush":
            h = np.maximum(_to_f16(a, flush=True), np.float32(0))
        else:
            if mutant != "no_relu":
                a = np.maximum(a, np.float32(0))
            h = _to_f16(a, truncate=mutant == "truncate_f16")
        part[sl] = _mm_blocks(h, c["w2"][:, u])
    order = list(range(n_sl))
    if mutant == "drop_slice":
        order = order[:-1] if n_sl > 1 else []
    if mutant == "double_slice":
        order = order + [n_sl // 2]
    v = x + c["b2"]
    for sl in order:
        v = v + part[sl]
        if mutant == "b2_per_slice" and sl > 0:
            v = v + c["b2"]
    first, second = (("gf", "bef"), ("g3", "be3")) if mutant == "norms_swapped" else (("g3", "be3"), ("gf", "bef"))
    y = _wave_ln(v, c[first[0]], c[first[1]])
    out = _wave_ln(y, c[second[0]], c[second[1]])
    if mutant == "final_norm_written_back":
        y = out
    return part, v, y, out


def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound (inf where a finite value is missing or a zero bound is missed)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())      # (a zero bound - an exact zero output - allows no error)
