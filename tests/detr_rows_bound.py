"""What the five row kernels of hoigen_amd/csrc/hg_detr_rows.hip are held to when each runs alone (hg_test_detr_rows): a float64
reference, a bound PER ELEMENT derived from the roundings the kernels perform, a restatement of their fp32 arithmetic, and bit-exact
statements for everything that is data movement or conversion.  A plain module beside the tests: no fixtures, no GPU, no library.
`ln_bound`, `_wave_ln`, `f16` and `worst_ratio` are tests/detr_ffn_bound.py's (its docstring derives the LayerNorm bound).

Reference (float64)
    post-norm   y = (x - mean) / sqrt(var + 1e-5) g + b, biased variance
    tail        s = ((x + b2) + p_0) + p_1 + ..., y = LayerNorm3(s), out = LayerNorm_final(y)

Bound (every element has |got - want| <= bound; u = 2^-24)
    post-norm   ln_bound(x, 0, g, y): the input is the kernel's own, its error is 0
    tail        E_s = (n_sl + 2) u (|x| + |b2| + sum |p|): the n_sl + 1 additions of the slice sum; E_y = ln_bound(s, E_s, g3, y);
                E_out = ln_bound(y, E_y, gf, out)
    ln_bound counts 12 roundings on the mean and 20 on what multiplies (x - mean) for two 16-byte pieces a lane.  At D = 640 the post-norm's
    loops make three trips: the mean is 4 additions in a lane, 6 in the butterfly and the division (11 <= 12); the variance is 12 fma
    and 6 additions of positive terms, the division and the add (20 relative roundings of the variance, 10 of its root), the root, the
    reciprocal, the subtraction twice (in the squares and in the output) and the multiply: 15 <= 20.  So the same bound holds there.
    ln_bound needs q < sigma / 2 (else it is infinite); `bounds_*` must be finite on every family - the CPU test asserts it.

Restatement (fp32)
    `wave_ln_loops` transliterates detr_postnorm_kernel's three `for (i = lane; i < n4; i += 64)` loops.  detr_dec_tail_kernel holds
    the row in two register pieces a lane instead (`t = 0, 1`, column 4 (lane + 64 t)): trip k of the loop IS piece t = k, the lane's
    sum and fma chain run over them in the same ascending order, and the butterfly is the same, so both kernels are `_wave_ln`'s
    arithmetic: wave_ln_loops(v) == _wave_ln(v) bit for bit at every width (asserted on the CPU, 640 - three trips - included).

Bit-exact statements (`derived`): x16 = fp16(x) and xp16 = fp16(x + p) - the add in fp32, ONE rounding to nearest even -, posb = p,
    copy = x, exit's out = x, and zeros (+0) for a null tgt and a null pos.  For the two norm kernels x is the kernel's own fp32 output.

Buffers: the stream x is read and written in place.  A NaN row normalises to NaN, so a NaN canary cannot see a write into the rows behind
    M of x: those PAD rows hold the finite GUARD instead and must keep their bits (a constant row would come back as the norm's bias);
    every pure output (x16, xp16, copy, out, the entry kernels' four) has NaN canaries.

Families (`make_rows`, `make_tail`; seeded)
    randn      unit Gaussians
    offset     row mean 1000, spread 1 (the three-pass variance has to survive it; E[x^2] - mean^2 does not)
    constant   every channel of a row is the same small multiple of 1/4: the sum and the mean are exact, every x - mean is 0, and
               the output must equal the norm's bias bit for bit
    tiny       spread 1e-4 about a row mean of order 1: var = 1e-8, eps decides the result
    outlier    randn with one channel of each row times 1e4
    exact      integers / 4: the tail's slice sum is exact; compared bit for bit with the restatement
    f16edge    (entry kernels) pairs (x, p) from: ties between two fp16 numbers, sums x + p where rounding each term first gives
               another fp16, fp16 subnormals and the tie at half the smallest, -0, magnitudes past 65504 (65520 is the tie to infinity)
"""
import numpy as np

from detr_ffn_bound import U, _fma, _to_f16, _wave_ln, f16, ln_bound, worst_ratio      # noqa: F401 (re-exported for the tests)

PAD = 4
GUARD = np.float32(1.5)
NORM_FAMILIES = ("randn", "offset", "constant", "tiny", "outlier", "exact")
BITWISE_FAMILIES = ("constant", "exact")
NORM_MUTANTS = ("one_pass_variance", "eps_missing", "eps_1e-6", "variance_over_d_minus_1", "gain_bias_swapped", "xp16_two_roundings",
                "truncate_f16", "columns_from_256_unwritten", "rows_beyond_m_written")
TAIL_MUTANTS = NORM_MUTANTS + ("b2_per_slice", "final_norm_written_back")
ENTRY_MUTANTS = ("xp16_two_roundings", "truncate_f16", "pos_strides_swapped", "columns_from_256_unwritten")
MUTANTS = tuple(dict.fromkeys(TAIL_MUTANTS + ENTRY_MUTANTS))


def _rng(seed, *key):
    return np.random.default_rng([seed, *key])


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def make_rows(family, M, D, seed):
    """x [M, D] float32 of a family, from its own generator"""
    r = _rng(seed, M, D, NORM_FAMILIES.index(family))
    if family == "randn":
        x = r.standard_normal((M, D))
    elif family == "offset":
        x = 1000.0 + r.standard_normal((M, D))
    elif family == "constant":
        x = np.repeat(r.integers(-8, 9, (M, 1)) / 4, D, axis=1)
    elif family == "tiny":
        x = r.standard_normal((M, 1)) + 1e-4 * r.standard_normal((M, D))
    elif family == "outlier":
        x = r.standard_normal((M, D))
        x[np.arange(M), (7 * np.arange(M) + 3) % D] *= 1e4
    else:
        assert family == "exact", family
        x = r.integers(-16, 17, (M, D)) / 4
    return _f32(x)


def _norm_params(r, D):
    return _f32(1 + 0.2 * r.standard_normal(D)), _f32(0.1 * r.standard_normal(D))


def make_postnorm(family, M, D, seed):
    r = _rng(seed, M, D, 101)
    g, b = _norm_params(r, D)
    return dict(family=family, M=M, D=D, x=make_rows(family, M, D, seed), g=g, b=b, pos=_f32(r.standard_normal((M, D))))


def make_tail(family, M, D, n_sl, seed, with_b2=True):
    """x [M, D], b2 [D] or None, part [n_sl, M, D], norm3 (g3, be3), the final norm (gf, bef), qpos [M, D]"""
    r = _rng(seed, M, D, n_sl, 102)
    x = make_rows(family, M, D, seed)
    if family == "constant":      # a row of every operand is one value: the slice sum is exact and constant along the row
        part, b2 = np.repeat(r.integers(-8, 9, (n_sl, M, 1)) / 4, D, axis=2), np.repeat(r.integers(-8, 9, 1) / 4, D)
    elif family == "exact":
        part, b2 = r.integers(-8, 9, (n_sl, M, D)) / 4, r.integers(-8, 9, D) / 4
    else:
        k = 1e-5 if family == "tiny" else 0.3
        part, b2 = k * r.standard_normal((n_sl, M, D)), k / 3 * r.standard_normal(D)
    g3, be3 = _norm_params(r, D)
    gf, bef = _norm_params(r, D)
    return dict(family=family, M=M, D=D, n_sl=n_sl, x=x, b2=_f32(b2) if with_b2 else None, part=_f32(part), g3=g3, be3=be3, gf=gf, bef=bef,
                qpos=_f32(r.standard_normal((M, D))))


# fp16 edges: (x, p) pairs, all exact fp32 numbers
_E = 2.0 ** -10
F16_EDGE_PAIRS = (
    (1 + _E / 2, 0.0), (1 + 3 * _E / 2, 0.0), (-(1 + _E / 2), 0.0), (2048.0 + 1.0, 0.0), (2048.0 + 3.0, 0.0),      # ties: to even
    (1 + 3 * 2.0 ** -13, 3 * 2.0 ** -13), (1 + _E / 4, _E / 2), (-(1 + 3 * 2.0 ** -13), -3 * 2.0 ** -13),        # x + p rounds up, fp16(x) + fp16(p) does not
    (1 + _E / 2 + 2.0 ** -20, -(2.0 ** -20)), (0.1, 0.2), (1.0 / 3, 1000.0),
    (2.0 ** -24, 0.0), (3 * 2.0 ** -24, 0.0), (2.0 ** -25, 0.0), (1.5 * 2.0 ** -24, 0.0), (2.0 ** -15 + 2.0 ** -24, 0.0),      # subnormals, ties
    (2.0 ** -25 + 2.0 ** -40, 0.0), (-(2.0 ** -24), 0.0), (2.0 ** -25, 2.0 ** -25), (2.0 ** -14, -(2.0 ** -24)),
    (-0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (1.0, -1.0),                                                               # -0
    (65504.0, 0.0), (65519.0, 0.0), (65520.0, 0.0), (-65520.0, 0.0), (1e5, 0.0), (-7e4, 0.0), (65504.0, 15.0), (65504.0, 16.0),      # past the largest
    (40000.0, 40000.0), (1e5, -5e4),
)


def make_f16edge(rows, D):
    """(x, p) [rows, D] float32: the pairs above, cyclically, shifted by one from row to row so that every column sees every pair"""
    n = len(F16_EDGE_PAIRS)
    idx = (np.arange(rows)[:, None] + np.arange(D)[None, :]) % n
    pairs = np.array(F16_EDGE_PAIRS, np.float32)
    return _f32(pairs[idx, 0]), _f32(pairs[idx, 1])


def make_entry(family, B, T, D, seed):
    """logical src, pos [B, T, D] float32 for the entry kernels (`randn` or `f16edge`)"""
    if family == "f16edge":
        x, p = make_f16edge(B * T, D)
        return x.reshape(B, T, D), p.reshape(B, T, D)
    r = _rng(seed, B, T, D, 103)
    return _f32(r.standard_normal((B, T, D))), _f32(r.standard_normal((B, T, D)))


# ---- float64 -------------------------------------------------------------------------------------------------------------------------
def _ln64(s, g, b):
    mu = s.mean(-1, keepdims=True)
    d = s - mu
    return d / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5) * g + b


def reference_postnorm(c):
    return _ln64(c["x"].astype(np.float64), c["g"].astype(np.float64), c["b"].astype(np.float64))


def bounds_postnorm(c):
    x = c["x"].astype(np.float64)
    return ln_bound(x, np.zeros_like(x), c["g"].astype(np.float64), reference_postnorm(c))


def reference_tail(c):
    """float64 (s, y, out) [M, D]"""
    d = lambda k: c[k].astype(np.float64)
    s = d("x") + (d("b2") if c["b2"] is not None else 0.0) + d("part").sum(0)
    y = _ln64(s, d("g3"), d("be3"))
    return s, y, _ln64(y, d("gf"), d("bef"))


def bounds_tail(c):
    """(E_s, E_y, E_out) [M, D] float64"""
    d = lambda k: np.abs(c[k].astype(np.float64))
    s, y, o = reference_tail(c)
    E_s = (c["n_sl"] + 2) * U * (d("x") + (d("b2") if c["b2"] is not None else 0.0) + d("part").sum(0))
    E_y = ln_bound(s, E_s, c["g3"].astype(np.float64), y)
    return E_s, E_y, ln_bound(y, E_y, c["gf"].astype(np.float64), o)


# ---- the kernels' arithmetic in fp32 -------------------------------------------------------------------------------------------------
def _wsum(x):
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, np.arange(64) ^ o]
    return x[:, :1]


def wave_ln_loops(v, g, b, mutant=None):
    """detr_postnorm_kernel's three loops over a row, one wave a row: lane `lane` visits the 16-byte pieces i = lane, lane + 64, ..."""
    v = _f32(v)
    M, D = v.shape
    n4 = D // 4
    g, b = np.broadcast_to(_f32(g), v.shape), np.broadcast_to(_f32(b), v.shape)
    if mutant == "gain_bias_swapped":
        g, b = b, g
    lane = np.arange(64)
    v4 = v.reshape(M, n4, 4)

    def trips():
        for i0 in range(0, n4, 64):
            i = i0 + lane
            yield i < n4, v4[:, np.minimum(i, n4 - 1)]      # [64], [M, 64, 4]

    with np.errstate(all="ignore"):
        s = np.zeros((M, 64), np.float32)
        for have, p in trips():
            s = np.where(have, s + ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])), s)
        mean = _wsum(s) / np.float32(D)
        sq = np.zeros((M, 64), np.float32)
        for have, p in trips():
            for e in range(4):
                dd = p[..., e] if mutant == "one_pass_variance" else p[..., e] - mean
                sq = np.where(have, _fma(dd, dd, sq), sq)
        var = _wsum(sq) / np.float32(D - 1 if mutant == "variance_over_d_minus_1" else D)
        if mutant == "one_pass_variance":
            var = var - mean * mean
        eps = np.float32({"eps_missing": 0.0, "eps_1e-6": 1e-6}.get(mutant, 1e-5))
        rstd = np.float32(1.0) / np.sqrt(var + eps)
        return _fma((v - mean) * rstd, g, b)


def _cvt(v, mutant):
    with np.errstate(over="ignore"):
        return _to_f16(v, truncate=mutant == "truncate_f16")


def _sum16(x, p, mutant):
    """xp16 as fp32 numbers: fp16(x + p), the add in fp32"""
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == "xp16_two_roundings":
            return _cvt(_cvt(x, None) + _cvt(p, None), None)
        return _cvt(_f32(x) + _f32(p), mutant)


def derived(x, pos=None):
    """(x16, xp16 or None, copy) as fp32 arrays from an fp32 x [M, D]: what the norm kernels must write beside it, bit for bit"""
    return _cvt(x, None), (None if pos is None else _sum16(x, pos, None)), _f32(x).copy()


def _stream_buffer(x):
    return np.concatenate([_f32(x), np.full((PAD, x.shape[1]), GUARD, np.float32)])


def _canary(M, D):
    return np.full((M + PAD, D), np.nan, np.float32)


def _norm_outputs(buf, y, rows, cols, pos, want_copy, mutant):
    """write a norm kernel's outputs for `rows` rows and `cols` columns: the stream in place, x16, xp16 (pos given), copy"""
    M_all, D = buf.shape
    out = dict(x=buf, x16=_canary(M_all - PAD, D), xp16=_canary(M_all - PAD, D) if pos is not None else None,
               copy=_canary(M_all - PAD, D) if want_copy else None)
    sl = (slice(0, rows), slice(0, cols))
    buf[sl] = y[sl]
    out["x16"][sl] = _cvt(y, mutant)[sl]
    if want_copy:
        out["copy"][sl] = y[sl]
    if pos is not None:
        pp = np.zeros_like(y)
        pp[:pos.shape[0]] = pos
        out["xp16"][sl] = _sum16(y, pp, mutant)[sl]
    return out


def model_postnorm(c, mutant=None, with_pos=True, with_copy=True):
    """detr_postnorm_kernel on buffers of M + PAD rows -> dict x (in place; GUARD rows behind M), x16, xp16, copy (NaN rows behind M)"""
    assert mutant is None or mutant in NORM_MUTANTS, mutant
    M, D = c["M"], c["D"]
    buf = _stream_buffer(c["x"])
    rows = -(-M // 4) * 4 if mutant == "rows_beyond_m_written" else M      # (the whole workgroup of four rows)
    cols = min(D, 256) if mutant == "columns_from_256_unwritten" else D
    y = wave_ln_loops(buf, c["g"], c["b"], mutant)
    return _norm_outputs(buf, y, rows, cols, c["pos"] if with_pos else None, with_copy, mutant)


def model_tail(c, mutant=None, with_pos=True, with_copy=True, with_out=True):
    """detr_dec_tail_kernel -> model_postnorm's dict and `out` [M + PAD, D] (dense rows; the test lays them out)"""
    assert mutant is None or mutant in TAIL_MUTANTS, mutant
    M, D, n_sl = c["M"], c["D"], c["n_sl"]
    buf = _stream_buffer(c["x"])
    part = np.concatenate([c["part"], np.zeros((n_sl, PAD, D), np.float32)], axis=1)
    rows = -(-M // 4) * 4 if mutant == "rows_beyond_m_written" else M      # (the whole workgroup of four rows)
    cols = min(D, 256) if mutant == "columns_from_256_unwritten" else D
    v = buf.copy()
    if c["b2"] is not None:
        v = v + c["b2"]
    for sl in range(n_sl):
        v = v + part[sl]
        if mutant == "b2_per_slice" and sl > 0 and c["b2"] is not None:
            v = v + c["b2"]
    y = wave_ln_loops(v, c["g3"], c["be3"], mutant)
    o = wave_ln_loops(y, c["gf"], c["bef"], mutant)
    if mutant == "final_norm_written_back" and with_out:
        y = o
    res = _norm_outputs(buf, y, rows, cols, c["qpos"] if with_pos else None, with_copy, mutant)
    res["out"] = None
    if with_out:
        res["out"] = _canary(M, D)
        res["out"][:rows, :cols] = o[:rows, :cols]
    return res


def model_entry(src, pos, sb, ss, pb, ps, B, T, D, mutant=None):
    """detr_entry_kernel / detr_dec_entry_kernel on FLAT fp32 buffers with element strides, as the kernels address them: element
    (b, t, ch) of src at b * sb + t * ss + ch.  src None (a null tgt) or pos None (a null pos) read as +0.
    -> dict x, x16, xp16, posb [B * T + PAD, D] with NaN rows behind the last"""
    assert mutant is None or mutant in ENTRY_MUTANTS, mutant
    b, t = np.divmod(np.arange(B * T), T)
    ch = np.arange(D)

    def rows(flat, s_b, s_t, swap=False):
        if flat is None:
            return np.zeros((B * T, D), np.float32)
        off = (t * s_b + b * s_t) if swap else (b * s_b + t * s_t)
        return _f32(flat)[(off[:, None] + ch[None, :]) % flat.size]

    v, p = rows(src, sb, ss), rows(pos, pb, ps, mutant == "pos_strides_swapped")
    cols = min(D, 256) if mutant == "columns_from_256_unwritten" else D
    out = {k: _canary(B * T, D) for k in ("x", "x16", "xp16", "posb")}
    for k, a in (("x", v), ("x16", _cvt(v, mutant)), ("xp16", _sum16(v, p, mutant)), ("posb", p)):
        out[k][:B * T, :cols] = a[:, :cols]
    return out


def model_exit(x, ob, os_, B, T, D, size):
    """detr_exit_kernel: a flat NaN buffer of `size` elements with out[b * ob + t * os + ch] = x[b * T + t, ch]"""
    out = np.full(size, np.nan, np.float32)
    b, t = np.divmod(np.arange(B * T), T)
    out[(b * ob + t * os_)[:, None] + np.arange(D)[None, :]] = _f32(x)[:B * T]
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pads_intact(res, M, guard_x):
    """names of the buffers of a result dict whose rows behind M are no longer what they were: NaN, or GUARD for an in-place x"""
    bad = []
    for k, a in res.items():
        if a is None:
            continue
        tail = a[M:]
        if not (same_bits(tail, np.full_like(tail, GUARD)) if k == "x" and guard_x else bool(np.isnan(tail).all())):
            bad.append(k)
    return bad


def judge_norm(res, M, want, bound, pos, exact=None, what="x"):
    """failures (strings) of a norm kernel's result dict against the float64 `want` with `bound`, the bit-exact statements derived from
    its own fp32 stream, its pads, and - where `exact` (the restatement's stream) is given - bit equality with that; and the worst ratio"""
    fails = [f"rows behind M of {k} were written" for k in pads_intact(res, M, True)]
    x = res["x"][:M]
    r = worst_ratio(x, want, bound)
    if not r <= 1.0:
        fails.append(f"{what}: worst |err| / bound {r:.3g}")
    if exact is not None and not same_bits(x, exact[:M]):
        fails.append(f"{what}: not the restatement's bits ({int((bits(x) != bits(exact[:M])).sum())} elements)")
    x16, xp16, copy = derived(x, pos)
    for k, w in (("x16", x16), ("xp16", xp16), ("copy", copy)):
        if res.get(k) is not None and not same_bits(res[k][:M], w):
            fails.append(f"{k}: not derived from the kernel's own fp32 stream bit for bit ({int((bits(res[k][:M]) != bits(w)).sum())} elements)")
    return fails, r
