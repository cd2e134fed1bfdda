"""What the row / elementwise kernels of hoigen_amd/csrc/hg_elem.hip (and finalize_stats_row, hg_gemm_dev.h) are held to: the operation
evaluated in float64 on the CPU from the fp32 / fp16 inputs, and a bound PER OUTPUT ELEMENT that is the sum of the worst case of each
rounding the source performs.  A plain module beside the tests (tests/test_elem_rounding_model.py, tests/test_gpu_elem.py import it): no
fixtures, no GPU, no library; numpy only.  The reasoning is that of tests/gemm_bound.py wherever a term exists there (B_mean, the M2
perturbation argument of B_rstd, the fp16 output term with t = |want| + the fp32 terms and the subnormal step) and is said so below.

u = 2^-24.  ASSUMED, not measured (as gemm_bound.py assumes 1 ulp for v_exp_f32): an fp32 division is off by at most 2.5 ulp (DIV =
5 u relative), sqrtf by at most 3 ulp (SQRT = 6 u), expf by at most 4 ulp (EXP = 8 u).  2.5 and 3 ulp are the limits OpenCL's full profile
sets for them; the library is built without fast-math, where hipcc asks for the correctly rounded forms (0.5 ulp), so the assumption has
four to six times that as slack.  Every term below that carries DIV, SQRT or EXP rests on it.  "Sum of n terms in any order":
|computed - exact| <= n u sum |term| (the classical (n - 1) u / (1 - (n - 1) u), rounded up to n u, which holds for n <= 4096).

LayerNorm (layernorm_kernel) and the statistics of rowstats_cast / layernorm_rowstats: two passes, one wave per row, D columns.
    A = sum |x_j|, mean = sum x_j / D, d_j = x_j - mean, M2 = sum d_j^2, rstd = 1 / sqrt(M2 / D + 1e-5f)      (float64; 1e-5f the fp32 constant)
    mean      D values in any order, then one division:   B_mean = u A + DIV (|mean| + u A)            (gemm_bound's B_mean with one group of D)
    d^        fl(x - mean^): off from d by dm = mean^ - mean (the same for every column) and rho_j, |rho_j| <= u a_j, a_j = |d_j| + B_mean
    q         sum_j d^_j^2 = M2 + D dm^2 + 2 sum (d_j - dm) rho_j + sum rho_j^2: the cross term sum d_j dm vanishes, as in gemm_bound's M2
              argument; each square rounds once and the D terms (all >= 0) are summed in any order, relative (D + 2) u (an fma that
              fuses square and add rounds once less):
              E_q = E1 + (D + 2) u (M2 + E1),   E1 = D B_mean^2 + (2 u + u^2) sum a_j^2
    rstd      / D (DIV), + 1e-5f (u), sqrtf (SQRT), 1 / . (DIV): halves of the first two, the last two whole, one u for second order:
              B_rstd = rstd (E_q / (2 (M2 + 1e-5f D)) + 15 u)
    y         (x - mean^) rstd^ g + b as four operations (a contraction of the last two into an fma rounds once less):
              e1 = (B_mean + u a) (rstd + B_rstd) + |d| B_rstd, + u (|d rstd| + e1);   e2 = e1 |g| + u (|d rstd g| + e1 |g|);
              B_y = e2 + u (|y| + e2);  layernorm_f16 adds the fp16 term f16(|y| + B_y): 2^-11 t, or 2^-25 where t < 2^-14 (gemm_bound.f16_term)
    copy      against the mu the kernel RETURNED: fp16(fl(x - mu)): u |x - mu| + f16(|x - mu| (1 + u)); with gamma, fp16(fl(fl(x - mu) gamma)):
              2 u |want| + f16(|want| (1 + 2 u))                                                      (gemm_bound's copy terms, unchanged)
    mu and mr[:, 1] are judged against the float64 mean and rstd of the input with B_mean and B_rstd; mr[:, 0] == 0 and muc == mu exactly.

finalize_stats (finalize_stats_row): the inputs are the fp32 partials (s_g, M2_g) of G = nt groups of gw columns, D = nt gw; the
expectation is Chan's merge of those numbers in float64: mean = sum s_g / D, M2 = sum [M2_g + gw (s_g / gw - mean)^2].  gemm_bound's
(70 + 2 G) u derivation without the in-group part (the groups arrive finished):
    mean      G sums in order, one division:   B_mean = G u sum |s_g| / D + DIV (|mean| + G u sum |s_g| / D)
    mr[:, 0]  fl(mean^ - c): B_mean + u (|mean - c| + B_mean); with `centred` it is mean^ itself: B_mean.  mu <- mean^ (the same bits as
              mr[:, 0] + ... is not required: mu is judged with B_mean), or stays when centred; muc <- the old mu, bit for bit.
    M2        g^ = fl(s_g / gw) (DIV |g|), d0 = fl(g^ - mean^) = (g - mean) - dm + rho_g, |rho_g| <= DIV |g| + u a_g, a_g = |g - mean| + B_mean +
              DIV |g|; sum gw (g - mean) dm = 0 exactly, so only D dm^2 is left of the common shift.  Two multiplies and one add per
              group (3 u), G additions of non-negative terms (G u), one u for second order:
              E_M2 = D B_mean^2 + sum_g gw (2 a_g rho_g + rho_g^2) + (G + 4) u (M2 + sum_g gw a_g^2),   B_rstd = rstd (E_M2 / (2 (M2 + 1e-5f D)) + 15 u)
    The hand-unrolled nt == 12 path is held to the same bound as the loop (not to the loop's bits: contraction may differ).

fold_ln: wf16 == fp16(fl(w gamma)) bit for bit (one fp32 multiply, one RNE).  cs against the float64 sum of the RETURNED wf16: K exact
terms in any order, K u sum |wf|.  bf = bias + sum w beta and csg = sum w gamma: each product rounds once, K terms in any order, the bias add once:
(K + 1) u sum |w beta| + u (|bf| + (K + 1) u sum |w beta|), csg without the last term.
l2_normalize: q = sum x^2 (each square u, or half a subnormal step 2^-150 where it underflows; D terms any order), sqrtf, 1 / ., one multiply:
B = |want| ((D + 2) u / 2 + D 2^-150 / (2 q) + SQRT + DIV + 2 u).  Where q exceeds FLT_MAX (1 + (D + 2) u) the fp32 sum is +Inf and the row is
expected as zeros; between FLT_MAX (1 - (D + 2) u) and that the reference refuses the row.
vae_loss: sum over R D of t = d^2 - 0.5 (1 + lv - m^2 - exp(lv)), d = recon - x, divided by R.  Per term, from the source's operations:
e_t = u (4 d^2 + 2 |1 + lv| + 2 m^2) + (EXP / 2 + u) exp(lv); the n = R D terms in any order (lanes, wave, workgroup, atomicAdd), the division
per workgroup: B = (n u sum (|t| + e_t) + sum e_t) (1 + DIV) / R + DIV sum |t| / R.  Order-dependent: a bound, never a bit test.
f16_remainder: fp16((x - fp16(x)) 2048) is exact in fp32 up to the last rounding: expected bit for bit (remainder_expected).
Everything else is data movement or conversion: a numpy / torch indexing expression, bit for bit.

Rule: every element of every output is bit-equal or has |got - want| <= B.  No global scale, no row norm, no element left out.

`model_*` restate the arithmetic kernels in fp32 numpy (LayerNorm, rowstats, finalize_stats in the loop order and in the nt == 12 order,
fold_ln) with the mutants tests/test_elem_rounding_model.py proves the bound catches (MUTANTS).

Input families (`make_rows`; seeded, generated on the CPU): randn; offset 100 + 0.5 randn (why the copy is centred); small 0.3 + 0.02 randn
(the copy reaches fp16's subnormals); wide 2 randn + 8 randn per row, every 97th column x 30; constant: every third row constant (an
integer / 4), variance exactly 0; exact: c + a pattern of +- pairs on a 1/8 grid, c a multiple of 1/4 - sum, mean and every d exact in
any order; nonfinite: randn with an Inf in one row and a NaN in another.  fold_ln: randn, and drift (w a positive power of two, gamma =
1 + 2^-12: every fp16 rounding of w gamma goes the same way).

Worst |err| / B over all elements, `model` / kernel: the model at the shapes of tests/test_elem_rounding_model.py, the kernels as
tests/test_gpu_elem.py prints them (lines starting ELEM_RATIO) on an MI355X, worst over its shapes.

    kernel . quantity           randn           offset          small           wide            constant        exact           drift
    layernorm_f16               0.985 / 0.985   0.863 / 0.863   0.950 / 0.950   0.986 / 0.986   0.985 / 0.985   0.978 / 0.978   -
    layernorm_f32               0.131 / 0.145   0.108 / 0.107   0.151 / 0.151   0.250 / 0.250   0.146 / 0.141   0.084 / 0.084   -
    rowstats_cast.copy          1.000 / 1.000   0.999 / 0.999   1.000 / 1.000   1.000 / 1.000   1.000 / 1.000   0     / 0       -
    rowstats_cast.mean          0.168 / 0.168   0.108 / 0.108   0.152 / 0.152   0.184 / 0.184   0.172 / 0.172   0     / 0       -
    rowstats_cast.rstd          0.133 / 0.133   0.112 / 0.112   0.106 / 0.106   0.125 / 0.125   0.129 / 0.129   0.071 / 0.071   -
    rowstats_cast, gamma .copy  0.999 / 0.999   0.999 / 0.999   1.000 / 1.000   0.999 / 0.999   0.999 / 0.999   0.991 / 0.991   -
    layernorm_rowstats.copy     -     / 1.000   -     / 1.000   -               -               -     / 1.000   -               -
    layernorm_rowstats.mean     -     / 0.159   -     / 0.155   -               -               -     / 0.153   -               -
    layernorm_rowstats.rstd     -     / 0.144   -     / 0.139   -               -               -     / 0.128   -               -
    finalize_stats.mean         0.214 / 0.214   0.207 / 0.178   0.224 / 0.224   0.201 / 0.201   -               -               -
    finalize_stats.mr0          0.383 / 0.383   0.207 / 0.178   0.222 / 0.222   0.201 / 0.201   -               -               -
    finalize_stats.rstd         0.104 / 0.104   0.133 / 0.133   0.125 / 0.125   0.135 / 0.127   -               -               -
    finalize_stats nt 12 .mean  0.125 / 0.125   0.207 / 0.207   0.196 / 0.196   0.184 / 0.184   -               -               -
    finalize_stats nt 12 .mr0   0.147 / 0.147   0.207 / 0.207   0.194 / 0.194   0.184 / 0.184   -               -               -
    finalize_stats nt 12 .rstd  0.103 / 0.103   0.132 / 0.132   0.112 / 0.112   0.135 / 0.135   -               -               -
    fold_ln.cs                  0.002 / 0.002   -               -               -               -               -               0     / 0
    fold_ln.bf                  0.003 / 0.003   -               -               -               -               -               0.002 / 0.002
    fold_ln.csg                 0.006 / 0.006   -               -               -               -               -               0     / 0
    vae_loss                    -     / 0.081   l2_normalize (wide rows, the 1e-20 and the 1e18 row)   - / 0.600

Recorded, not tuned to; no entry is above 1 (1.000 is 0.9995 or more, rounded; the tests assert <= 1).  layernorm_rowstats is judged on
the LayerNorm output it wrote (its bits equal layernorm_f32 + rowstats_cast, which the test asserts; the model column is theirs).  The
statistics of `constant` leave out the zero-variance rows, which are held to 15 u of 1 / sqrt(1e-5f) and to the bits of mu instead (the
any-order B_mean^2 / 1e-5 is no statement about them).  The copy and layernorm_f16 sit at 0.99 - 1.000: one fp16 rounding is nearly all they
are allowed, and a result just above a power of two uses it up.  The kernels land on the model almost to the digit because model and kernel
add in the same order (lane partials, xor butterfly); where they differ (layernorm_f32, finalize_stats on `offset` and `wide`) it is the fma
contraction the bound counts as two roundings.  mean and rstd stay below 0.4: D u sum |x| is the worst case over every order, and 2.5 / 3 ulp
for the division and sqrtf is five to six times what a correctly rounded one needs.  fold_ln's sums are far below the (K + 1) u sum |.| of an
arbitrary order of K = 64 .. 1000 terms.  l2_normalize's 0.600 is the 1e-20 row at D = 1: its square is an fp32 subnormal, half a step is
what the bound allows and most of it is used.

A finding of these tests: fold_ln's wf16.  Built with -ffp-contract=fast, `(half_t)(w * gamma[k])` became one mixed-precision instruction
that rounds the exact product once: at (N, K) = (128, 768) 3 of 98 304 weights and at (7, 1000) 1 of 7 000 were one fp16 step off
fp16(fl(w gamma)) and equal to the once-rounded product (e. g. w = 0x25de, gamma = 1.1561251878738403: 0x26c9 for 0x26c8); none on
`drift`, whose products are exact in fp32.  The kernel now rounds the product to fp32 first, as its source and hg_kernels.h state.
"""
import functools

import numpy as np

U = 2.0 ** -24
DIV, SQRT, EXP = 5 * U, 6 * U, 8 * U          # assumed: 2.5, 3 and 4 ulp
EPS32 = float(np.float32(1e-5))
FLT_MAX = float(np.finfo(np.float32).max)
ROW_FAMILIES = ("randn", "offset", "small", "wide", "constant", "exact", "nonfinite")
FOLD_FAMILIES = ("randn", "drift")
DS = (4, 64, 252, 256, 260, 512, 768, 1020, 1024)
MS = (1, 3, 4, 5, 1027)
MUTANTS = ("var_naive", "no_eps", "unbiased", "copy_uncentred", "f16_truncate", "f16_flush", "chan_no_cross", "mr0_sign", "cs_unrounded")
f32 = np.float32
RSTD0 = 1.0 / np.sqrt(EPS32)


def seed_of(family, *dims):
    s = (ROW_FAMILIES + FOLD_FAMILIES).index(family) + 1
    for d in dims:
        s = s * 8209 + int(d)
    return s


@functools.lru_cache(maxsize=8)
def make_rows(family, M, D):
    """x [M, D] float32 (read-only: shared by the tests).  `nonfinite` is `randn` with an Inf in row 0 and a NaN in row 2 (M >= 3) or 1."""
    base = "randn" if family == "nonfinite" else family
    g = np.random.default_rng(seed_of(base, M, D))
    x = g.standard_normal((M, D))
    if family == "offset":
        x = 100.0 + 0.5 * x
    elif family == "small":
        x = 0.3 + 0.02 * x
    elif family == "wide":
        x = 2 * x + 8 * g.standard_normal((M, 1))
        x[:, 5::97] *= 30.0
    elif family == "constant":
        x[::3] = np.round(400.0 * g.standard_normal((M, 1)))[::3] / 4
    elif family == "exact":
        half = g.integers(-16, 17, (M, D // 2)) / 8.0
        pat = np.concatenate([half, -half], 1)
        pat = np.take_along_axis(pat, np.argsort(g.random((M, D)), 1), 1)
        x = g.integers(-256, 257, (M, 1)) / 4.0 + pat
    elif family == "nonfinite":
        x[0, (3 * D) // 4] = np.inf
        if M > 1:
            x[min(2, M - 1), D // 3] = np.nan
    x = x.astype(f32)
    x.setflags(write=False)
    return x


def nonfinite_rows(M):
    return sorted({0, min(2, M - 1)})


def make_affine(D, seed=0):
    """LayerNorm weight and bias [D] float32"""
    g = np.random.default_rng(977 * D + seed)
    return (1.0 + 0.3 * g.standard_normal(D)).astype(f32), (0.2 * g.standard_normal(D)).astype(f32)


@functools.lru_cache(maxsize=8)
def make_stats(family, M, nt, gw, centred=False):
    """Partial statistics as a residual GEMM leaves them: stats [M, nt, 2] fp32 = (sum, M2 about the group mean) of the groups of
    make_rows(family, M, nt gw), and the centre mu [M] the copy was written with (near the mean; `centred`: the rows are centred first).
    `nonfinite` has the centres of `randn`: the finite mean a row had before it turned non-finite."""
    x = make_rows(family, M, nt * gw).astype(np.float64)
    base = "randn" if family == "nonfinite" else family
    g = np.random.default_rng(seed_of(base, M, nt, gw) + 1)
    mu = make_rows(base, M, nt * gw).astype(np.float64).mean(1) + 0.05 * g.standard_normal(M)
    if centred:
        x = x - mu.astype(f32).astype(np.float64)[:, None]
    xg = x.reshape(M, nt, gw)
    with np.errstate(all="ignore"):
        s = xg.sum(2)
        m2 = ((xg - s[:, :, None] / gw) ** 2).sum(2)
        stats = np.stack([s, m2], 2).astype(f32)
    stats.setflags(write=False)
    mu = mu.astype(f32)
    mu.setflags(write=False)
    return stats, mu


@functools.lru_cache(maxsize=8)
def make_fold(family, N, K):
    """w16 [N, K] float16, gamma, beta [K], bias [N] float32"""
    g = np.random.default_rng(seed_of(family, N, K))
    if family == "drift":
        w = 2.0 ** g.integers(-1, 2, (N, K))
        gamma = np.full(K, 1.0 + 2.0 ** -12)
    else:
        w = g.standard_normal((N, K)) * K ** -0.5
        gamma = 1.0 + 0.3 * g.standard_normal(K)
    out = (w.astype(np.float16), gamma.astype(f32), (0.2 * g.standard_normal(K)).astype(f32), (0.1 * g.standard_normal(N)).astype(f32))
    for a in out:
        a.setflags(write=False)
    return out


# ---- float64 references and bounds ----------------------------------------------------------------------------------------------------
def f16_term(t):
    """worst case of one RNE rounding to fp16 of a computed value of magnitude <= t (gemm_bound.f16_term)"""
    return np.where(t < 2.0 ** -14, 2.0 ** -25, 2.0 ** -11 * t)


def row_stats_reference(x):
    """float64 statistics of the rows of x [M, D] and their bounds: dict of mean, d, M2, rstd, B_mean, B_rstd"""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    with np.errstate(all="ignore"):
        A = np.abs(x).sum(1)
        mean = x.sum(1) / D
        d = x - mean[:, None]
        M2 = (d * d).sum(1)
        rstd = 1.0 / np.sqrt(M2 / D + EPS32)
        B_mean = U * A + DIV * (np.abs(mean) + U * A)
        a = np.abs(d) + B_mean[:, None]
        E1 = D * B_mean ** 2 + (2 * U + U * U) * (a * a).sum(1)
        E_q = E1 + (D + 2) * U * (M2 + E1)
        B_rstd = rstd * (E_q / (2 * (M2 + EPS32 * D)) + 15 * U)
    return {"mean": mean, "d": d, "M2": M2, "rstd": rstd, "B_mean": B_mean, "B_rstd": B_rstd}


def layernorm_reference(x, w, b, f16):
    """(want, B) [M, D] of LayerNorm(x; w, b), float64"""
    s = row_stats_reference(x)
    g, be = np.asarray(w, np.float64)[None], np.asarray(b, np.float64)[None]
    with np.errstate(all="ignore"):
        d, rstd, B_mean, B_rstd = s["d"], s["rstd"][:, None], s["B_mean"][:, None], s["B_rstd"][:, None]
        a = np.abs(d) + B_mean
        e1 = (B_mean + U * a) * (rstd + B_rstd) + np.abs(d) * B_rstd
        e1 = e1 + U * (np.abs(d * rstd) + e1)
        e2 = e1 * np.abs(g)
        e2 = e2 + U * (np.abs(d * rstd * g) + e2)
        want = d * rstd * g + be
        B = e2 + U * (np.abs(want) + e2)
        if f16:
            B = B + f16_term(np.abs(want) + B)
    return want, B


def copy_reference(x, mu, gamma=None):
    """(want, B) of the centred fp16 copy against the RETURNED centre mu [M] (fp32)"""
    with np.errstate(all="ignore"):
        d = np.asarray(x, np.float64) - np.asarray(mu, np.float64)[:, None]
        if gamma is None:
            return d, U * np.abs(d) + f16_term(np.abs(d) * (1 + U))
        want = d * np.asarray(gamma, np.float64)[None]
        return want, 2 * U * np.abs(want) + f16_term(np.abs(want) * (1 + 2 * U))


def finalize_reference(stats, mu, gw, centred):
    """Chan's merge in float64 of stats [M, nt, 2] (fp32 numbers): dict of mean, mr0, rstd, B_mean, B_mr0, B_rstd"""
    st = np.asarray(stats, np.float64)
    c = np.asarray(mu, np.float64)
    nt = st.shape[1]
    D = nt * gw
    with np.errstate(all="ignore"):
        s, m2g = st[:, :, 0], st[:, :, 1]
        e_sum = nt * U * np.abs(s).sum(1) / D
        mean = s.sum(1) / D
        B_mean = e_sum + DIV * (np.abs(mean) + e_sum)
        gm = s / gw
        dev = gm - mean[:, None]
        M2 = (m2g + gw * dev * dev).sum(1)
        rstd = 1.0 / np.sqrt(M2 / D + EPS32)
        a = np.abs(dev) + B_mean[:, None] + DIV * np.abs(gm)
        rho = DIV * np.abs(gm) + U * a
        E = (D * B_mean ** 2 + (gw * (2 * a * rho + rho * rho)).sum(1) + (nt + 4) * U * (M2 + (gw * a * a).sum(1)))
        B_rstd = rstd * (E / (2 * (M2 + EPS32 * D)) + 15 * U)
        mr0 = mean if centred else mean - c
        B_mr0 = B_mean if centred else B_mean + U * (np.abs(mean - c) + B_mean)
    return {"mean": mean, "mr0": mr0, "rstd": rstd, "B_mean": B_mean, "B_mr0": B_mr0, "B_rstd": B_rstd}


def fold_wf16_expected(w16, gamma):
    """fp16(fl(w gamma)): one fp32 multiply, one RNE - the bits fold_ln must write"""
    return (w16.astype(f32) * gamma[None].astype(f32)).astype(np.float16)


def fold_reference(w16, gamma, beta, bias, wf16):
    """dict of cs, bf, csg (want) and B_cs, B_bf, B_csg [N]; cs from the RETURNED wf16"""
    w = w16.astype(np.float64)
    K = w.shape[1]
    wf = np.asarray(wf16).astype(np.float64)
    pb, pg = w * beta.astype(np.float64)[None], w * gamma.astype(np.float64)[None]
    bf = pb.sum(1) + (0.0 if bias is None else bias.astype(np.float64))
    e_b = (K + 1) * U * np.abs(pb).sum(1)
    return {"cs": wf.sum(1), "B_cs": K * U * np.abs(wf).sum(1), "bf": bf, "B_bf": e_b + U * (np.abs(bf) + e_b),
            "csg": pg.sum(1), "B_csg": (K + 1) * U * np.abs(pg).sum(1)}


def l2_reference(x):
    """(want, B) of x / ||x||_2 per row; rows whose fp32 sum of squares overflows are expected as zeros (B = 0)"""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    q = (x * x).sum(1)
    over = q > FLT_MAX * (1 + (D + 2) * U)
    assert not np.any((q > FLT_MAX * (1 - (D + 2) * U)) & ~over), "a row's sum of squares sits on fp32's overflow threshold"
    want = x / np.sqrt(q)[:, None]
    rel = (D + 2) * U / 2 + D * 2.0 ** -150 / (2 * q) + SQRT + DIV + 2 * U
    B = np.abs(want) * rel[:, None]
    want[over], B[over] = 0.0, 0.0
    return want, B


def vae_loss_reference(recon, x, mean, logvar):
    """(want, B) of the scalar loss"""
    r, x, m, lv = (np.asarray(t, np.float64) for t in (recon, x, mean, logvar))
    R = r.shape[0]
    n = r.size
    d = r - x
    ex = np.exp(lv)
    t = d * d - 0.5 * (1.0 + lv - m * m - ex)
    e = U * (4 * d * d + 2 * np.abs(1 + lv) + 2 * m * m) + (EXP / 2 + U) * ex
    B = (n * U * (np.abs(t) + e).sum() + e.sum()) * (1 + DIV) / R + DIV * np.abs(t).sum() / R
    return t.sum() / R, B


def remainder_expected(x):
    """fp16((x - fp16(x)) 2048) as the kernel computes it: the subtraction and the scaling are exact in fp32"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        return ((x - x.astype(np.float16).astype(f32)) * f32(2048.0)).astype(np.float16)


def worst(got, want, B):
    """worst |err| / B over all elements (0 where the error is 0, inf where got is not finite)"""
    got = np.asarray(got, np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / B)
    return float(r.max()) if r.size else 0.0


def stats_ratios(x, mr, mu, x16, gamma=None):
    """rowstats_cast / layernorm_rowstats outputs against the float64 statistics of x: dict mean, rstd, copy"""
    s = row_stats_reference(x)
    want, B = copy_reference(x, mu, gamma)
    return {"mean": worst(mu, s["mean"], s["B_mean"]), "rstd": worst(mr[:, 1], s["rstd"], s["B_rstd"]), "copy": worst(x16, want, B)}


def family_stats_ratios(family, x, mr, mu, x16, gamma=None):
    """stats_ratios plus what the family promises bit for bit (check_special_rows).  `constant`: the any-order B_mean^2 / 1e-5 says nothing
    about rstd of a zero-variance row, so rstd's ratio is taken over the other rows and check_special_rows holds those rows to 15 u"""
    r = stats_ratios(x, mr, mu, x16, gamma)
    if family == "constant":
        keep = np.arange(x.shape[0]) % 3 != 0
        r["rstd"] = stats_ratios(x[keep], mr[keep], mu[keep], x16[keep], gamma)["rstd"] if keep.any() else 0.0
    check_special_rows(family, x, mu, mr[:, 1], x16 if gamma is None else None)
    return r


def finalize_ratios(stats, mu_in, gw, centred, mr, mu_out):
    r = finalize_reference(stats, mu_in, gw, centred)
    out = {"mr0": worst(mr[:, 0], r["mr0"], r["B_mr0"]), "rstd": worst(mr[:, 1], r["rstd"], r["B_rstd"])}
    if not centred:
        out["mean"] = worst(mu_out, r["mean"], r["B_mean"])
    return out


def fold_ratios(w16, gamma, beta, bias, got):
    r = fold_reference(w16, gamma, beta, bias, got["wf16"])
    out = {"cs": worst(got["cs"], r["cs"], r["B_cs"]), "bf": worst(got["bf"], r["bf"], r["B_bf"])}
    if got.get("csg") is not None:
        out["csg"] = worst(got["csg"], r["csg"], r["B_csg"])
    return out


def check_constant_layernorm(family, x, y, b):
    """`constant`: LayerNorm of a constant row is beta (fp16(beta) from the f16 kernel) bit for bit: d = 0 exactly"""
    if family == "constant":
        rows = np.arange(0, x.shape[0], 3)
        assert np.array_equal(y[rows], np.broadcast_to(b, y[rows].shape)), "LayerNorm of a constant row is beta"


def check_special_rows(family, x, mu, rstd, copy):
    """the bit-for-bit expectations of `constant` and `exact` on the statistics and on the copy (None: a copy scaled by gamma, not checked)"""
    M = x.shape[0]
    if family == "constant":
        rows = np.arange(0, M, 3)
        assert np.array_equal(mu[rows], x[rows, 0]), "the mean of a constant row is the constant"
        assert np.all(np.abs(rstd[rows].astype(np.float64) - RSTD0) <= 15 * U * RSTD0), "rstd of a zero-variance row: 1 / sqrt(1e-5f)"
        if copy is not None:
            assert not np.any(copy[rows]), "the centred copy of a constant row is exactly 0"
    if family == "exact":
        assert np.array_equal(mu, x.astype(np.float64).mean(1).astype(f32)), "mu == c"
        if copy is not None:
            assert np.array_equal(copy, x - mu[:, None]), "every d is exact"


# ---- the layout of the lo half of a hi / lo stream (copy_rows_hilo) -----------------------------------------------------------------------
def lo_fragment_order(lo_bytes):
    """lo_bytes [R, D] uint8 in matrix order (R % 128 == 0, D % 256 == 0) -> the flat buffer in gemm_ring2's tile-fragment order, as the
    comments of hg_kernels.h / hg_elem.hip state it: tiles of 128 x 256, row-major over the tiles; inside a tile 8 waves x 8 pieces x 64
    lanes x 8 bytes with wave = ((row % 64) / 32, (col % 128) / 32), piece = (row / 64 % 2, col / 128 % 2, col / 16 % 2), lane = ((col % 16) / 4, row % 16),
    byte = ((row % 32) / 16, col % 4).  Written as a reshape and one transpose: each row / column digit is named once."""
    R, D = lo_bytes.shape
    assert R % 128 == 0 and D % 256 == 0
    #            row digits: tile, /64, /32, /16, %16        column digits: tile, /128, /32 (of 128), /16, /4 (of 16), %4
    v = lo_bytes.reshape(R // 128, 2, 2, 2, 16, D // 256, 2, 4, 2, 4, 4)
    names = ("rt", "r64", "r32", "r16", "r1", "ct", "c128", "c32", "c16", "c4", "c1")
    order = ("rt", "ct", "r32", "c32", "r64", "c128", "c16", "c4", "r1", "r16", "c1")      # tile, wave, piece, lane, byte
    return np.ascontiguousarray(v.transpose([names.index(n) for n in order])).reshape(-1)


# ---- fp32 restatement of the arithmetic kernels, with mutants ------------------------------------------------------------------------------
def _to_f16(v, mutant=None):
    """fp32 -> fp16 (RNE, subnormals kept) -> fp32"""
    with np.errstate(all="ignore"):
        h = v.astype(np.float16)
        if mutant == "f16_truncate":
            bits = h.view(np.uint16)
            over = np.abs(h.astype(f32)) > np.abs(v)
            h = np.where(over, bits - 1, bits).astype(np.uint16).view(np.float16)      # one step towards zero
        if mutant == "f16_flush":
            h = np.where(np.abs(h) < 2.0 ** -14, np.float16(0), h)
        return h.astype(f32)


def _wave_sum(part):
    """[M, 64] lane partials -> [M]: the xor butterfly of wave_sum (hg_common.h)"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ o]
    return part[:, 0]


def _lanes(x):
    """x [M, D] -> [M, I, 64, 4] (chunk c = lane + 64 i; missing chunks are zero, which adds nothing)"""
    M, D = x.shape
    nc = D // 4
    I = (nc + 63) // 64
    v = np.zeros((M, I * 64, 4), f32)
    v[:, :nc] = x.reshape(M, nc, 4)
    return v.reshape(M, I, 64, 4)


def _row_stats32(x, mutant=None):
    """(mean, rstd, d) fp32 in the kernels' order: per-lane chunk sums, butterfly, second pass over x - mean"""
    D = x.shape[1]
    Df = f32(D)
    with np.errstate(all="ignore"):
        v = _lanes(x)
        s = np.zeros((x.shape[0], 64), f32)
        for i in range(v.shape[1]):
            s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        mean = _wave_sum(s) / Df
        d = x - mean[:, None]
        dl = _lanes(d)
        sq = _lanes(x) if mutant == "var_naive" else dl
        q = np.zeros((x.shape[0], 64), f32)
        for i in range(v.shape[1]):
            for e in range(4):
                q = q + sq[:, i, :, e] * sq[:, i, :, e]
        q = _wave_sum(q)
        var = q / (Df - f32(1) if mutant == "unbiased" else Df)
        if mutant == "var_naive":
            var = np.maximum(var - mean * mean, f32(0))
        rstd = f32(1) / np.sqrt(var + (f32(0) if mutant == "no_eps" else f32(1e-5)))
    return mean, rstd.astype(f32), d


def model_layernorm(x, w, b, f16, mutant=None):
    """layernorm_kernel: out [M, D] fp32 (fp16 values widened when f16)"""
    mean, rstd, d = _row_stats32(x, mutant)
    with np.errstate(all="ignore"):
        y = d * rstd[:, None] * w[None] + b[None]
    return _to_f16(y, mutant) if f16 else y


def model_rowstats(x, gamma=None, mutant=None):
    """rowstats_cast_kernel: dict x16 (fp16 values as fp32), mr [M, 2], mu, muc"""
    mean, rstd, d = _row_stats32(x, mutant)
    with np.errstate(all="ignore"):
        c = x if mutant == "copy_uncentred" else d
        x16 = _to_f16(c * gamma[None] if gamma is not None else c, mutant)
    return {"x16": x16, "mr": np.stack([np.zeros_like(mean), rstd], 1), "mu": mean, "muc": mean.copy()}


def model_finalize(stats, mu, gw, centred, order="loop", mutant=None):
    """finalize_stats_row: dict mr [M, 2], mu, muc.  order "loop": load, add, load, add; "nt12": the hand-unrolled path of nt == 12 (the
    same additions written over six 4-vectors; the division by gw and the Chan term evaluated per vector half)"""
    st = np.asarray(stats, f32)
    M, nt, _ = st.shape
    Df, gwf = f32(nt * gw), f32(gw)
    with np.errstate(all="ignore"):
        s1 = np.zeros(M, f32)
        m2 = np.zeros(M, f32)
        if order == "nt12":
            assert nt == 12
            v = st.reshape(M, 6, 4)
            for i in range(6):
                s1 = s1 + v[:, i, 0]
                s1 = s1 + v[:, i, 2]
            mean = s1 / Df
            for i in range(6):
                for h in (0, 2):
                    d0 = v[:, i, h] / gwf - mean
                    m2 = m2 + (v[:, i, h + 1] + (f32(0) if mutant == "chan_no_cross" else gwf * d0 * d0))
        else:
            for t in range(nt):
                s1 = s1 + st[:, t, 0]
            mean = s1 / Df
            for t in range(nt):
                d0 = st[:, t, 0] / gwf - mean
                m2 = m2 + (st[:, t, 1] + (f32(0) if mutant == "chan_no_cross" else gwf * d0 * d0))
        rstd = f32(1) / np.sqrt(m2 / Df + (f32(0) if mutant == "no_eps" else f32(1e-5)))
        mr0 = mean if centred else (mu - mean if mutant == "mr0_sign" else mean - mu)
    return {"mr": np.stack([mr0, rstd], 1).astype(f32), "mu": mu.copy() if centred else mean, "muc": mu.copy()}


def model_fold(w16, gamma, beta, bias, mutant=None):
    """fold_ln_kernel: dict wf16 (float16), cs, bf, csg [N] fp32; lane k % 64 owns column k, butterfly over the lanes"""
    N, K = w16.shape
    w = w16.astype(f32)
    I = (K + 63) // 64
    with np.errstate(all="ignore"):
        pg = w * gamma[None]
        wf16 = pg.astype(np.float16)
        if mutant == "f16_truncate":
            wf16 = _to_f16(pg, mutant).astype(np.float16)
        terms = {"cs": pg if mutant == "cs_unrounded" else wf16.astype(f32), "bf": w * beta[None], "csg": pg}
        out = {"wf16": wf16}
        for k, t in terms.items():
            p = np.zeros((N, I * 64), f32)
            p[:, :K] = t
            p = p.reshape(N, I, 64)
            acc = np.zeros((N, 64), f32)
            for i in range(I):
                acc = acc + p[:, i]
            out[k] = _wave_sum(acc)
        out["bf"] = (bias if bias is not None else np.zeros(N, f32)) + out["bf"]
    return out
