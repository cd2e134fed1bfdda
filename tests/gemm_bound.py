"""What the GEMM kernels (hg_gemm.hip, hg_gemm_ring*.hip, hg_gemm_ring*_body.h, hg_gemm_duo.hip, the epilogues of hg_gemm_dev.h) are held
to: the epilogue's expression evaluated in float64 on the CPU from the fp16-rounded operands, and a bound PER OUTPUT ELEMENT that is the
sum of the worst case of each rounding the kernel performs.  A plain module beside the tests (tests/test_gemm_rounding_model.py,
tests/test_gpu_gemm.py import it): no fixtures, no GPU, no library.

For the output element (m, n), all float64, u = 2^-24:

    acc = sum_k a_mk w_nk          S = sum_k |a_mk| |w_nk|          want = the epilogue's expression of acc

    B = K 2^-23 S                  fp32 accumulation of K exact products (an fp16 x fp16 product has 22 bits).  The classical worst case of
                                   a sum of K terms in ANY order is (K - 1) u' S; u' = 2^-23, not 2^-24, so that the bound does not depend on
                                   whether the matrix unit's internal adds round to nearest or truncate.  This is a worst case that can be
                                   proved, not a measurement.
      + u |term| per fp32 operation of the epilogue, counted from the source (a fused multiply-add rounds once where two operations
                                   are counted: the bound covers both code shapes):
            bias add               u |acc + b|                                            (absent without a bias)
            LayerNorm fold 8 / 9   (acc - cs mean) rstd + b' (hg_gemm_ring_body.h): u |cs mean| and u |acc - cs mean| in front of the rstd
                                   multiply (both times rstd), u |(acc - cs mean) rstd| for it, u |want| for the bias add
            residual add 3, 7, 10, 12      u |x0 + v|
            scale multiply 7, 12   u |(acc + b) scale|, the error of acc + b times |scale|
            positional add 5       u |acc + b + pos|
            epilogue 11            fmaf(mu, cs, acc): u |acc + mu cs|, and u |mu cs| for the caller's fp32 rounding of cs (the expectation
                                   is relu(W (x16 + mu) + b) with the exact column sums)
      + QuickGELU g = v / (1 + 2^(k v)), k = -1.702 log2(e) held as fp32:  1.1 x (the error of v; sup |g'| = 1.0998) + rho |g|,
            rho = (2 u |k v| ln 2 + 2^-23) e / (1 + e) + 2^-23 + 2 u,   e = 2^(k v):
                                   the rounding of k v and of k move the exponential by |k v| ln 2 u each, the hardware exp2 by 1 ulp (2^-23),
                                   both reach the denominator 1 + e scaled by e / (1 + e); the add rounds once (u), the hardware reciprocal
                                   is 1 ulp, the last multiply rounds once (u).  The 1 ulp of v_exp_f32 / v_rcp_f32 is ASSUMED: the kernel
                                   guides do not state it.  Every QuickGELU epilogue ends in fp16, so this term only has to be right, not
                                   tight.
      + fp16 output (0, 1, 2, 8, 9, the centred copy of 10 / 12): with t = |want| + the fp32 terms above, 2^-11 t for a normal result,
                                   2^-25 absolute where t < 2^-14 (a subnormal: step 2^-24).  A deliberate deviation from the plain
                                   2^-11 |want|: what is rounded is the computed value, which may lie the fp32 terms away from want (and
                                   on the other side of 2^-14 or of a power of two), so only t makes the sum a worst case.  It is larger
                                   than 2^-11 |want| by 2^-11 times the fp32 terms, below 1e-3 of B; the mutant tests (truncation,
                                   flushed subnormals) pass unchanged with it.

Rule: every element has |got - want| <= B.  No global scale, no row norm, no element left out.

Row statistics of the residual epilogues 10 / 12 are judged apart from the stream: against float64 statistics (two-pass variance) of the
stream the kernel itself RETURNED (x as fp32, D columns, G = D / 64 groups).  The kernels keep per 64-column group (sum, M2 about the group
mean) and finalize_stats_row (hg_gemm_dev.h) combines them with Chan's formula.  Derived, not calibrated:

    mean       a group sum of 64 fp32 values in any order is off by <= 63 u A_g (A_g = the group's sum of |x|), the sum of the G group sums
               by <= (G - 1) u sum_g A_g, the division rounds once:       B_mean = (64 + G) u sum_j |x_mj| / D.
               mr_out[:, 0] = fl(mean - mu): + u |mean - mu|.
    rstd       M2^ = sum_g [sum_j (x_j - g^)^2 + 64 (g^ - m^)^2] with perturbed group means g^ = g + dg (|dg| <= 63 u A_g / 64) and mean
               m^ = m + dm: in exact arithmetic M2^ - M2 = 128 sum_g (g^ - m^) (g - g^) + D dm^2 - 64 sum_g dg^2; every term of the sums is
               >= 0 and carries a relative (2 + 64) u (group) resp. 4 u (Chan term), the 2 G additions 2 G u, / D, + 1e-5f, sqrt, 1 / .:
               E_M2 = (70 + 2 G) u M2 + 126 u sum_g (|g - m| + |dg| + |dm|) A_g + 64 sum_g dg^2 + D dm^2,
               B_rstd = rstd (E_M2 / (2 (M2 + 1e-5 D)) + 5 u).
    copy       fp16(fl(x - mu)) of the returned x: one fp32 subtraction and one fp16 rounding, u |x - mu| + the fp16 term.  The copy scaled by
               the next LayerNorm's weight (GemmArgs::gamma), fp16(fl(fl(x - mu) gamma)): 2 u |(x - mu) gamma| + the fp16 term.

`model()` is the CPU restatement of a tile's arithmetic: fp32 accumulation K-tile by K-tile (64 wide, the kernels' K order; torch's fp32
matmul inside a K-tile), the epilogue in fp32 in the source's operation order, RNE to fp16, the per-group (sum, M2) and finalize_stats_row;
vectorised over the output, with the mutants that tests/test_gemm_rounding_model.py proves the bound catches.

Input families (`make_case`; seeded, generated on the CPU, a and w always fp16 numbers):

    exact      a, w uniform integers in [-16, 16] / 8, bias integers 2^-10 in [-1, 1], x0 and pos on the same grid, scale integers / 4 in
               [-1, 1]: every product and partial sum is exact in fp32 in any order, so fp32 outputs (3, 4, 5, 6, 7) are expected bit for
               bit and fp16 outputs (0, 2) as the float64 result rounded once, where fp16's spacing is up to 0.25
    tiny       integers in [-16, 16] x 2^-11 for both operands, bias integers 2^-22: still exact; about an eighth of the outputs are
               non-zero fp16 subnormals
    randn      a ~ randn, w ~ randn K^-0.5, bias 0.1 randn
    outlier    randn with every 97th column of a times 67 and every 89th row of w times 30
    cancel     a equal on the column pairs (k, k + K / 2), w of opposite signs there, plus 2^-6 randn: |acc| << S
    lnfold     (8 / 9) randn operands; mr[:, 0] = 0.02 randn in two thirds of the rows, 3 randn in the rest; rstd log-uniform in [0.05, 300]
    offset     (10 / 12) x0 = 100 + 0.5 randn: E[x^2] - mean^2 in fp32 is off by 1e-2 relative
    constant   (10 / 12) every third row has x0 constant (an integer / 4, about 100 randn) and a = 0, bias = 0: the update is zero, every
               partial sum of the row is exact, the variance exactly zero and rstd = 1 / sqrt(1e-5) to the last few bits
    wide       (10 / 12) x0 = 2 randn + 8 randn per row, every 97th column times 30

Worst |err| / B over all elements, `model()` / kernels: `model()` at the eight shapes of tests/test_gemm_rounding_model.py, with and
without bias; the kernels as tests/test_gpu_gemm.py prints it (lines starting GEMM_RATIO) on an MI355X, worst over its shapes and over
the kernels that have the epilogue (0 - 6: simple = ring = ring2 = duo bit for bit; 8, 9: ring; 10: ring2 and duo; 12: duo; 5, 7, 11
through hg_test_gemm_ex).  `outlier` and `cancel` run on the GPU at M = 641 and 2048 x 768 x 768 only, the model also at K = 64, 128.

    epilogue  exact           tiny            randn           outlier         cancel          lnfold          offset          constant        wide
    0 out     0.968 / 0.968   0.967 / 0.967   0.948 / 0.948   0.972 / 0.915   0.787 / 0.312   -               -               -               -
    1 out     0.954 / 0.954   0.859 / 0.859   0.909 / 0.909   0.960 / 0.908   0.614 / 0.177   -               -               -               -
    2 out     0.958 / 0.958   0.963 / 0.963   0.936 / 0.936   0.962 / 0.915   0.787 / 0.300   -               -               -               -
    3 out     0     / 0       0     / 0       0.025 / 0.020   0.088 / 0.012   0.023 / 0.002   -               -               -               -
    4 out     0     / 0       0     / 0       0.027 / 0.010   0.088 / 0.011   0.022 / 0.002   -               -               -               -
    5 out     -     / 0       -               -     / 0.004   -               -               -               -               -               -
    6 out     0     / 0       0     / 0       0.027 / 0.009   0.088 / 0.011   0.022 / 0.002   -               -               -               -
    7 out     0     / 0       0     / -       0.868 / 0.841   0.708 / -       0.887 / -       -               -               -               -
    8 out     0.891 / 0.839   0.993 / 0.993   0.911 / 0.866   0.948 / 0.915   0.639 / 0.449   0.968 / 0.948   -               -               -
    9 out     0.863 / 0.806   0.988 / 0.991   0.905 / 0.833   0.942 / 0.897   0.545 / 0.268   0.965 / 0.938   -               -               -
    10 out    0     / 0       0     / 0       0.010 / 0.005   0.037 / 0.012   0.011 / 0.002   -               0.050 / 0.017   0.009 / 0.004   0.211 / 0.100
    10 copy   0.999 / 0.999   0.999 / 0.999   1.000 / 1.000   0.999 / 1.000   1.000 / 1.000   -               0.999 / 0.999   1.000 / 1.000   1.000 / 1.000
    10 mean   0.001 / 0.001   0.001 / 0.001   0.034 / 0.037   0.024 / 0.024   0.028 / 0.040   -               0.044 / 0.050   0.023 / 0.036   0.041 / 0.055
    10 mr0    0.002 / 0.002   0.002 / 0.002   0.034 / 0.037   0.024 / 0.024   0.028 / 0.040   -               0.044 / 0.050   0.023 / 0.036   0.041 / 0.055
    10 rstd   0.053 / 0.055   0.347 / 0.361   0.047 / 0.052   0.057 / 0.075   0.048 / 0.053   -               0.028 / 0.089   0.182 / 0.182   0.068 / 0.090
    11 out    0     / 0       0     / -       0.026 / 0.001   0.083 / -       0.021 / -       -               -               -               -
    12 out    0     / 0       0     / 0       0.636 / 0.878   0.708 / 0.238   0.767 / 0.548   -               0.633 / 0.634   0.769 / 0.539   0.889 / 0.960
    12 copy   0.999 / 0.999   0.999 / 0.999   1.000 / 1.000   1.000 / 1.000   1.000 / 1.000   -               0.999 / 0.999   0.999 / 1.000   0.999 / 1.000
    12 mean   0.001 / 0.002   0.001 / 0.001   0.035 / 0.042   0.030 / 0.026   0.035 / 0.038   -               0.041 / 0.044   0.029 / 0.033   0.043 / 0.052
    12 mr0    0.003 / 0.003   0.003 / 0.003   0.035 / 0.042   0.030 / 0.028   0.035 / 0.038   -               0.041 / 0.044   0.029 / 0.033   0.043 / 0.052
    12 rstd   0.049 / 0.056   0.362 / 0.367   0.051 / 0.055   0.064 / 0.073   0.052 / 0.049   -               0.024 / 0.020   0.182 / 0.182   0.062 / 0.089

The gamma-scaled copy of gemm_ring2 (hg_test_gemm_ex; 641 x 256 x 256 and 769 x 768 x 320, `exact` and `randn`): against
fp16((x - mu) gamma) of the returned stream 0.999 (hl 0) and 0.999 (hl 3), against the hi half it is written beside 0.960 (hl 1, 2); the
first hi half against float64 0.896.

No entry is above 1 (1.000 is 0.9995 or more, rounded; the tests assert <= 1).  fp16 outputs (0, 1, 2, 8, 9) reach 0.97 - 0.99 at K = 64 .. 256,
where the fp16 rounding is nearly all of B: a result just above a power of two, where half an fp16 ulp IS 2^-11 |want|; on `exact` and
`tiny` the kernels land on the model to the digit, because there is nothing but that rounding.  The centred copy sits at 1.000 for the
same reason (one fp16 rounding is all it is allowed).  The fp32 outputs (3, 4, 5, 6, 10, 11) stay below 0.1 (0.21 in the model on `wide`): the
accumulation term K 2^-23 S is what makes B loose there - a worst case over every summation order and over truncating adds, where the
matrix unit's error grows like sqrt(K) u; at K = 3072 it is ten times the fp16 term, and what B cannot see there (a truncated fp16
conversion, say) the bit-for-bit expectation of `exact` does.  7 and 12 reach 0.96 where scale[n] is small: the residual add's single
rounding, u |x|, is then nearly all of B.  mean stays below 0.06 and rstd below 0.1 on real-valued rows: (64 + G) u sum |x| / D is a worst
case for a sum of 64 + G terms whose error grows like its square root; `tiny` rows (0.36) and the zero-variance rows of `constant` (0.18)
leave rstd little but the 5 u of its last four operations.
"""
import functools
import math

import torch

U = 2.0 ** -24
FAMILIES = ("exact", "tiny", "randn", "outlier", "cancel")
LN_FAMILIES = ("lnfold",)
RESID_FAMILIES = ("offset", "constant", "wide")
MUTANTS = ("bias_shift4", "drop_last_k", "f16_partials", "gelu_1p7", "f16_truncate", "f16_flush", "rstd_after_bias", "mean_uncentred",
           "var_naive", "copy_new_mean", "relu_split_swapped", "patch_no_cls")
F16_EPIS = (0, 1, 2, 8, 9)
STATS_EPIS = (10, 12)
K_GELU = torch.tensor(-2.4554669595930157, dtype=torch.float32)      # the kernels' -1.702 log2(e), as fp32
EPS = 1e-5

def seed_of(family, M, N, K):
    fams = FAMILIES + LN_FAMILIES + RESID_FAMILIES
    return ((fams.index(family) * 100003 + M) * 8209 + N) * 4099 + K


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=3)
def make_case(family, M, N, K, rows_out=0):
    """Operands of one launch, float32 on the CPU: a [M, K], w [N, K] (fp16 numbers), bias [N], x0 [max(M, rows_out), N] (the buffer a
    residual / patch epilogue updates), scale [N], pos [rows_out or M, N], mu [M], mr [M, 2], cs [N] (fp32 of the exact column sums of w);
    and float64 acc, S [M, N], cs64 [N].  Cached: the epilogues and kernels of a test share it and must leave it unchanged."""
    g = torch.Generator().manual_seed(seed_of(family, M, N, K))
    R = max(M, rows_out)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    if family == "exact":
        a, w = _ints(g, -16, 16, M, K) / 8, _ints(g, -16, 16, N, K) / 8
        bias, x0, pos = _ints(g, -1024, 1024, N) / 1024, _ints(g, -1024, 1024, R, N) / 1024, _ints(g, -1024, 1024, R, N) / 1024
        scale = _ints(g, -4, 4, N) / 4
        mu = _ints(g, -64, 64, M) / 64
    elif family == "tiny":
        a, w = _ints(g, -16, 16, M, K) * 2.0 ** -11, _ints(g, -16, 16, N, K) * 2.0 ** -11
        bias, x0, pos = _ints(g, -64, 64, N) * 2.0 ** -22, _ints(g, -64, 64, R, N) * 2.0 ** -22, _ints(g, -64, 64, R, N) * 2.0 ** -22
        scale = _ints(g, -4, 4, N) / 4
        mu = _ints(g, -64, 64, M) * 2.0 ** -22
    else:
        a, w, bias = rn(M, K), rn(N, K) * K ** -0.5, 0.1 * rn(N)
        if family == "outlier":
            a[:, 5::97] *= 67.0
            w[3::89] *= 30.0
        elif family == "cancel":
            h = K // 2
            a[:, h:2 * h] = a[:, :h]
            w[:, h:2 * h] = -w[:, :h]
            a, w = a + 2.0 ** -6 * rn(M, K), w + 2.0 ** -6 * K ** -0.5 * rn(N, K)
        x0 = 2 * rn(R, N) + rn(R, 1)
        if family == "offset":
            x0 = 100.0 + 0.5 * rn(R, N)
        elif family == "wide":
            x0 = 2 * rn(R, N) + 8 * rn(R, 1)
            x0[:, 5::97] *= 30.0
        elif family == "constant":
            x0[::3] = (torch.round(400.0 * rn(R, 1)) / 4)[::3]      # few bits: the sums of such a row are exact in fp32
            a[::3] = 0.0
            bias = 0.0 * bias
        pos, scale = 0.3 * rn(R, N), 0.5 * rn(N)
        mu = x0[:M].mean(1) + 0.05 * rn(M)
    mean = 0.3 * rn(M)
    rstd = 0.5 + 1.5 * torch.rand(M, generator=g, dtype=torch.float64)
    if family == "lnfold":
        mean = torch.where(torch.arange(M) % 3 == 2, 3.0 * rn(M), 0.02 * rn(M))
        rstd = torch.exp(math.log(0.05) + (math.log(300.0) - math.log(0.05)) * torch.rand(M, generator=g, dtype=torch.float64))
    a, w = a.half().double(), w.half().double()
    c = {"family": family, "M": M, "N": N, "K": K, "a": a.float(), "w": w.float(), "bias": bias.float(), "x0": x0.float().contiguous(),
         "scale": scale.float(), "pos": pos.float().contiguous(), "mu": mu.float(), "mr": torch.stack([mean, rstd], 1).float().contiguous(),
         "acc": a @ w.t(), "S": a.abs() @ w.abs().t(), "cs64": w.sum(1)}
    c["cs"] = c["cs64"].float()
    return c


# ---- the float64 reference and the bound ------------------------------------------------------------------------------------------
def f16_term(t):
    """worst case of one RNE rounding to fp16 of a computed value of magnitude <= t"""
    return torch.where(t < 2.0 ** -14, torch.full_like(t, 2.0 ** -25), 2.0 ** -11 * t)


def quick_gelu64(v):
    t = (K_GELU.double() * v).clamp(-1000.0, 1000.0)
    return v / (1.0 + torch.exp2(t))


def reference(c, epi, bias=True, n_split=0, G=0, L=0, pos=True):
    """(want, B) of epilogue `epi` on case c, float64 [M, N] ([rows_out, N] for epilogue 5: class rows want x0 with B = 0).  For 10 / 12
    the stream only (statistics and copy: stats_reference)."""
    acc, S, K = c["acc"], c["S"], c["K"]
    M = c["M"]
    e_acc = K * 2.0 ** -23 * S
    b = c["bias"].double()[None] if bias else None
    x0 = c["x0"].double()

    def add_bias(v, e):
        if b is None:
            return v, e
        return v + b, e + U * (v + b).abs()

    if epi in (8, 9):
        mean, rstd = c["mr"].double()[:, :1], c["mr"].double()[:, 1:]
        cm = c["cs"].double()[None] * mean
        t = (acc - cm) * rstd
        e = rstd * (e_acc + U * cm.abs() + U * (acc - cm).abs()) + U * t.abs()
        v, e = add_bias(t, e)
    elif epi == 11:
        mc = c["mu"].double()[:, None] * c["cs64"][None]
        v, e = add_bias(acc + mc, e_acc + U * (acc + mc).abs() + U * mc.abs())
    else:
        v, e = add_bias(acc, e_acc)
    if epi in (1, 9):
        kv = K_GELU.double() * v
        sig = 1.0 / (1.0 + torch.exp2(kv.clamp(-1000.0, 1000.0)))
        g = v * sig
        rho = (2 * U * kv.abs() * math.log(2.0) + 2.0 ** -23) * (1.0 - sig) + 2.0 ** -23 + 2 * U
        v, e = g, 1.1 * e + rho * g.abs()
    if epi in (2, 6):
        v = v.clamp_min(0.0)
    if epi == 11:
        lin = torch.arange(c["N"]) >= n_split if n_split else torch.zeros(c["N"], dtype=torch.bool)
        v = torch.where(lin[None], v, v.clamp_min(0.0))
    if epi in (7, 12):
        sc = c["scale"].double()[None]
        v, e = v * sc, e * sc.abs() + U * (v * sc).abs()
    if epi in (3, 7, 10, 12):
        v = x0[:M] + v
        e = e + U * v.abs()
    if epi == 5:
        if pos:
            t = torch.arange(M) % G
            v = v + c["pos"].double()[1 + t]
            e = e + U * v.abs()
        want, B = x0.clone(), torch.zeros_like(x0)
        rows = (torch.arange(M) // G) * L + 1 + torch.arange(M) % G
        want[rows], B[rows] = v, e
        return want, B
    if epi in F16_EPIS:
        e = e + f16_term(v.abs() + e)
    return v, e


def stats_reference(x, mu):
    """float64 statistics of the returned stream x [M, D] and the bounds of the module docstring: dict of mean, rstd, copy (want),
    B_mean, B_mr0, B_rstd, B_copy"""
    x = x.detach().cpu().double()
    mu = mu.detach().cpu().double()
    M, D = x.shape
    G = D // 64
    mean = x.mean(1)
    dev = x - mean[:, None]
    M2 = (dev * dev).sum(1)
    rstd = 1.0 / torch.sqrt(M2 / D + EPS)
    A = x.abs().view(M, G, 64).sum(2)
    gmean = x.view(M, G, 64).mean(2)
    B_mean = (64 + G) * U * A.sum(1) / D
    dg = 63 * U * A / 64
    e_m2 = ((70 + 2 * G) * U * M2 + 126 * U * (((gmean - mean[:, None]).abs() + dg + B_mean[:, None]) * A).sum(1)
            + 64 * (dg * dg).sum(1) + D * B_mean * B_mean)
    d = x - mu[:, None]
    return {"mean": mean, "rstd": rstd, "copy": d, "B_mean": B_mean, "B_mr0": B_mean + U * (mean - mu).abs(),
            "B_rstd": rstd * (e_m2 / (2 * (M2 + EPS * D)) + 5 * U), "B_copy": U * d.abs() + f16_term(d.abs() * (1 + U))}


def scaled_copy_reference(d, gamma):
    """fp16(fl(fl(x - mu) gamma)) (GemmArgs::gamma) from d = x - mu in float64: (want, B) - the two fp32 operations and one fp16 rounding"""
    want = d * gamma.double()[None]
    return want, 2 * U * want.abs() + f16_term(want.abs() * (1 + 2 * U))


def _worst(got, want, B):
    got = got.detach().cpu().double()
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / B)
    return float(r.max()) if bool(torch.isfinite(got).all()) else float("inf")


def ratios(c, epi, out, **kw):
    """Worst |err| / B per checked quantity of one launch's outputs: out = {"out": [M, N]} and, for 10 / 12, "out2", "mr_out", "mu_out"
    too.  Keys: out; mean, mr0, rstd, copy."""
    want, B = reference(c, epi, **kw)
    r = {"out": _worst(out["out"], want, B)}
    if epi in STATS_EPIS:
        s = stats_reference(out["out"], c["mu"])
        mu = c["mu"].double()
        r["mean"] = _worst(out["mu_out"], s["mean"], s["B_mean"])
        r["mr0"] = _worst(out["mr_out"][:, 0].detach().cpu().double() + mu, s["mean"], s["B_mr0"])
        r["rstd"] = _worst(out["mr_out"][:, 1], s["rstd"], s["B_rstd"])
        r["copy"] = _worst(out["out2"], s["copy"], s["B_copy"])
    return r


def exact_expected(c, epi, **kw):
    """`exact` / `tiny`: the float64 result, rounded once to fp16 for the fp16 epilogues, as float32 - what torch.equal is asked for"""
    want, _ = reference(c, epi, **kw)
    assert bool((want.float().double() == want).all()), "the family is not exact in fp32 at this shape"
    return want.half().float() if epi in F16_EPIS else want.float()


# ---- the CPU restatement of a tile's arithmetic ------------------------------------------------------------------------------------
def _to_f16(v, mutant):
    """fp32 -> fp16 -> fp32 as the kernels' v_cvt_pk_f16_f32 (RNE, subnormals kept)"""
    h = v.half()
    if mutant == "f16_truncate":
        bits = h.view(torch.int16).int()
        over = h.float().abs() > v.abs()
        h = torch.where(over, bits - 1, bits).short().view(torch.float16)      # one step towards zero (sign bit untouched)
    if mutant == "f16_flush":
        h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
    return h.float()


def _gelu32(v, k):
    t = v * k
    e = torch.exp2(t.double()).float()
    r = (1.0 / (1.0 + e).double()).float()
    return v * r


def finalize_stats(sums, m2s, mu, mutant=None):
    """finalize_stats_row: sums, m2s [M, G] fp32 per 64-column group -> (mr0, rstd, mean) fp32"""
    M, G = sums.shape
    D = torch.tensor(float(G * 64), dtype=torch.float32)
    gw = torch.tensor(64.0, dtype=torch.float32)
    s1 = torch.zeros(M, dtype=torch.float32)
    for t in range(G):
        s1 = s1 + sums[:, t]
    mean = s1 / D
    m2 = torch.zeros(M, dtype=torch.float32)
    for t in range(G):
        d0 = sums[:, t] / gw - mean
        m2 = m2 + (m2s[:, t] + gw * d0 * d0)
    rstd = 1.0 / torch.sqrt(m2 / D + torch.tensor(EPS, dtype=torch.float32))
    return (mean.clone() if mutant == "mean_uncentred" else mean - mu), rstd, mean


def model(c, epi, mutant=None, bias=True, n_split=0, G=0, L=0, pos=True):
    """The kernels' arithmetic on the CPU -> {"out"} (+ "out2", "mr_out", "mu_out" for 10 / 12), float32; fp16 outputs as the hooks
    return them (widened).  mutant: one of MUTANTS -
      bias_shift4         the bias is read four columns to the right
      drop_last_k         the last k element is left out
      f16_partials        the partial sums are rounded to fp16 once per K-tile
      gelu_1p7            QuickGELU with 1.7 for 1.702
      f16_truncate        fp16 outputs truncated instead of rounded to nearest even
      f16_flush           fp16 subnormal outputs flushed to zero
      rstd_after_bias     8 / 9: ((acc - cs mean) + b') rstd
      mean_uncentred      10 / 12: mr_out[:, 0] = mean where mean - mu belongs
      var_naive           10 / 12: variance as E[x^2] - mean^2 in fp32
      copy_new_mean       10 / 12: the fp16 copy centred on the new mean instead of mu
      relu_split_swapped  11: no ReLU on the columns below n_split, ReLU on those above
      patch_no_cls        5: output row b L + t, without the + 1 for the class token"""
    assert mutant is None or mutant in MUTANTS, mutant
    a, w, M, N, K = c["a"], c["w"], c["M"], c["N"], c["K"]
    if mutant == "drop_last_k":
        a = a.clone()
        a[:, K - 1] = 0.0
    acc = torch.zeros(M, N, dtype=torch.float32)
    for k0 in range(0, K, 64):
        acc = acc + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
        if mutant == "f16_partials":
            acc = acc.half().float()
    b = c["bias"] if bias else None
    if b is not None and mutant == "bias_shift4":
        b = torch.roll(b, -4)
    k = torch.tensor(-1.7 * 1.4426950408889634, dtype=torch.float32) if mutant == "gelu_1p7" else K_GELU
    if epi in (8, 9):
        mean, rstd = c["mr"][:, :1], c["mr"][:, 1:]
        v = acc - c["cs"][None] * mean
        if mutant == "rstd_after_bias":
            v = (v + b) * rstd if b is not None else v * rstd
        else:
            v = v * rstd
            v = v + b if b is not None else v
    elif epi == 11:
        v = (c["mu"].double()[:, None] * c["cs"].double()[None] + acc.double()).float()      # fmaf
        v = v + b if b is not None else v
    else:
        v = acc + b[None] if b is not None else acc
    if epi in (1, 9):
        v = _gelu32(v, k)
    if epi in (2, 6):
        v = v.clamp_min(0.0)
    if epi == 11:
        lin = torch.arange(N) >= n_split if n_split else torch.zeros(N, dtype=torch.bool)
        if mutant == "relu_split_swapped" and n_split:
            lin = ~lin
        v = torch.where(lin[None], v, v.clamp_min(0.0))
    if epi == 7:          # one fused multiply-add in every kernel (fma4, hg_common.h)
        v = (c["x0"][:M].double() + v.double() * c["scale"].double()[None]).float()
    if epi == 12:
        v = v * c["scale"][None]
    if epi in (3, 10, 12):
        v = c["x0"][:M] + v
    if epi == 5:
        t = torch.arange(M) % G
        if pos:
            v = v + c["pos"][1 + t]
        out = c["x0"].clone()
        out[(torch.arange(M) // G) * L + (0 if mutant == "patch_no_cls" else 1) + t] = v
        return {"out": out}
    if epi in F16_EPIS:
        v = _to_f16(v, mutant)
    if epi not in STATS_EPIS:
        return {"out": v}
    mu = c["mu"]
    xg = v.view(M, N // 64, 64)
    sums = xg.sum(2)
    gm = sums * torch.tensor(1.0 / 64.0, dtype=torch.float32)
    d = xg - gm[:, :, None]
    m2s = (d * d).sum(2)
    mr0, rstd, mean = finalize_stats(sums, m2s, mu, mutant)
    if mutant == "var_naive":
        D = torch.tensor(float(N), dtype=torch.float32)
        rstd = 1.0 / torch.sqrt(((v * v).sum(1) / D - mean * mean).clamp_min(0.0) + torch.tensor(EPS, dtype=torch.float32))
    centre = mean if mutant == "copy_new_mean" else mu
    return {"out": v, "out2": _to_f16(v - centre[:, None], mutant), "mr_out": torch.stack([mr0, rstd], 1), "mu_out": mean}
