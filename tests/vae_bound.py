"""What the CoOp-VAE kernels are held to - hg_vae_fused.hip (Encoder -> reparameterise -> Generator as one persistent kernel), the GEMM path
and the default hybrid of hg_heads.hip, launch_reparam of hg_elem.hip: a float64 CPU reference of every stage and a bound PER OUTPUT
ELEMENT that is the sum of the worst case of each rounding the stage performs.  A plain module beside the tests
(tests/test_vae_rounding_model.py, tests/test_gpu_vae_bound.py import it): no fixtures, no GPU, no library.

    h  = relu(x W0^T + b0)      mean | log_var = h Wm^T + bm | h Wl^T + bl      z = exp(0.5 log_var) eps + mean
    g  = relu(z G0^T + c0)      bias = g G2^T + c2

Each stage is judged from the operands the kernel itself had - for a later stage the tensors the launch RETURNED.  (A worst-case bound
chained from x through four layers is useless: on `bias` a dropped generator block scores 0.02 of it at 2048 / 4096.)  All terms are
float64, u = 2^-24.

  mean, log_var   from x16 = fp16(x) and the fp16 weights (`two_layer`):
      layer 1, unit j    pre = sum_k x16_k w0_jk + b0_j: the MFMA chain starts from the bias as its C operand, K + 1 terms.
                         S = sum |x16| |w0| + |b0|,   E_pre = (K + 1) 2^-23 S   (the proved any-order, truncate-or-round worst case of
                         gemm_bound.py),   h = relu(pre),   E_h = E_pre + f16(h + E_pre),   f16(t) = 2^-11 t, or 2^-25 absolute below
                         2^-14.  relu is 1-Lipschitz: it adds nothing.
      layer 2, output n  want = sum_j h_j w_nj + b_n,
                         E = sum_j |w_nj| E_h_j + H 2^-23 sum_j (|h_j| + E_h_j) |w_nj| + u |want|   (the last term: the epilogue's bias add)
  z               from the returned mean, log_var and eps (`z_reference`): want = exp(0.5 lv) eps + mean,
                         E = |eps| exp(lv / 2) rho + u |want|.   0.5 * lv is exact, reparam1 (hg_gemm_dev.h) is one fma.  rho = 2^-23, one
                         ulp of expf: ASSUMED - the HIP math documentation that states expf's error does not ship with the toolkit the
                         project builds against, and the kernel guides do not state it.
  bias            from fp16(z returned) as an exact operand (the one kernel converts the very fp32 value it stores, launch_reparam too):
                         `two_layer` with the generator's weights.  The same expression serves hg_generator with fp16(z given).

Rule: every element of every returned tensor has |got - want| <= E.  No row norm, no global scale, no element left out.

The bound is dominated by the hidden layer's fp16 rounding summed in the worst case (sum_j |w_nj| 2^-11 h_j, where the errors add like
a random walk), so it cannot see a truncated conversion or flushed subnormals.  The families `rounded` and `tiny` carry those: every
product and partial sum is exact in fp32 in any order, the hidden layer is the exact value rounded ONCE to fp16, and mean, log_var (and
hg_generator's bias on a z of the same grid) are expected bit for bit (`exact_expected`).

`model()` is the CPU restatement of hg_vae_fused.hip's arithmetic in its own order: fp32 accumulation from the bias, 16-wide k-step by
k-step; RNE fp16 and relu of the hidden layer; layer 2 per block of 32 units; the fp32 epilogues; fp16 of the fp32 z.  With the mutants
that tests/test_vae_rounding_model.py proves the bound and the exact families reject.

Input families (`make_case`; seeded, built on the CPU, every weight an fp16 number; each asserts its own precondition):

    rounded    x and first-layer weights integers in [-16, 16], first-layer biases integers in [-64, 64]; second-layer weights integers in
               [-2, 2] times 2^-s, their biases integers in [-64, 64] on the same grid, s the smallest that keeps |outputs| <= 0.5.  Both
               layers have S < 2^24 on the integer grid.  More than a tenth of the positive h are changed by the fp16 rounding (measured
               0.16 - 0.18, max h 6 000 - 9 000 < 65 504): truncating the conversion changes most output bits.
    tiny       the same with x and first-layer weights integers in [-2, 2] x 2^-13, biases integers x 2^-26: layer-1 results fall in fp16's
               subnormal range, more than a quarter of h are non-zero subnormals (measured 0.47); second-layer weights integers in [-2, 2],
               biases integers x 2^-24.
    randn      weights 0.02 randn, all five biases 0.3 randn, x ~ randn
    unit       weights and biases as randn, x L2-normalised: the workload's input
    outlier    randn with every 97th column of x (from column 5) times 67
    dead       randn with first-layer biases -4 in every third unit and in every unit of every third 16-unit k-step (those k-steps of h
               are zero in every row: asserted) and x = 0 in every fifth row (the outputs depend on the biases alone)
    logvar     log_var.bias uniform over [-16, 16], log_var weights 0.002 randn: exp(lv / 2) runs from 3e-4 to 3e3; |z| < 6e4 asserted
    The input of a Generator-alone call (`zg`) is on x's grid for rounded / tiny, L2-normalised for unit, randn (x 30 in every 97th
    column for outlier) otherwise.

Worst |err| / E over all elements, `model()` / kernels.  `model()`: 40 rows, worst over the width pairs (128, 128), (128, 384),
(2048, 4096) of tests/test_vae_rounding_model.py.  Kernels: what tests/test_gpu_vae_bound.py prints (lines starting VAE_RATIO) on an
MI355X, worst over its widths and row counts; one = option vae_fused 2 (one kernel), gemm = option 0, `gen`: Generator alone.

    output   by       rounded  tiny     randn    unit     outlier  dead     logvar
    mean     model    0.062    0.199    0.068    0.209    0.166    0.062    0.071
             one      0.068    0.214    0.078    0.233    0.187    0.066    0.079
             gemm     0.068    0.214    0.078    0.233    0.187    0.066    0.079
             hybrid   0.068    0.214    0.072    -        -        -        -
    log_var  model    0.070    0.192    0.076    0.222    0.163    0.063    0.068
             one      0.067    0.219    0.081    0.243    0.177    0.060    0.089
             gemm     0.067    0.219    0.081    0.243    0.177    0.060    0.089
             hybrid   0.067    0.219    0.075    -        -        -        -
    z        model    0.836    0.656    0.925    0.908    0.963    0.918    0.992
             one      0.921    0.666    0.951    0.946    0.974    0.953    0.994
             gemm     0.921    0.666    0.950    0.942    0.979    0.953    0.994
             hybrid   0.921    0.666    0.942    -        -        -        -
    bias     model    0.058    0.060    0.076    0.086    0.071    0.062    0.123
             one      0.062    0.065    0.095    0.079    0.086    0.054    0.172
             gemm     0.062    0.065    0.095    0.079    0.086    0.054    0.172
             hybrid   0.062    0.065    0.037    -        -        -        -
    gen      model    0.061    0.187    0.067    0.203    0.129    0.057    0.065
             one      0.068    0.202    0.086    0.232    0.150    0.061    0.082
             gemm     0.068    0.202    0.086    0.232    0.150    0.061    0.082
             hybrid   0.068    0.202    0.042    -        -        -        -

No entry is above 1; the tests assert <= 1 and bit-equality, and no measured value is a threshold.
mean, log_var, bias, gen   0.05 - 0.25 everywhere: E is the hidden layer's fp16 rounding (and the (K + 1) 2^-23 S of its accumulation) summed
          in the worst case over H units, where the real errors add like a random walk - a fifth of E at H = 128, a fiftieth at 4096.
          `unit` and `tiny` sit highest (0.2): small |x| makes S, and with it the accumulation term, a small part of E, so that the fp16
          rounding itself is most of it.  The one kernel and the GEMM path agree to the digit: the same roundings, and at these widths
          the order of the fp32 additions moves nothing that shows in a worst case.  On `rounded` and `tiny` both paths return the float64
          result with h rounded once, bit for bit, on all three option values.
z         0.9 - 0.99 by construction: u |want| is exactly half an ulp of a result just above a power of two, so whenever the eps term is
          small the fma's own rounding fills the bound; the restatement (a correctly rounded exp) reaches the same values.  `logvar` reaches
          0.994: exp(lv / 2) up to 3e3 makes the rho term all of E and the kernel's exponential uses half of its assumed ulp.  BEFORE the
          correction of reparam1's exponential (exp_f32, hg_gemm_dev.h) this column read 2.4 - 2.8 on `logvar` and 1.5 - 2.0 on `outlier` at
          (2048, 4096) / (4096, 2048), on both paths: the build's -ffp-contract=fast let the backend contract the compiler's expansion of
          expf, whose error then grew with |lv|.
hybrid    option 1 with one round of work items and 129 rows (`rounded`, `randn` only): sampled rows; the Generator of the first
          128 n_cu rows ran as the one kernel (asserted through hg_profile).

Mutants (`MUTANTS`; numbers as in the table of tests/test_vae_rounding_model.py):
    f16_truncate          1  h / g converted to fp16 by truncation
    f16_flush             2  fp16 subnormals of h / g flushed to zero
    drop_block_mean       3  the last hidden block missing from the mean sum,
    drop_block_logvar        from the log_var sum,
    drop_block_bias          from the bias sum of the Encoder + Generator call,
    drop_block_gen           from the bias sum of the Generator-alone call
    drop_x_kstep          4  k-step 30 of x (columns 480 .. 495) dropped from every first layer
    bias_shift4           5  first-layer bias table read four units further (the lane-half offset applied twice)
    no_kidx_perm          6  layer-2 weights in the MFMA's natural k order, without the vf_kidx permutation inside a k-step
    swap_mean_logvar      7  mean and log_var output blocks swapped (ob < 8 / >= 8)
    swap_z_halves         8  z column halves [0, 256) / [256, 512) swapped as generator operand
    exp_full_lv           9  exp(lv) for exp(0.5 lv),
    exp2                     exp2(0.5 lv) for exp(0.5 lv)
    no_relu              10  relu missing on both hidden layers
    eps_neighbour        11  eps taken from the next row
    block_twice          12  hidden block nb - 1 accumulated twice (a padding iteration that is not zero)
    lv_bias_at_mean      13  log_var bias read at the mean bias's offset
"""
import functools

import torch

U = 2.0 ** -24
RHO_EXPF = 2.0 ** -23          # ASSUMED: expf within 1 ulp (module docstring)
DIM = 512
FAMILIES = ("rounded", "tiny", "randn", "unit", "outlier", "dead", "logvar")
EXACT_FAMILIES = ("rounded", "tiny")
NAMES = ("mean", "log_var", "z", "bias")
MUTANTS = ("f16_truncate", "f16_flush", "drop_block_mean", "drop_block_logvar", "drop_block_bias", "drop_block_gen", "drop_x_kstep",
           "bias_shift4", "no_kidx_perm", "swap_mean_logvar", "swap_z_halves", "exp_full_lv", "exp2", "no_relu", "eps_neighbour",
           "block_twice", "lv_bias_at_mean")
DROPPED_KSTEP = 30


def seed_of(family, eh, gh, R):
    return ((FAMILIES.index(family) * 100003 + eh) * 8209 + gh) * 4099 + R


def f16_term(t):
    """worst case of one RNE rounding to fp16 of a computed value of magnitude <= t"""
    return torch.where(t < 2.0 ** -14, torch.full_like(t, 2.0 ** -25), 2.0 ** -11 * t)


def f16(t):
    """the fp16 number nearest to t (RNE, subnormals kept), as float64"""
    return t.detach().cpu().float().half().double()


# ---- the float64 reference and the bound, stage by stage ---------------------------------------------------------------------------
def hidden(a16, w0, b0):
    """layer 1 in float64 from fp16 operands: (pre, h, E_h, S)"""
    K = a16.shape[1]
    pre = a16 @ w0.t() + b0[None]
    S = a16.abs() @ w0.abs().t() + b0.abs()[None]
    e_pre = (K + 1) * 2.0 ** -23 * S
    h = pre.clamp_min(0.0)
    return pre, h, e_pre + f16_term(h + e_pre), S


def chain(a16, layers):
    """(want, E) [R, N] of a chain of GEMMs from the fp16 operand a16: layers = [(w [N, K], b [N] or None, relu)], every operand float64,
    weights fp16 numbers.  Every layer but the last is rounded once to fp16 (after its relu, where it has one) and carries its error
    E_h into the next: E_h @ |w| for what the operand is off, K 2^-23 (|h| + E_h) @ |w| for the accumulation (K + 1 terms and + |b| with
    a bias, which starts the MFMA chain or is added by the epilogue: the bound covers both).  The last layer is returned in fp32: its
    bias add rounds once, u |want|.  chain(a16, [(w0, b0, True), (w2, b2, False)]) is `two_layer` term for term."""
    h, e_h = a16, torch.zeros_like(a16)
    for i, (w, b, relu) in enumerate(layers):
        K, aw = w.shape[1], w.abs().t()
        last = i == len(layers) - 1
        pre = h @ w.t() + (b[None] if b is not None else 0.0)
        S = (h.abs() + e_h) @ aw
        if last:
            e = e_h @ aw + K * 2.0 ** -23 * S
            return pre, (e + U * pre.abs() if b is not None else e)
        e_pre = e_h @ aw + ((K + 1) * 2.0 ** -23 * (S + b.abs()[None]) if b is not None else K * 2.0 ** -23 * S)
        h = pre.clamp_min(0.0) if relu else pre
        e_h = e_pre + f16_term(h.abs() + e_pre)


def two_layer(a16, w0, b0, w2, b2):
    """(want, E) [R, N] of relu(a16 w0^T + b0) w2^T + b2; every operand float64, a16 / w0 / w2 fp16 numbers"""
    return chain(a16, [(w0, b0, True), (w2, b2, False)])


def _d(t, rows=None):
    t = t.detach().cpu().double()
    return t if rows is None else t[rows]


def enc_reference(c, rows=None):
    """{"mean": (want, E), "log_var": (want, E)} from fp16(x) of the case (rows: an index into the case's rows)"""
    w2 = torch.cat([c["e_wm"], c["e_wl"]]).double()
    b2 = torch.cat([c["e_bm"], c["e_bl"]]).double()
    want, E = two_layer(f16(_d(c["x"], rows)), c["e_w0"].double(), c["e_b0"].double(), w2, b2)
    return {"mean": (want[:, :DIM], E[:, :DIM]), "log_var": (want[:, DIM:], E[:, DIM:])}


def z_reference(mean, log_var, eps):
    """(want, E) of z from the mean and log_var the launch returned"""
    mean, lv, eps = _d(mean), _d(log_var), _d(eps)
    std = torch.exp(0.5 * lv)
    want = std * eps + mean
    return want, eps.abs() * std * RHO_EXPF + U * want.abs()


def gen_reference(c, z):
    """(want, E) of the Generator on fp16(z): z the fp32 tensor the launch returned (or was given)"""
    return two_layer(f16(z), c["g_w0"].double(), c["g_b0"].double(), c["g_w2"].double(), c["g_b2"].double())


def worst(got, want, E):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / E)
    return float(r.max()) if bool(torch.isfinite(got).all()) else float("inf")


def ratios(c, out, rows=None, enc_ref=None, operands=None):
    """Worst |err| / E per tensor of one launch: out = {name: tensor} with any of mean, log_var, z, bias (Encoder / VAE call on the
    case's x and eps, restricted to `rows` if given - the tensors of `out` are then those rows) and gen (Generator alone on zg).
    enc_ref: a cached enc_reference(c, rows).  operands: the tensors to take mean / log_var / z from where `out` lacks them (a call
    that returned only some outputs, judged with those of a call that returned all, bit-identical where both have them)."""
    ops = dict(operands or {})
    ops.update(out)
    r = {}
    if "mean" in out or "log_var" in out:
        ref = enc_ref or enc_reference(c, rows)
        for n in ("mean", "log_var"):
            if n in out:
                r[n] = worst(out[n], *ref[n])
    if "z" in out:
        r["z"] = worst(out["z"], *z_reference(ops["mean"], ops["log_var"], _d(c["eps"], rows)))
    if "bias" in out:
        r["bias"] = worst(out["bias"], *gen_reference(c, ops["z"]))
    if "gen" in out:
        r["gen"] = worst(out["gen"], *gen_reference(c, _d(c["zg"], rows)))
    return r


def exact_expected(c, rows=None):
    """`rounded` / `tiny`: {"mean", "log_var", "gen"} as float32 - the float64 result with h rounded once, what torch.equal is asked for"""
    assert c["family"] in EXACT_FAMILIES
    exp = {}

    def layer(a, w0, b0, w2, b2):
        _, h, _, _ = hidden(f16(a), w0.double(), b0.double())
        want = f16(h) @ w2.double().t() + b2.double()[None]
        assert bool((want.float().double() == want).all()), "the family is not exact in fp32 at this shape"
        return want.float()

    ml = layer(_d(c["x"], rows), c["e_w0"], c["e_b0"], torch.cat([c["e_wm"], c["e_wl"]]), torch.cat([c["e_bm"], c["e_bl"]]))
    exp["mean"], exp["log_var"] = ml[:, :DIM].contiguous(), ml[:, DIM:].contiguous()
    exp["gen"] = layer(_d(c["zg"], rows), c["g_w0"], c["g_b0"], c["g_w2"], c["g_b2"])
    return exp


# ---- input families ---------------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _exact_layers(g, a, H, unit1, unit_b, family):
    """first layer on a's grid and a second layer [512 .. , H] of integers in [-2, 2] x 2^-s (rounded) / x 1 (tiny) for the input a
    (float64 [R, 512]); asserts the family's preconditions -> (w0, b0, w2 [1024, H], b2 [1024])"""
    w0 = _ints(g, -16, 16, H, DIM) * unit1 if family == "rounded" else _ints(g, -2, 2, H, DIM) * unit1
    b0 = _ints(g, -64, 64, H) * unit_b
    pre, h, _, S = hidden(a, w0, b0)
    assert float(S.max()) / unit_b < 2.0 ** 24, "layer 1 is not exact in fp32"
    assert float(h.max()) < 65504.0
    h16 = f16(h)
    pos = h > 0
    if family == "rounded":
        share = float((h16 != h)[pos].double().mean())
        assert share >= 0.1, f"only {share:.3f} of the positive h are changed by the fp16 rounding"
        unit_h = 1.0
    else:
        sub = (h16 > 0) & (h16 < 2.0 ** -14)
        assert float(sub.double().mean()) >= 0.25, f"only {float(sub.double().mean()):.3f} of h are non-zero fp16 subnormals"
        assert float(h.max()) < 2.0 ** -14
        unit_h = 2.0 ** -24
    w2i, b2i = _ints(g, -2, 2, 2 * DIM, H), _ints(g, -64, 64, 2 * DIM)
    acc = (h16 / unit_h) @ w2i.t() + b2i[None]
    S2 = (h16 / unit_h) @ w2i.abs().t() + b2i.abs()[None]
    assert float(S2.max()) < 2.0 ** 24, "layer 2 is not exact in fp32"
    s = 0
    if family == "rounded":
        while float(acc.abs().max()) * 2.0 ** -s > 0.5:
            s += 1
    return w0, b0, w2i * 2.0 ** -s, b2i * (unit_h * 2.0 ** -s)


@functools.lru_cache(maxsize=4)
def make_case(family, eh, gh, R):
    """Weights and inputs of one VAE, float32 on the CPU: x, eps, zg [R, 512]; e_w0 [eh, 512], e_b0 [eh], e_wm, e_wl [512, eh], e_bm,
    e_bl [512]; g_w0 [gh, 512], g_b0 [gh], g_w2 [512, gh], g_b2 [512].  Weights are fp16 numbers.  Cached: the tests that share a case
    must leave it unchanged."""
    assert family in FAMILIES and eh % 128 == 0 and gh % 128 == 0
    g = torch.Generator().manual_seed(seed_of(family, eh, gh, R))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    c = {"family": family, "eh": eh, "gh": gh, "R": R}
    eps = rn(R, DIM)
    if family in EXACT_FAMILIES:
        assert R <= 1024, "the exact families fix their scale from every row"
        if family == "rounded":
            x, zg, unit1, unit_b = _ints(g, -16, 16, R, DIM), _ints(g, -16, 16, R, DIM), 1.0, 1.0
        else:
            x, zg, unit1, unit_b = _ints(g, -2, 2, R, DIM) * 2.0 ** -13, _ints(g, -2, 2, R, DIM) * 2.0 ** -13, 2.0 ** -13, 2.0 ** -26
        e_w0, e_b0, wml, bml = _exact_layers(g, x, eh, unit1, unit_b, family)
        g_w0, g_b0, w2, b2 = _exact_layers(g, zg, gh, unit1, unit_b, family)
        e_wm, e_wl, e_bm, e_bl = wml[:DIM], wml[DIM:], bml[:DIM], bml[DIM:]
        g_w2, g_b2 = w2[:DIM], b2[:DIM]
    else:
        x, zg = rn(R, DIM), rn(R, DIM)
        e_w0, e_wm, e_wl, g_w0, g_w2 = 0.02 * rn(eh, DIM), 0.02 * rn(DIM, eh), 0.02 * rn(DIM, eh), 0.02 * rn(gh, DIM), 0.02 * rn(DIM, gh)
        e_b0, e_bm, e_bl, g_b0, g_b2 = 0.3 * rn(eh), 0.3 * rn(DIM), 0.3 * rn(DIM), 0.3 * rn(gh), 0.3 * rn(DIM)
        if family == "unit":
            x, zg = x / x.norm(dim=1, keepdim=True), zg / zg.norm(dim=1, keepdim=True)
        elif family == "outlier":
            x[:, 5::97] *= 67.0
            zg[:, 5::97] *= 30.0
        elif family == "dead":
            for b0 in (e_b0, g_b0):
                j = torch.arange(b0.numel())
                b0[(j % 3 == 0) | ((j // 16) % 3 == 0)] = -4.0
            x[::5] = 0.0
            zg[::5] = 0.0
        elif family == "logvar":
            e_wl = 0.002 * rn(DIM, eh)
            e_bl = 32.0 * torch.rand(DIM, generator=g, dtype=torch.float64) - 16.0
    for k, v in (("x", x), ("eps", eps), ("zg", zg), ("e_b0", e_b0), ("e_bm", e_bm), ("e_bl", e_bl), ("g_b0", g_b0), ("g_b2", g_b2)):
        c[k] = v.float().contiguous()
    for k, v in (("e_w0", e_w0), ("e_wm", e_wm), ("e_wl", e_wl), ("g_w0", g_w0), ("g_w2", g_w2)):
        c[k] = v.half().float().contiguous()
    if family in EXACT_FAMILIES:
        for k in ("x", "zg", "e_b0", "e_bm", "e_bl", "g_b0", "g_b2", "e_w0", "e_wm", "e_wl", "g_w0", "g_w2"):
            src = {"x": x, "zg": zg, "e_b0": e_b0, "e_bm": e_bm, "e_bl": e_bl, "g_b0": g_b0, "g_b2": g_b2, "e_w0": e_w0, "e_wm": e_wm,
                   "e_wl": e_wl, "g_w0": g_w0, "g_w2": g_w2}[k]
            assert bool((c[k].double() == src).all()), f"{k} is not exact in its storage format"
    if family == "dead":
        sample = slice(0, min(R, 64))
        for a, w0, b0 in ((c["x"], c["e_w0"], c["e_b0"]), (c["zg"], c["g_w0"], c["g_b0"])):
            _, h, _, _ = hidden(f16(a[sample]), w0.double(), b0.double())
            assert bool((h.view(h.shape[0], -1, 16)[:, ::3] == 0).all()), "dead: a k-step of h that should be zero is not"
    if family == "logvar":
        sample = torch.arange(0, R, max(1, R // 256))
        ref = enc_reference(c, sample)
        zw, _ = z_reference(ref["mean"][0], ref["log_var"][0], c["eps"][sample])
        std = torch.exp(0.5 * ref["log_var"][0])
        assert float(zw.abs().max()) < 6e4 and float(std.min()) < 1e-3 and float(std.max()) > 1e3
    return c


# ---- the CPU restatement of hg_vae_fused.hip's arithmetic ---------------------------------------------------------------------------
def vf_kidx(s, h, j):
    return 16 * s + (j & 3) + 8 * (j >> 2) + 4 * h


def _to_f16(v, mutant):
    """fp32 -> fp16 -> fp32 as v_cvt_pk_f16_f32 (RNE, subnormals kept)"""
    h = v.half()
    if mutant == "f16_truncate":
        bits = h.view(torch.int16).int()
        over = h.float().abs() > v.abs()
        h = torch.where(over, bits - 1, bits).short().view(torch.float16)      # one step towards zero (sign bit untouched)
    if mutant == "f16_flush":
        h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
    return h.float()


def _pass(a, w0, b0, w2, mutant, drop_cols=None, twice=False):
    """one pass of the kernel: a [R, 512] fp32 (fp16 numbers), -> the layer-2 accumulators [R, N] fp32, before the epilogue"""
    R, H = a.shape[0], w0.shape[0]
    nb = H // 32
    if mutant == "bias_shift4":
        b0 = torch.roll(b0, -4)
    if mutant == "no_kidx_perm":
        src = torch.empty(H, dtype=torch.long)
        for s in range(H // 16):
            for hh in range(2):
                for j in range(8):
                    src[vf_kidx(s, hh, j)] = 16 * s + 8 * hh + j      # unit vf_kidx(s, hh, j) of h meets the weight of unit 16 s + 8 hh + j
        w2 = w2[:, src]
    acc = b0[None].expand(R, H).contiguous()
    for s in range(DIM // 16):
        if mutant == "drop_x_kstep" and s == DROPPED_KSTEP:
            continue
        acc = acc + a[:, 16 * s:16 * s + 16] @ w0[:, 16 * s:16 * s + 16].t()
    h = _to_f16(acc, mutant)
    if mutant != "no_relu":
        h = h.clamp_min(0.0)
    out = torch.zeros(R, w2.shape[0], dtype=torch.float32)
    for t in range(nb):
        part = h[:, 32 * t:32 * t + 32] @ w2[:, 32 * t:32 * t + 32].t()
        if t == nb - 1 and drop_cols is not None:
            part[:, drop_cols] = 0.0
        out = out + part
        if t == nb - 1 and twice:
            out = out + part
    return out


def model(c, mutant=None, rows=None):
    """The one kernel's arithmetic on the CPU -> {"mean", "log_var", "z", "bias", "gen"} float32 (gen: the Generator alone on zg)"""
    assert mutant is None or mutant in MUTANTS, mutant
    x, eps, zg = c["x"], c["eps"], c["zg"]
    if rows is not None:
        x, eps, zg = x[rows], eps[rows], zg[rows]
    wml, bm, bl = torch.cat([c["e_wm"], c["e_wl"]]), c["e_bm"], c["e_bl"]
    drop = {"drop_block_mean": slice(0, DIM), "drop_block_logvar": slice(DIM, 2 * DIM)}.get(mutant)
    acc = _pass(x.half().float(), c["e_w0"], c["e_b0"], wml, mutant, drop, mutant == "block_twice")
    m_acc, l_acc = acc[:, :DIM], acc[:, DIM:]
    if mutant == "swap_mean_logvar":
        m_acc, l_acc = l_acc, m_acc
    mean = m_acc + bm[None]
    lv = l_acc + (bm if mutant == "lv_bias_at_mean" else bl)[None]
    e = torch.roll(eps, -1, 0) if mutant == "eps_neighbour" else eps
    t = 0.5 * lv
    if mutant == "exp_full_lv":
        t = lv
    std = (torch.exp2(t.double()) if mutant == "exp2" else torch.exp(t.double())).float()
    z = (std.double() * e.double() + mean.double()).float()      # one fma
    z16 = z.half().float()
    if mutant == "swap_z_halves":
        z16 = torch.cat([z16[:, DIM // 2:], z16[:, :DIM // 2]], 1)
    all_cols = slice(0, DIM)
    bias = _pass(z16, c["g_w0"], c["g_b0"], c["g_w2"], mutant, all_cols if mutant == "drop_block_bias" else None,
                 mutant == "block_twice") + c["g_b2"][None]
    gen = _pass(zg.half().float(), c["g_w0"], c["g_b0"], c["g_w2"], mutant, all_cols if mutant == "drop_block_gen" else None,
                mutant == "block_twice") + c["g_b2"][None]
    return {"mean": mean.contiguous(), "log_var": lv.contiguous(), "z": z, "bias": bias, "gen": gen}
