"""What the heads at the end of the pipeline are held to - hg_cache_logits / hg_mlp_net (hg_heads.hip) with the host folding of
hg_load_cache / hg_load_mlp (hg_load.hip): a float64 CPU reference from the operands the device holds and a bound PER OUTPUT ELEMENT
that is the sum of the worst case of each rounding.  A plain module beside the tests (tests/test_heads_rounding_model.py,
tests/test_gpu_heads.py import it): no fixtures, no GPU, no library.  The accumulation bound is `vae_bound.chain` (K 2^-23 S per GEMM, the
proved any-order worst case of gemm_bound.py; a hidden layer's fp16 rounding carried through the next weights); nothing here restates it.

cache logits with labels      out[r, c] = ((f16 W16^T) L16 + bL) * scale          f16 = fp16(features), W16 = fp16(weight), L16 = fp16(labels)
    phi = f16 W16^T is accumulated in fp32 and rounded ONCE to fp16; the second GEMM accumulates phi16 L16 in fp32; the epilogue adds
    bL[c] and multiplies by scale[c].  bL[c] = sum_s bias_s labels_sc is the host's double sum over the fp32 bias and the fp32 labels
    (the labels of THIS term never pass through fp16), rounded to fp32; scale[c] = fl(1 / fl(lens_c post_div)) as the loader computes it
    in fp32, taken as an exact operand.  u = 2^-24:
        E = chain's error of phi L                 first GEMM's K 2^-23 S1 and phi's fp16 rounding through sum_s |L16|, plus S 2^-23 (|phi| + E_phi) |L16|
          + |scale| (u |bL| + u |phi L + bL|)       bL's rounding to fp32, the epilogue's add
          + 2 u |want|                             the scale multiply and the add onto the zeroed destination (one fma in the kernels)
    Precondition: |phi| + E_phi <= 65504 (beyond it fp16(phi) is inf and no bound holds); `cache_reference` asserts it, for every family.
cache logits without labels   out[r, s] = f16 W16^T + b: `chain` with the one layer.
mlp_net                       relu(relu(x16 W0^T + b0) W2^T + b2) W4^T + b4, two fp16 hidden layers, fp32 output: `chain` with three.

Rule: every element of every output has |got - want| <= E; on the exact families got is the float64 result (hidden layers rounded once
to fp16) bit for bit, on either GEMM kernel.

Families (`cache_case`, `mlp_case`; seeded, built on the CPU):
    rounded    as exact with features and weights integers in [-m, m], m from K such that |phi| reaches a few thousand: above 2048 the
               fp16 rounding changes phi (asserted: more than 2 %); expected is the float64 result with phi rounded ONCE, bit for bit
    exact      features and weights integers in [-2, 2], labels in {0, 1}, biases integers in [-4, 4], lens and post_div powers of two: phi
               is an integer that fp16 holds exactly (asserted), every sum is exact in fp32 in any order (asserted).  mlp_net: x, W0
               integers in [-2, 2], W2 in [-m, m] (m from the widths), W4 in [-2, 2], integer biases; the first hidden layer is exact in fp16, the second is
               rounded (values above 2048; asserted), the output exact in fp32 (asserted).
    unit       L2-normalised feature and weight rows: the workload            randn      f randn, W randn K^-0.5, b randn
    outlier    randn with one feature column x 67                            soft       labels uniform in [0, 1], not fp16 numbers
    sparse     one-hot labels, every fifth class empty with lens = 1          biasdom    b = 100 randn and f = 0.01 randn: |bL| >> |phi L|

`cache_model` / `mlp_model` restate the arithmetic on the CPU (fp32 accumulation K-tile by K-tile, RNE fp16, the padded layouts Sp / Cp,
the chunk loop and copy_cols), with the mutants tests/test_heads_rounding_model.py proves the rule rejects:
    phi_truncate       phi truncated to fp16                      bias_in_phi        the bias added inside phi, in front of the fp16 rounding
    bl_dropped         bL left out                                post_div_twice / post_div_none
    scale_padded       scale read at the column's index counted from the end of the padded row (c + Cp - C)
    drop_last_block    the last 128-column block of Sp missing from the second sum
    pad_row_nonzero    the weight rows S .. Sp - 1 not zeroed (uninitialised memory, here NaN: the padded labels are zero, and only a
                       non-finite phi shows through a zero)
    labels_stride      the transposed labels written with row stride Cp where Sp belongs
    copy_ld_nout       copy_cols reading with ld = Nout           chunk_at_np        a chunk's rows written at out + r0 * Np
    relu_missing       (mlp_net) no relu                          bias_l2_for_l1     (mlp_net) layer 1 adds layer 2's bias

Worst |err| / E over all elements: `cache_model` / `mlp_model` on the shapes of tests/test_heads_rounding_model.py, and the kernels as
tests/test_gpu_heads.py prints them (lines HEADS_RATIO) on an MI355X, worst over its shapes, row counts and both GEMM kernels:

    output                 by       exact    rounded  unit     randn    outlier  soft     sparse   biasdom
    cache logits, labels   model    0        0.396    0.684    0.607    0.579    0.187    0.816    0.487
                           kernels  0        0.512    0.745    0.591    0.532    0.123    0.717    0.395
    cache logits, linear   model    0        0        0.024    0.031    0.058    0.030    0.022    0.940
                           kernels  0        0        0.019    0.004    0.012    -        -        0.847
    mlp_net                model    0.019    -        0.040    0.027    0.036    -        -        -
                           kernels  0.023    -        0.008    0.046    0.005    -        -        -

No entry is above 1; the tests assert <= 1 and bit-equality, and no measured value is a threshold.  On `exact` and `rounded` every
output of every call - simple kernel, ring kernels, any chunking - is the float64 result bit for bit (0 in the table where that result
is the reference itself; mlp_net's 0.02 is its second hidden layer's fp16 rounding, which the float64 reference does not make and the
bit-for-bit expectation does).  With labels E is mostly phi's fp16 rounding carried in the worst case through sum |L16|, where the real
errors add like a random walk: 0.4 - 0.8, highest on `sparse` and `unit`, whose few labels per class leave little to average.  The linear
map and mlp_net's fp32 output are dominated by K 2^-23 S, a worst case over every summation order: a few hundredths; `biasdom` is the
exception (0.85 - 0.94), where |b| >> |acc| and the single rounding of acc + b, u |want|, is nearly all of E and half an ulp of a result
just above a power of two uses it up.  No bug was found in hg_heads.hip or the loaders by these tests.
"""
import functools

import torch

import vae_bound as vb

U = 2.0 ** -24
CACHE_FAMILIES = ("exact", "rounded", "unit", "randn", "outlier", "soft", "sparse", "biasdom")
EXACT_FAMILIES = ("exact", "rounded")
MLP_FAMILIES = ("exact", "randn", "unit", "outlier")
CACHE_MUTANTS = ("phi_truncate", "bias_in_phi", "bl_dropped", "post_div_twice", "post_div_none", "scale_padded", "drop_last_block",
                 "pad_row_nonzero", "labels_stride", "copy_ld_nout", "chunk_at_np")
MLP_MUTANTS = ("relu_missing", "bias_l2_for_l1")


def rup(n, m):
    return (n + m - 1) // m * m


def ring_kernel(M, N, K):
    """launch_gemm's choice (gemm_ring_ok, hg_gemm_ring.hip): the ring kernels for M >= 512, K >= 256, N % 256 == 0, else the simple one"""
    return M >= 512 and K >= 256 and K % 64 == 0 and N % 256 == 0 and N <= 8192


def chunks(R, m):
    """chunk_rows of hg_heads.hip: the last chunk absorbs a tail of up to an eighth"""
    out, left = [], R
    while left > 0:
        rc = left if left <= m + m // 8 else m
        out.append(rc)
        left -= rc
    return out


_ints = vb._ints


# ---- cache logits -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def cache_case(family, R, S, C, K, labels=True, post_div=2.0):
    """float32 CPU tensors: f [R, K], w [S, K], b [S], lab [S, C], lens [C]; post_div.  Cached: leave unchanged."""
    assert family in CACHE_FAMILIES
    g = torch.Generator().manual_seed((((CACHE_FAMILIES.index(family) * 1009 + R) * 1013 + S) * 1019 + C) * 1021 + K)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    if family == "exact":
        f, w, b = _ints(g, -2, 2, R, K), _ints(g, -2, 2, S, K), _ints(g, -4, 4, S)
        lab = (torch.rand(S, C, generator=g) < 0.25).double()
        lens = 2.0 ** _ints(g, 0, 3, C)
    elif family == "rounded":
        m = int(round((6000.0 / K ** 0.5) ** 0.5))          # phi of a few thousand: above 2048 fp16 rounds integers
        f, w, b = _ints(g, -m, m, R, K), _ints(g, -m, m, S, K), _ints(g, -4, 4, S)
        lab = (torch.rand(S, C, generator=g) < 0.25).double()
        lens = 2.0 ** _ints(g, 0, 3, C)
    else:
        f, w, b = rn(R, K), rn(S, K) * K ** -0.5, rn(S)
        lab = (torch.rand(S, C, generator=g) < 0.1).double()
        if family == "unit":
            f, w, b = f / f.norm(dim=1, keepdim=True), w / w.norm(dim=1, keepdim=True), 0.1 * b
        elif family == "outlier":
            f[:, K // 3] *= 67.0
        elif family == "soft":
            lab = torch.rand(S, C, generator=g, dtype=torch.float64)
        elif family == "sparse":
            lab = torch.zeros(S, C, dtype=torch.float64)
            cls = torch.randint(0, C, (S,), generator=g)
            cls = torch.where(cls % 5 == 4, (cls + 1) % C if C > 1 else cls, cls)      # every fifth class stays empty (C > 5)
            lab[torch.arange(S), cls] = 1.0
        elif family == "biasdom":
            f, b = 0.01 * f, 100.0 * b
        lens = lab.sum(0).clamp_min(1.0) if family != "soft" else torch.full((C,), float(S), dtype=torch.float64)
    c = {"family": family, "R": R, "S": S, "C": C, "K": K, "has_labels": labels, "post_div": post_div if labels else 1.0,
         "f": f.float().contiguous(), "w": w.float().contiguous(), "b": b.float().contiguous(),
         "lab": lab.float().contiguous(), "lens": lens.float().contiguous()}
    if family == "soft":
        assert bool((c["lab"].half().float() != c["lab"]).float().mean() > 0.9), "soft labels must not be fp16 numbers"
    if family == "sparse" and C > 5:
        assert bool((lab.sum(0) == 0).any()) and bool((c["lens"][lab.sum(0) == 0] == 1).all())
    return c


def loader_scale(c):
    """scale[C] as hg_load_cache computes it: 1.0f / (lens * post_div) in fp32 -> float64"""
    pd = torch.tensor(c["post_div"] if c["post_div"] != 0 else 1.0, dtype=torch.float32)
    return (torch.tensor(1.0, dtype=torch.float32) / (c["lens"] * pd)).double()


def host_bl(c):
    """sum_s bias_s labels_sc over the fp32 bias and the fp32 labels, float64 (the host rounds it to fp32: a term of E)"""
    return c["b"].double() @ c["lab"].double()


def cache_reference(c, rows=None):
    """(want, E) float64 [R, C] ([R, S] without labels), asserting the bound's precondition |phi| <= 65504"""
    f16 = vb.f16(c["f"] if rows is None else c["f"][rows])
    w16 = vb.f16(c["w"])
    if not c["has_labels"]:
        return vb.chain(f16, [(w16, c["b"].double(), False)])
    phi = f16 @ w16.t()
    e_phi = c["K"] * 2.0 ** -23 * (f16.abs() @ w16.abs().t())
    assert float((phi.abs() + e_phi).max()) <= 65504.0, "|phi| > 65504: fp16(phi) is inf, the bound has no meaning"
    acc, e = vb.chain(f16, [(w16, None, False), (vb.f16(c["lab"]).t().contiguous(), None, False)])
    bl, sc = host_bl(c)[None], loader_scale(c)[None]
    want = (acc + bl) * sc
    return want, sc.abs() * (e + U * bl.abs() + U * (acc + bl).abs()) + 2 * U * want.abs()


def cache_exact(c, rows=None):
    """`exact`: the float64 result as float32, what torch.equal is asked for; asserts that every stage is exact"""
    assert c["family"] in EXACT_FAMILIES
    f, w = (c["f"] if rows is None else c["f"][rows]).double(), c["w"].double()
    assert bool((vb.f16(c["f"]) == c["f"].double()).all()) and bool((vb.f16(c["w"]) == w).all())
    phi = f @ w.t()
    if not c["has_labels"]:
        want = phi + c["b"].double()[None]
    else:
        assert float(phi.abs().max()) <= 65504.0 and float((f.abs() @ w.abs().t()).max()) < 2.0 ** 24
        if c["family"] == "exact":
            assert bool((vb.f16(phi) == phi).all()), "phi is not exact in fp16"
        elif c["has_labels"] and phi.shape[0] >= 16:
            assert float((vb.f16(phi) != phi).double().mean()) > 0.02, "too few phi are changed by the fp16 rounding"
        phi = vb.f16(phi)
        lab = c["lab"].double()
        assert float((phi.abs() @ lab).max()) + float(host_bl(c).abs().max()) < 2.0 ** 24, "the second sum is not exact in fp32"
        sc = loader_scale(c)
        assert bool((torch.log2(sc) == torch.log2(sc).round()).all()), "scale is not a power of two"
        want = (phi @ lab + host_bl(c)[None]) * sc[None]
    assert bool((want.float().double() == want).all())
    return want.float()


def _to_f16(v, truncate=False):
    h = v.half()
    if truncate:
        bits = h.view(torch.int16).int()
        h = torch.where(h.float().abs() > v.abs(), bits - 1, bits).short().view(torch.float16)
    return h.float()


def _gemm32(a, w):
    """fp32 accumulation K-tile by K-tile (64 wide), as gemm_bound.model"""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 64):
        acc = acc + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
    return acc


def cache_model(c, mutant=None, chunk_rows=1 << 30):
    """hg_load_cache + hg_cache_logits on the CPU -> float32 [R, Nout]"""
    assert mutant is None or mutant in CACHE_MUTANTS, mutant
    R, S, C, K = c["R"], c["S"], c["C"], c["K"]
    Sp, Cp = rup(S, 128), rup(C, 128) if c["has_labels"] else 0
    w16 = torch.zeros(Sp, K)
    if mutant == "pad_row_nonzero":
        w16[S:] = float("nan")
    w16[:S] = c["w"].half().float()
    bias = torch.zeros(Sp)
    bias[:S] = c["b"]
    if c["has_labels"]:
        lt = torch.zeros(Cp * Sp)
        stride = Cp if mutant == "labels_stride" else Sp
        idx = (torch.arange(C)[:, None] * stride + torch.arange(S)[None]).reshape(-1)
        ok = idx < lt.numel()
        lt[idx[ok]] = c["lab"].t().reshape(-1)[ok]
        lt16 = lt.half().float().view(Cp, Sp)
        bc, sc = torch.zeros(Cp), torch.zeros(Cp)
        bc[:C] = torch.zeros(C) if mutant == "bl_dropped" or mutant == "bias_in_phi" else host_bl(c).float()
        pd = torch.tensor(c["post_div"], dtype=torch.float32)
        div = c["lens"] * (pd * pd if mutant == "post_div_twice" else (torch.tensor(1.0) if mutant == "post_div_none" else pd))
        sc[:C] = torch.tensor(1.0, dtype=torch.float32) / div
        if mutant == "scale_padded":
            sc = torch.roll(sc, -(Cp - C))
    Np, Nout = (Cp, C) if c["has_labels"] else (Sp, S)
    out = torch.full((R * Nout + Np * (R + 1),), float("nan"))      # (room behind the tensor for the mutants that write there)
    r0 = 0
    for Rc in chunks(R, chunk_rows):
        f16 = c["f"][r0:r0 + Rc].half().float()
        if not c["has_labels"]:
            tmp = _gemm32(f16, w16) + bias[None]
        else:
            phi = _gemm32(f16, w16)
            if mutant == "bias_in_phi":
                phi = phi + bias[None]
            phi16 = _to_f16(phi, mutant == "phi_truncate")
            a, l16 = (phi16[:, :Sp - 128], lt16[:, :Sp - 128]) if mutant == "drop_last_block" else (phi16, lt16)
            acc = _gemm32(a, l16) if a.shape[1] else torch.zeros(Rc, Cp)
            tmp = ((acc + bc[None]).double() * sc[None].double()).float()          # fmaf(acc + b, scale, 0)
        ld = Nout if mutant == "copy_ld_nout" else Np
        flat = torch.cat([tmp.reshape(-1), torch.zeros(Np)])
        rows = torch.arange(Rc)[:, None] * ld + torch.arange(Nout)[None]
        at = r0 * (Np if mutant == "chunk_at_np" else Nout)
        out[at:at + Rc * Nout] = flat[rows].reshape(-1)
        r0 += Rc
    return out[:R * Nout].view(R, Nout).clone()


# ---- mlp_net ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def mlp_case(family, R, d_in, hid, d_out):
    """float32 CPU tensors x [R, in], w0 [hid, in], b0, w2 [hid, hid], b2, w4 [out, hid], b4; weights fp16 numbers.  Cached."""
    assert family in MLP_FAMILIES
    g = torch.Generator().manual_seed((((MLP_FAMILIES.index(family) * 1009 + R) * 1013 + d_in) * 1019 + hid) * 1021 + d_out)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    if family == "exact":
        x, w0, b0 = _ints(g, -2, 2, R, d_in), _ints(g, -2, 2, hid, d_in), _ints(g, -8, 8, hid)
        m2 = max(2, int(round(5200.0 / (2.0 * d_in * hid) ** 0.5)))          # second hidden layer of a few thousand: above 2048 fp16 rounds integers
        w2, b2 = _ints(g, -m2, m2, hid, hid), _ints(g, -64, 64, hid)
        w4, b4 = _ints(g, -2, 2, d_out, hid), _ints(g, -64, 64, d_out)
    else:
        x = rn(R, d_in)
        w0, w2, w4 = rn(hid, d_in) * d_in ** -0.5, rn(hid, hid) * hid ** -0.5, rn(d_out, hid) * hid ** -0.5
        b0, b2, b4 = 0.3 * rn(hid), 0.3 * rn(hid), 0.3 * rn(d_out)
        if family == "unit":
            x = x / x.norm(dim=1, keepdim=True)
        elif family == "outlier":
            x[:, d_in // 3] *= 67.0
    c = {"family": family, "R": R, "dims": (d_in, hid, d_out), "x": x.float().contiguous()}
    for k, v in (("w0", w0), ("w2", w2), ("w4", w4)):
        c[k] = v.half().float().contiguous()
    for k, v in (("b0", b0), ("b2", b2), ("b4", b4)):
        c[k] = v.float().contiguous()
    return c


def _layers(c):
    return [(c["w0"].double(), c["b0"].double(), True), (c["w2"].double(), c["b2"].double(), True), (c["w4"].double(), c["b4"].double(), False)]


def mlp_reference(c, rows=None):
    return vb.chain(vb.f16(c["x"] if rows is None else c["x"][rows]), _layers(c))


def mlp_exact(c, rows=None):
    """`exact`: float64 with each hidden layer rounded once to fp16, as float32; asserts the exactness of every sum"""
    assert c["family"] == "exact"
    h = (c["x"] if rows is None else c["x"][rows]).double()
    assert bool((vb.f16(c["x"]) == c["x"].double()).all())
    changed = []
    for i, (w, b, relu) in enumerate(_layers(c)):
        assert float((h.abs() @ w.abs().t() + b.abs()[None]).max()) < 2.0 ** 24, f"layer {i} is not exact in fp32"
        pre = h @ w.t() + b[None]
        if not relu:
            assert bool((pre.float().double() == pre).all())
            assert changed[0] == 0.0 and changed[1] > 0.01, f"hidden layers changed by the fp16 rounding: {changed}"
            return pre.float()
        pre = pre.clamp_min(0.0)
        assert float(pre.max()) <= 65504.0
        h = vb.f16(pre)
        changed.append(float((h != pre).double().mean()))


def mlp_model(c, mutant=None):
    assert mutant is None or mutant in MLP_MUTANTS, mutant
    h = c["x"].half().float()
    b0 = c["b2"] if mutant == "bias_l2_for_l1" else c["b0"]
    for w, b, relu in ((c["w0"], b0, True), (c["w2"], c["b2"], True)):
        v = _gemm32(h, w) + b[None]
        h = _to_f16(v if mutant == "relu_missing" else v.clamp_min(0.0))
    return _gemm32(h, c["w4"]) + c["b4"][None]


def worst(got, want, E):
    return vb.worst(got, want, E)
