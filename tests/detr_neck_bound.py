"""What the DETR neck (hoigen_amd/csrc/hg_detr_neck.hip: input_proj, the key-padding mask on the feature grid and the sine embedding in
one call; the reference's upt_tip_cache_model_free_finetune_distill3.py:1594-1597 over detr/models/detr.py:40, :65, backbone.py:78,
position_encoding.py:28-48) is held to: the statements in float64 on the CPU from the UNROUNDED operands (x and the weights as the caller
holds them, fp32; scale and temperature as Python floats), and a bound PER ELEMENT that sums the worst case of every rounding the kernel
performs.  A plain module beside the tests: no fixtures, no GPU, no library.

All float64, u = 2^-24.

  src    y = sum_k x_k W_k + b.  The kernel holds x^ = fp16(x) and W^ = fp16(W) (ex = |x^ - x|, eW = |W^ - W|, the ACTUAL roundings):
             E = sum_k (ex_k |W_k| + |x_k| eW_k + ex_k eW_k)      the operands' errors through the product
               + K u T,  T = sum_k (|x_k| + ex_k)(|W_k| + eW_k)    fp32 accumulation of K products (K u sum |a| |b|)
               + (n - 1) u T (1 + K u)                             the n - 1 additions of the partial sums of a split over n slices
               + u (T (1 + K u) + |b|)                             the bias add after the sum
         A NaN operand makes the row NaN in the reference and must in the kernel; no other row may change (the GPU test compares the
         other rows bit for bit with the same case without the NaN).
  mask   exact: legacy `nearest`, source index min((int)floorf(i * ((float)n_in / (float)n_out)), n_in - 1) - `src_index`.
  pos    the argument a = count / (last + eps) * scale / dim_t (normalize) or count / dim_t, counts exact.  The kernel rounds eps and
         scale to fp32 (u each, relative, eps's only through last + eps), the table entry (u; the loader rounds the float64 power), and
         the add, the division, the multiplication and the second division (u each: the correctly rounded forms): |a^ - a| <= 8 u |a|,
         which covers (1 + u)^7 - 1.  sin and cos have slope at most 1, so E_pos = 8 u |a| + SINCOS.
         SINCOS = 8 u is the ASSUMED accuracy of the device's sinf / cosf: 4 ulp of a result of magnitude up to 1, the limit OpenCL's full
         profile sets for sin and cos; ROCm's own figure was not available when this was written (the toolchain ships no document that
         states it), so this is an assumption like EXP and DIV of tests/elem_bound.py, next to which it stands.  DESIGN.md section 19 records the worst observed
         |err| / bound.  For scale: the reference's fp32 CPU run of position_encoding.py sits 7.3e-7 (max abs) from its fp64 run on a
         25 x 42 grid with padding.
         A fully padded column or row has count = last = 0: 0 / 1e-6 * scale = 0, sin 0 = 0, cos 0 = 1 - no NaN (`check` asserts it).

Rule: every element has |got - want| <= bound.  The two exact families (tests/detr_neck_cases.py) hold numbers whose products and partial
sums are exact in fp32 in any order: there src is compared BIT FOR BIT with the reference rounded to fp32, whatever the split.

`model()` restates the kernel in fp16 / fp32 with one rounding per operation: x16 = fp16(x), w16 = fp16(W), fp32 accumulation over k in
ascending blocks of 32 from zero per slice (a block's 32 products are summed exactly and rounded once - the MFMA's inner order is not
specified), the slices added in ascending order, the bias last; the mask by `src_index`; pos with every operation of the argument in
fp32 and numpy's sin / cos of the fp32 argument, which are not the device's.  `mutant=` names one of the wrong kernels of `MUTANTS`."""
import numpy as np

from detr_neck_cases import src_index
from elem_bound import DIV, EXP  # noqa: F401  (the assumed figures SINCOS stands beside)

U = 2.0 ** -24
SINCOS = 8 * U          # ASSUMED: 4 ulp at magnitude 1
TOKENS = 32             # tokens of a tile (hoigen_amd/csrc/hg_kernels.h DETR_NECK_TOKENS)
MUTANTS = ("drop_kblock", "truncate_f16", "tile_into_next_image", "bias_twice_split", "index_scale_double", "index_round",
           "cumsum_image_mask", "no_eps", "normalise_by_grid_last", "dim_t_i", "sincos_swapped", "halves_swapped")


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def f16_trunc(a):
    """fp16 by truncation towards zero (a wrong kernel)"""
    a = np.asarray(a, np.float32)
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


def down_mask(c, index=src_index):
    """[B, H, W] bool: the image mask on the feature grid (backbone.py:78)"""
    iy, ix = index(c["H"], c["Hi"]), index(c["W"], c["Wi"])
    return c["image_mask"][:, iy][:, :, ix] != 0


def dim_t64(c):
    i = np.arange(c["D"] // 2)
    return np.float64(c["temperature"]) ** (2.0 * (i // 2) / (c["D"] // 2))


def reference(c):
    """float64 from the unrounded operands -> dict(src [B, S, D], pos [B, S, D], mask [B, S] bool, arg [B, S, D] the sine's argument)"""
    B, Cin, H, W, D = c["B"], c["Cin"], c["H"], c["W"], c["D"]
    x = c["x"].astype(np.float64).reshape(B, Cin, H * W)
    with np.errstate(invalid="ignore"):
        src = x.transpose(0, 2, 1) @ c["w"].astype(np.float64).T + c["bias"].astype(np.float64)
    m = down_mask(c)
    nm = (~m).astype(np.float64)
    ye, xe = nm.cumsum(1), nm.cumsum(2)
    if c["normalize"]:
        ye = ye / (ye[:, -1:, :] + 1e-6) * c["scale"]
        xe = xe / (xe[:, :, -1:] + 1e-6) * c["scale"]
    dt = dim_t64(c)
    ay, ax = ye[..., None] / dt, xe[..., None] / dt
    arg = np.concatenate([ay, ax], -1).reshape(B, H * W, D)
    odd = (np.arange(D) % (D // 2)) % 2 == 1
    pos = np.where(odd, np.cos(arg), np.sin(arg))
    return dict(src=src, pos=pos, mask=m.reshape(B, H * W), arg=arg)


def bounds(c, nsplit=1):
    """per-element bounds of src and pos: dict(src [B, S, D], pos [B, S, D])"""
    B, Cin, H, W = c["B"], c["Cin"], c["H"], c["W"]
    x = np.nan_to_num(c["x"].astype(np.float64).reshape(B, Cin, H * W))
    w = c["w"].astype(np.float64)
    ex, ew = np.abs(f16(np.nan_to_num(c["x"])).astype(np.float64).reshape(B, Cin, H * W) - x), np.abs(f16(c["w"]).astype(np.float64) - w)
    ax, aw = np.abs(x), np.abs(w)
    mm = lambda a, b: a.transpose(0, 2, 1) @ b.T
    T = mm(ax + ex, aw + ew)
    E = mm(ex, aw) + mm(ax, ew) + mm(ex, ew) + Cin * U * T + (nsplit - 1) * U * T * (1 + Cin * U) + \
        U * (T * (1 + Cin * U) + np.abs(c["bias"].astype(np.float64)))
    ref = reference(c)
    return dict(src=E, pos=8 * U * np.abs(ref["arg"]) + SINCOS)


def model(c, nsplit=1, mutant=None):
    """the kernel restated -> dict(src fp32 [B, S, D], pos fp32 [B, S, D], mask bool [B, S])"""
    B, Cin, H, W, D = c["B"], c["Cin"], c["H"], c["W"], c["D"]
    S = H * W
    rnd = f16_trunc if mutant == "truncate_f16" else f16
    with np.errstate(invalid="ignore"):
        x16 = rnd(c["x"]).reshape(B, Cin, S)
    w16 = rnd(c["w"])
    xt = np.ascontiguousarray(x16.transpose(0, 2, 1))      # [B, S, Cin]
    if mutant == "tile_into_next_image":      # tiles over the flat token index b S + s: rows of the next image read on in image b0's memory
        flat = x16.reshape(B, Cin * S)
        for g0 in range(0, B * S, TOKENS):
            b0 = g0 // S
            for g in range(g0, min(g0 + TOKENS, B * S)):
                if g // S != b0:
                    idx = np.minimum(np.arange(Cin) * S + (g - b0 * S), Cin * S - 1)
                    xt[g // S, g % S] = flat[b0, idx]
    ks = Cin // nsplit
    src = None
    with np.errstate(invalid="ignore"):
        for z in range(nsplit):
            acc = np.zeros((B, S, D), np.float32)
            blocks = range(z * ks, (z + 1) * ks, 32)
            if mutant == "drop_kblock" and z == nsplit - 1:
                blocks = list(blocks)[:-1]
            for k0 in blocks:
                p = xt[:, :, k0:k0 + 32].astype(np.float64) @ w16[:, k0:k0 + 32].astype(np.float64).T
                acc = (acc.astype(np.float64) + p).astype(np.float32)
            if mutant == "bias_twice_split" and nsplit > 1:
                acc = acc + c["bias"]
            src = acc if src is None else src + acc
        src = (src + c["bias"]).astype(np.float32)
    index = src_index
    if mutant == "index_scale_double":
        index = lambda n_out, n_in: np.minimum(np.floor(np.arange(n_out) * (n_in / n_out)).astype(np.int64), n_in - 1)
    elif mutant == "index_round":
        index = lambda n_out, n_in: np.minimum(np.rint(np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)
    m = down_mask(c, index)
    f = np.float32
    if mutant == "cumsum_image_mask":      # the cumulative sums run over the image's mask and are sampled afterwards
        nmi = (c["image_mask"] == 0).astype(f)
        iy, ix = src_index(H, c["Hi"]), src_index(W, c["Wi"])
        ye, xe = nmi.cumsum(1, dtype=f)[:, iy][:, :, ix], nmi.cumsum(2, dtype=f)[:, iy][:, :, ix]
    else:
        nm = (~m).astype(f)
        ye, xe = nm.cumsum(1, dtype=f), nm.cumsum(2, dtype=f)
    if c["normalize"]:
        eps = f(0.0) if mutant == "no_eps" else f(1e-6)
        ly, lx = ye[:, -1:, :], xe[:, :, -1:]
        if mutant == "normalise_by_grid_last":
            ly, lx = ye[:, -1:, -1:], xe[:, -1:, -1:]
        with np.errstate(invalid="ignore", divide="ignore"):
            ye = ye / (ly + eps) * f(c["scale"])
            xe = xe / (lx + eps) * f(c["scale"])
    i = np.arange(D // 2)
    dt = (np.float64(c["temperature"]) ** (2.0 * ((i if mutant == "dim_t_i" else i // 2)) / (D // 2))).astype(f)
    ay, ax = (ye[..., None] / dt).astype(f), (xe[..., None] / dt).astype(f)
    halves = [ax, ay] if mutant == "halves_swapped" else [ay, ax]
    arg = np.concatenate(halves, -1).reshape(B, S, D)
    odd = (np.arange(D) % (D // 2)) % 2 == 1
    if mutant == "sincos_swapped":
        odd = ~odd
    with np.errstate(invalid="ignore"):
        pos = np.where(odd, np.cos(arg), np.sin(arg)).astype(f)
    return dict(src=src, pos=pos, mask=m.reshape(B, S))


def worst(got, want, bound):
    """(worst |err| / bound over the finite elements of want, count of violations - a NaN where the reference has none counts)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    err = np.abs(got - want)
    bad = fin & ~(err <= bound)
    bad |= ~fin & ~np.isnan(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(fin & np.isfinite(err), err / bound, 0.0)
    return float(ratio.max(initial=0.0)), int(bad.sum())


def check(c, got, nsplit=1, ref=None, bnd=None):
    """-> (list of failures, dict of worst ratios).  got: dict with src and any of pos, mask (numpy)."""
    ref = ref or reference(c)
    bnd = bnd or bounds(c, nsplit)
    fails, ratios = [], {}
    for k in ("src", "pos"):
        if got.get(k) is None:
            continue
        ratios[k], n_bad = worst(got[k], ref[k], bnd[k])
        if n_bad:
            fails.append(f"{k}: {n_bad} elements outside the bound (worst |err| / bound {ratios[k]:.3g})")
    if got.get("pos") is not None and np.isnan(np.asarray(got["pos"])).any():
        fails.append("pos: NaN")
    if c["feature"] in ("exact_int", "exact_pow2") and not np.array_equal(np.asarray(got["src"], np.float32), ref["src"].astype(np.float32)):
        fails.append("src: an exact family is not bit for bit the reference")
    if got.get("mask") is not None and not np.array_equal(np.asarray(got["mask"]).astype(bool), ref["mask"]):
        fails.append("mask: not equal")
    return fails, ratios
