"""What the tests ask of the DINO branch: the pool + normalise kernel behind the last ResNet block (hoigen_amd/csrc/hg_resnet_pool.hip,
hg_resnet_features) and the per-image branch source of hg_hoi_head (HG_HOI_SRC_IMAGE).  numpy / torch on the CPU; no GPU, no library.

Pool (`pool_model`, expected BIT FOR BIT).  Per (image, channel) one fp32 accumulator from 0, the HW positions of the NHWC map added in
ascending order, one IEEE division by float32(HW).  Adds only: a contraction has nothing to fuse.

Pooled mean against float64 (`pool_reference`).  With n = HW, u = 2^-24, A = the float64 mean of |x| over the positions: the sequential
sum of n terms is off by at most gamma_{n-1} sum |x| (Higham, gamma_k = k u / (1 - k u)); the division rounds once more: u |S / n| on
the exact quotient and a factor (1 + u) on the sum's error.  |S| / n <= A, so
    |got - want| <= A (gamma_{n-1} (1 + u) + u) <= A (n + 1) u      whenever (n - 1)(n + 1) u <= 1, i.e. n <= 4096,
which `pool_reference` asserts.  B_pool = A (HW + 1) 2^-24.  No measured value enters.

Normalised rows: elem_bound.l2_reference on the fp32 pooled rows the SAME call returned ("D terms any order", sqrtf, 1 / ., one
multiply) - the kernel's sum of squares is fused per thread, a 64-lane butterfly, then the waves in order; the bound holds for any order.

Image logits: heads_bound.cache_reference at K = K_img on the rows of feat_image (`image_case` builds its dict).

The head with per-image branches (`head`): an image branch's [B, NC] rows are broadcast to the pairs by the pair's image, then
hoi_head_bound.head sums scale_i * branch_i left to right in LIST order.  Expected bit for bit.

Mutants (tests/test_dino_model.py proves each is rejected by one of the rules above on the committed cases): MUTANTS.

Worst |err| / bound measured on an MI355X (recorded, not tuned to; the tests assert <= 1):

RECORDED (lines DINO_RATIO of tests/test_gpu_resnet_features.py and tests/test_gpu_hoi_dino_branch.py)
    (B, HW, C)         pooled    features          image_logits (worst of both batches)
    (1, 1, 64)         0.000     0.033             K_img 64,   S 5, bias -1     0.816
    (3, 49, 2048)      0.114     0.003             K_img 2048, S 300            0.012
    (2, 50, 320)       0.090     0.017             K_img 2048, S 5, bias -1     0.080
    (64, 4, 128)       0.390     0.038             K_img 64,   linear           0.006
    (2, 1025, 64)      0.020     0.045
    end to end on g24 (rows 5.8e-4 relative L2 from the fixture's): logits 0.016 - the 1e-3 contract term is most of that bound
    facade, small ResNet at 2 x 3 x 64 x 64 and 3 x 3 x 33 x 47: features 0.006; ResNet-50 at 2 x 3 x 224 x 224: 3.5e-4, 3.6e-4 relative L2
pooled sits far below 1 because the gamma bound is the worst case over every sign pattern of n roundings; (64, 4, 128) is closest: with
four positions there is little for the roundings to average over.
"""
import numpy as np

import elem_bound as eb
import hoi_head_bound as hb

U = 2.0 ** -24
F = np.float32
CH_STRIDE = 256      # hg_resnet_pool.hip: a thread's channels lie RESNET_POOL_THREADS apart (hoigen_amd._lib.HG_RESNET_POOL_THREADS)
POOL_MUTANTS = ("last_position_dropped", "mean_over_hw_plus_1", "nchw_read_as_nhwc", "channel_seam_skipped")
NORM_MUTANTS = ("norm_without_sqrt", "norm_over_batch")
HEAD_MUTANTS = ("image_row_by_pair", "image_row_next", "image_branch_summed_first", "image_scale_dropped", "image_bias_dropped")
MUTANTS = POOL_MUTANTS + NORM_MUTANTS + HEAD_MUTANTS
# (B, HW, C) of the kernel tests: one position and one wave; ResNet-50's 7 x 7 x 2048; a width that is no multiple of the workgroup;
# the largest batch; more positions than a workgroup has threads
SHAPES = ((1, 1, 64), (3, 49, 2048), (2, 50, 320), (64, 4, 128), (2, 1025, 64))
FAMILIES = ("randn", "relu", "ints", "cancel", "outlier", "zero_image", "nan_image")


def make_map(family, B, HW, C, seed=24):
    """x [B, HW, C] float32 NHWC, seeded.  `ints`: integers in -8 .. 8 - every partial sum is exact, and where HW is a power of two so
    is the mean (is_exact)."""
    g = np.random.default_rng((FAMILIES.index(family) * 1009 + B) * 1013 * 1019 + HW * 1021 + C + seed)
    x = g.standard_normal((B, HW, C))
    if family == "relu":
        x = np.maximum(x, 0.0)
    elif family == "ints":
        x = g.integers(-8, 9, (B, HW, C)).astype(np.float64)
    elif family == "cancel":      # large +- pairs in neighbouring positions with a remainder 1e-3 of their size
        big = 1000.0 * (1.0 + g.random((B, (HW + 1) // 2, C)))
        x = np.concatenate([big, -big * (1.0 + 1e-3 * g.standard_normal(big.shape))], 1)[:, :HW]
        x = x[:, g.permutation(HW)]
    elif family == "outlier":     # one channel carries 1e4 times the rest
        x = np.maximum(x, 0.0)
        x[:, :, C // 3] *= 1e4
    elif family == "zero_image":
        x = np.maximum(x, 0.0)
        x[B - 1] = 0.0
    elif family == "nan_image":
        x = np.maximum(x, 0.0)
        x[B // 2, HW // 2, (C // 2) + 1] = np.nan
    return np.ascontiguousarray(x, F)


def is_exact(family, HW):
    """every partial sum is an integer below 2^24 and the division is by a power of two: pooled is the float64 mean, bit for bit"""
    return family == "ints" and HW & (HW - 1) == 0


def special_image(family, B):
    return {"zero_image": B - 1, "nan_image": B // 2}.get(family)


def pool_model(x, mutant=None):
    """fp32 restatement of the pool: sequential adds in ascending position order, one division -> pooled [B, C] float32"""
    assert mutant is None or mutant in POOL_MUTANTS, mutant
    x = np.asarray(x, F)
    B, HW, C = x.shape
    if mutant == "nchw_read_as_nhwc":      # the same memory, taken for [B, C, HW]
        x = np.ascontiguousarray(x.reshape(B, C, HW).transpose(0, 2, 1))
    acc = np.zeros((B, C), F)
    with np.errstate(all="ignore"):
        for p in range(HW - 1 if mutant == "last_position_dropped" else HW):
            acc = acc + x[:, p, :]
        out = (acc / F(HW + 1 if mutant == "mean_over_hw_plus_1" else HW)).astype(F)
    if mutant == "channel_seam_skipped" and C > CH_STRIDE:
        out[:, CH_STRIDE] = 0.0
    return out


def pool_reference(x):
    """(want, B_pool) float64 [B, C]"""
    x = np.asarray(x, np.float64)
    HW = x.shape[1]
    assert (HW - 1) * (HW + 1) * U <= 1.0, "the bound's second-order terms need HW <= 4096"
    return x.mean(1), np.abs(x).mean(1) * (HW + 1) * U


def normalize_model(pooled, mutant=None):
    """fp32 statement of the norm on pooled rows (one order of the sum; held to l2_reference's bound, not to bits)"""
    assert mutant is None or mutant in NORM_MUTANTS, mutant
    p = np.asarray(pooled, F)
    with np.errstate(all="ignore"):
        q = (p * p).sum(0 if mutant == "norm_over_batch" else 1, dtype=F)
        n = q if mutant == "norm_without_sqrt" else np.sqrt(q)
        inv = F(1.0) / n
        return (p * (inv[None, :] if mutant == "norm_over_batch" else inv[:, None])).astype(F)


def worst_pool(got, x):
    want, B = pool_reference(x)
    return eb.worst(got, want, B)


def worst_norm(features, pooled, rows=None):
    """worst |features - l2(pooled)| / elem_bound's bound over `rows` (default: all) of the fp32 pooled rows"""
    rows = np.arange(len(pooled)) if rows is None else np.asarray(rows)
    want, B = eb.l2_reference(np.asarray(pooled)[rows])
    return eb.worst(np.asarray(features)[rows], want, B)


# ---- the head with per-image branches -------------------------------------------------------------------------------------------------
def image_case(f, w, b, lab, lens):
    """heads_bound's cache dict for feat_image rows f [B, K] (torch float32 CPU tensors); lab None: a plain linear slot"""
    import torch
    S, K = w.shape
    has = lab is not None
    return {"family": "unit", "R": int(f.shape[0]), "S": int(S), "C": int(lab.shape[1]) if has else 0, "K": int(K), "has_labels": has,
            "post_div": 1.0, "f": f.float().contiguous(), "w": w.float().contiguous(),
            "b": (b if b is not None else torch.zeros(S)).float().contiguous(),
            "lab": lab.float().contiguous() if has else torch.zeros(S, 1), "lens": lens.float().contiguous() if has else torch.ones(1)}


def image_logits_model(c, mutant=None):
    """hg_cache_logits on the B rows as heads_bound.cache_model restates it -> float32 numpy [B, NC]"""
    import heads_bound as hdb
    if mutant == "image_bias_dropped":
        c = dict(c, b=c["b"] * 0)
    return hdb.cache_model(c).numpy()


def broadcast(rows, image_of_pair, mutant=None):
    """[B, NC] -> [Pt, NC]: pair p reads the row of its image"""
    rows = np.asarray(rows, F)
    idx = np.asarray(image_of_pair, np.int64)
    if mutant == "image_row_by_pair":
        idx = np.arange(len(idx)) % len(rows)
    elif mutant == "image_row_next":
        idx = (idx + 1) % len(rows)
    return rows[idx]


def head(branches, per_image, scales, image_of_pair, scores_x, scores_y, labels_x, labels_y, obj2target, p, mutant=None):
    """hoi_head_bound.head with the per-image branches (per_image[i] true: branches[i] is [B, NC]) handed over as their broadcast rows"""
    assert mutant is None or mutant in HEAD_MUTANTS, mutant
    slabs = [broadcast(br, image_of_pair, mutant) if pi else np.asarray(br, F) for br, pi in zip(branches, per_image)]
    scales = [F(1.0) if (pi and mutant == "image_scale_dropped") else s for s, pi in zip(scales, per_image)]
    if mutant == "image_branch_summed_first":
        order = [i for i, pi in enumerate(per_image) if pi] + [i for i, pi in enumerate(per_image) if not pi]
        slabs, scales = [slabs[i] for i in order], [scales[i] for i in order]
    return hb.head(slabs, scales, scores_x, scores_y, labels_x, labels_y, obj2target, p)
