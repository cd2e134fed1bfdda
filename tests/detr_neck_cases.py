"""Seeded inputs of the DETR neck (hoigen_amd/csrc/hg_detr_neck.hip; the reference's input_proj, PositionEmbeddingSine and the mask
interpolation: detr/models/detr.py:40, :65, position_encoding.py:28-48, backbone.py:78) for tests/detr_neck_bound.py, the fixture
tests/golden/g21_detr_neck.npz and the tests that use them.  numpy only (`Generator`).  No GPU, no library.

A case is a dict: x [B, Cin, H, W] fp32 (the body's map), w [D, Cin] and bias [D] fp32 (input_proj), image_mask [B, Hi, Wi] uint8 (non-zero
= padded) and the embedding's settings.

Feature families (`FEATURES`):
    relu        post-ReLU-like: max(randn, 0), half of the values zero; Xavier-uniform w, 0.1 randn bias
    outlier     relu with every 29th channel times 60
    cancel      the second half of the channels equal to the first plus 2^-7 randn, the second half of every row of w minus the first
                plus an eighth of a Xavier draw: products tens of times what they leave
    exact_int   x integers / 4 in [-1, 1], w integers / 2 in [-1, 1], bias integers / 8: every product and partial sum is a multiple of
                2^-3 below 2^13, exact in fp32 in any order
    exact_pow2  x, w and bias +-2^-e, e in 0 .. 3: multiples of 2^-6 below 2^12
    nan_token   relu with all channels of ONE token of image 0 NaN (`nan_at`)

Mask families (`MASKS`), with Hi = 32 H - 13 and Wi = 32 W - 7 (no multiples of 32) except where said:
    none        nothing padded
    rect        right / bottom rectangles from per-image sizes, as a NestedTensor has them (image 0 is full size)
    random      random bytes, a third of them zero: arbitrary masks, and any non-zero byte counts as padded
    dead_image  rect with the last image fully padded
    cross       one interior row and one interior column of the feature grid fully padded in every image (where H, W >= 3), rect besides
    small       Hi = max(H - 1, 1), Wi = max(W - 2, 1): an image mask smaller than the grid; random bytes"""
import numpy as np

FEATURES = ("relu", "outlier", "cancel", "exact_int", "exact_pow2", "nan_token")
EXACT_FEATURES = ("exact_int", "exact_pow2")
MASKS = ("none", "rect", "random", "dead_image", "cross", "small")

# the fixture's case (tests/golden/make_golden_detr_neck.py): three images padded to 200 x 270, a 7 x 9 grid
G21 = dict(Cin=2048, D=256, B=3, H=7, W=9, Hi=200, Wi=270, sizes=((200, 270), (150, 270), (200, 181)), seed=21)


def src_index(n_out, n_in):
    """legacy `nearest`: the source index of every output index, min((int)floorf(i * ((float)n_in / (float)n_out)), n_in - 1)"""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def rect_mask(B, Hi, Wi, sizes):
    m = np.ones((B, Hi, Wi), np.uint8)
    for b, (h, w) in enumerate(sizes):
        m[b, :h, :w] = 0
    return m


def make_mask(family, B, H, W, r):
    Hi, Wi = (max(H - 1, 1), max(W - 2, 1)) if family == "small" else (32 * H - 13, 32 * W - 7)
    if family == "none":
        m = np.zeros((B, Hi, Wi), np.uint8)
    elif family in ("random", "small"):
        m = r.integers(0, 256, (B, Hi, Wi)).astype(np.uint8) * (r.random((B, Hi, Wi)) > 1 / 3)
    else:
        sizes = [(Hi, Wi)] + [(int(r.integers(Hi // 2 + 1, Hi + 1)), int(r.integers(Wi // 2 + 1, Wi + 1))) for _ in range(B - 1)]
        m = rect_mask(B, Hi, Wi, sizes)
        if family == "dead_image":
            m[B - 1] = 1
        if family == "cross":
            if H >= 3:
                m[:, src_index(H, Hi)[H // 2], :] = 1
            if W >= 3:
                m[:, :, src_index(W, Wi)[W // 2]] = 1
    return np.ascontiguousarray(m, np.uint8), Hi, Wi


def make_features(family, B, Cin, H, W, D, r):
    n = lambda *s: r.standard_normal(s)
    xav = lambda o, i: r.uniform(-1, 1, (o, i)) * np.sqrt(6.0 / (o + i))
    nan_at = None
    if family == "exact_int":
        x, w, bias = r.integers(-4, 5, (B, Cin, H, W)) / 4, r.integers(-2, 3, (D, Cin)) / 2, r.integers(-8, 9, D) / 8
    elif family == "exact_pow2":
        p2 = lambda *s: r.choice([-1.0, 1.0], s) * 2.0 ** -r.integers(0, 4, s)
        x, w, bias = p2(B, Cin, H, W), p2(D, Cin), p2(D)
    else:
        x, w, bias = np.maximum(n(B, Cin, H, W), 0), xav(D, Cin), 0.1 * n(D)
        if family == "outlier":
            x[:, ::29] *= 60
        elif family == "cancel":
            x[:, Cin // 2:] = x[:, :Cin // 2] + 2.0 ** -7 * n(B, Cin // 2, H, W)
            w[:, Cin // 2:] = -w[:, :Cin // 2] + 0.125 * xav(D, Cin // 2)
        elif family == "nan_token":
            nan_at = (0, (H * W) // 2)
            x.reshape(B, Cin, H * W)[nan_at[0], :, nan_at[1]] = np.nan
    return x, w, bias, nan_at


def make_case(feature, mask, B, Cin, H, W, D, seed, normalize=True, temperature=10000.0, scale=None):
    r = np.random.default_rng([seed, B, Cin, H, W, D, FEATURES.index(feature), MASKS.index(mask)])
    x, w, bias, nan_at = make_features(feature, B, Cin, H, W, D, r)
    m, Hi, Wi = make_mask(mask, B, H, W, r)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f32(x), w=f32(w), bias=f32(bias), image_mask=m, B=B, Cin=Cin, H=H, W=W, D=D, Hi=Hi, Wi=Wi, feature=feature, mask=mask,
                nan_at=nan_at, normalize=bool(normalize), temperature=float(temperature),
                scale=float(2 * np.pi if scale is None else scale))


def g21_case():
    """the fixture's inputs: relu features, the rectangles of G21's sizes"""
    g = G21
    r = np.random.default_rng([g["seed"], 0])
    x, w, bias, _ = make_features("relu", g["B"], g["Cin"], g["H"], g["W"], g["D"], r)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(x=f32(x), w=f32(w), bias=f32(bias), image_mask=rect_mask(g["B"], g["Hi"], g["Wi"], g["sizes"]), B=g["B"], Cin=g["Cin"],
                H=g["H"], W=g["W"], D=g["D"], Hi=g["Hi"], Wi=g["Wi"], feature="relu", mask="rect", nan_at=None, normalize=True,
                temperature=10000.0, scale=float(2 * np.pi))
