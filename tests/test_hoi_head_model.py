"""CPU proof of what tests/test_gpu_hoi_head.py asks of hg_hoi_head (tests/hoi_head_bound.py): the fp32 restatement of the set-up and
pooling kernels stays within the derived bound E of roi_bound.definition's float64 mean on every case; the exact family comes out bit
for bit; the screen loses no seeded random box; every mutant is rejected; and the batched arithmetic equals the composition the
per-image loop makes of oracle.roi_oracle -> normalise -> oracle.cache_oracle within the bounds.  Lines HOI_RATIO carry the
restatement's worst |err| / E."""
import functools

import numpy as np
import pytest

import hoi_head_bound as hb
import roi_bound as rb
from oracle import cache_oracle, roi_oracle

P7 = 7
# (name, family, C, H, W, P, scale key, boxes, rule 2)
CASES = [
    ("mixed_14x14", "randn", 80, 14, 14, 7, "1/16", np.concatenate([rb.random_boxes(20, 224, 41), rb.degenerate_boxes(224), hb.beyond_boxes(224), hb.sub_bin_boxes(224)]), True),
    ("mixed_24x24", "randn", 4, 24, 24, 7, "1/14", np.concatenate([rb.random_boxes(40, 336, 42), rb.degenerate_boxes(336), hb.beyond_boxes(336), hb.sub_bin_boxes(336)]), True),
    ("mixed_5x9", "randn", 4, 5, 9, 7, "1/14", np.concatenate([rb.random_boxes(40, 100, 43), rb.degenerate_boxes(100), hb.beyond_boxes(100)]), True),
    ("outlier_24x24", "outlier", 4, 24, 24, 7, "1/14", rb.random_boxes(20, 336, 44), True),
    ("affine_14x14_p2", "affine", 4, 14, 14, 2, "1/16", rb.random_boxes(20, 224, 45), True),
    ("cuts_14x14", "randn", 4, 14, 14, 7, "1/16", rb.on_the_cuts(14, 7, rb.SCALES["1/16"]), False),
    ("ints_p2", "ints", 70, 14, 14, 2, "1/16", rb.dyadic_boxes(rb.SCALES["1/16"], 2), True),
    ("ints_p1", "ints", 4, 24, 24, 1, "1/16", rb.dyadic_boxes(rb.SCALES["1/16"], 1), True),
]
N_RANDOM = {"mixed_14x14": 20, "mixed_24x24": 40, "mixed_5x9": 40, "outlier_24x24": 20, "affine_14x14_p2": 20}
BY_NAME = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def ref_of(name):
    _, fam, C, H, W, P, sk, boxes, _ = BY_NAME[name]
    return hb.reference(rb.make_map(fam, C, H, W), boxes, P, rb.SCALES[sk])


def run(name, mutant=None):
    _, fam, C, H, W, P, sk, boxes, _ = BY_NAME[name]
    return hb.pool(rb.make_map(fam, C, H, W), boxes, P, rb.SCALES[sk], mutant)


@pytest.mark.parametrize("name", [c[0] for c in CASES if c[8]])
def test_restatement_within_bound(name):
    ref, got = ref_of(name), run(name)
    r = hb.worst(got, ref)
    print(f"\nHOI_RATIO {name} restatement: mean {r:.3f} ({int(ref['kept'].sum())} of {len(ref['kept'])} boxes kept)")
    assert r <= 1.0
    n = N_RANDOM.get(name, 0)
    assert int((~ref["kept"][:n]).sum()) == 0, "a seeded random box is screened out"
    assert (~ref["kept"][:n]).mean() <= 0.05 if n else True
    if BY_NAME[name][1] == "ints":
        rb.exactness(rb.make_map(*BY_NAME[name][1:5]), BY_NAME[name][7], BY_NAME[name][5], rb.SCALES[BY_NAME[name][6]])
        assert np.array_equal(got, ref["mean"].astype(np.float32)), "the exact family is not the float64 result rounded once"


def test_agrees_with_roi_align_restatement_within_both_bounds():
    """the separable form against roi_bound.restate's mean (what hg_roi_align returns bit for bit): the two bounds add"""
    for name in ("mixed_14x14", "mixed_5x9"):
        _, fam, C, H, W, P, sk, boxes, _ = BY_NAME[name]
        _, m = rb.restate(rb.make_map(fam, C, H, W), boxes, P, rb.SCALES[sk])
        ref, got = ref_of(name), run(name)
        k = ref["kept"]
        assert (np.abs(got.astype(np.float64) - m)[k] <= (ref["E"] + ref["roi_E"])[k]).all()
        # the boxes off the screen (degenerate, on a cut) still agree to rounding, NaN for NaN
        assert np.allclose(got[~k], m[~k], rtol=1e-4, atol=1e-5, equal_nan=True)


@pytest.mark.parametrize("mutant", hb.POOL_MUTANTS)
def test_pool_mutants_rejected(mutant):
    rejected = []
    for name in ("mixed_14x14", "mixed_5x9", "mixed_24x24"):
        got = run(name, mutant)
        if hb.worst(got, ref_of(name)) > 1.0:
            rejected.append(name)
    assert rejected, f"{mutant} passes rule 2 on every case"
    if mutant == "seam_skipped":
        assert rejected == ["mixed_14x14"], "only the case with more than 64 channels has a seam"


def _batch():
    return hb.make_batch((5, 1, 4, 3), (2, 1, 0, 3), 14, 14, 64, 224, seed=7)


def test_pairs_against_the_reference_expression_and_mutants():
    import torch
    b = _batch()
    want = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    assert list(np.diff(want["pair_off"])) == [8, 0, 0, 6]
    for i, (n, nh) in enumerate(zip(np.diff(b["box_off"]), b["n_human"])):          # upt...:1007-1012
        x, y = torch.meshgrid(torch.arange(int(n)), torch.arange(int(n)), indexing="ij")
        xk, yk = torch.nonzero(torch.logical_and(x != y, x < int(nh))).unbind(1)
        lo, hi = want["pair_off"][i], want["pair_off"][i + 1]
        if nh == 0 or n <= 1:
            assert hi == lo
            continue
        assert np.array_equal(want["pair_h"][lo:hi], xk.numpy()) and np.array_equal(want["pair_o"][lo:hi], yk.numpy())
        bx = torch.from_numpy(b["boxes"][b["box_off"][i]:b["box_off"][i + 1]])
        u = torch.cat([torch.min(bx[xk][..., :2], bx[yk][..., :2]), torch.max(bx[xk][..., 2:], bx[yk][..., 2:])], -1)      # :1019-1023
        assert np.array_equal(want["union_boxes"][lo:hi], u.numpy())
    for m in hb.PAIR_MUTANTS:
        got = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"], m)
        same = all(got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in ("pair_h", "pair_o", "objects", "union_boxes"))
        assert not same, m


def test_head_against_reference_expressions_and_mutants():
    import torch
    b = _batch()
    pr = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    Pt, NC = len(pr["pair_h"]), b["num_classes"]
    rng = np.random.RandomState(3)
    branches = [rng.randn(Pt, NC).astype(np.float32) for _ in range(4)]
    scales = [0.7, 1.3, 2.1, 0.4]
    gx, gy = b["box_off"][pr["image"]] + pr["pair_h"], b["box_off"][pr["image"]] + pr["pair_o"]
    args = (b["scores"][gx], b["scores"][gy], b["labels"][gx], b["labels"][gy], b["obj2target"])
    lg, prior, sc = hb.head(branches, scales, *args, 1.0)
    t = [torch.from_numpy(x) for x in branches]
    want = t[0] * scales[0] + t[1] * scales[1] + t[2] * scales[2] + t[3] * scales[3]                  # :1195-1196
    assert np.array_equal(lg, want.numpy())
    ph = torch.zeros(Pt, NC)                                                                          # :806-833 at p = 1
    po = torch.zeros(Pt, NC)
    tgt = [np.nonzero(b["obj2target"][o])[0].tolist() for o in b["labels"][gy]]
    pi = [i for i, tar in enumerate(tgt) for _ in tar]
    fl = [k for tar in tgt for k in tar]
    ph[pi, fl] = torch.from_numpy(b["scores"][gx])[pi]
    po[pi, fl] = torch.from_numpy(b["scores"][gy])[pi]
    assert np.array_equal(prior, torch.stack([ph, po]).numpy())
    want_sc = torch.sigmoid(want) * torch.stack([ph, po]).prod(0)                                     # :1417-1423, dense
    assert np.allclose(sc, want_sc.numpy(), rtol=1e-6, atol=0)
    _, p28, s28 = hb.head(branches, scales, *args, 2.8)
    p64 = np.where(prior > 0, np.stack([b["scores"][gx], b["scores"][gy]]).astype(np.float64)[:, :, None] ** float(np.float32(2.8)), 0.0)
    assert (np.abs(p28 - p64) <= hb.prior_bound(p64)).all()
    w, e = hb.score_bound(lg, p64)
    assert (np.abs(s28 - w) <= e).all()
    for m in hb.HEAD_MUTANTS:
        lg_m, pr_m, sc_m = hb.head(branches, scales, *args, 2.8, m)
        assert not (np.array_equal(lg_m, lg) and np.array_equal(pr_m, p28)) or (np.abs(sc_m - w) > e).any(), m
        assert (np.abs(sc_m - w) > e).any(), f"{m}: the scores stay within the bound"


def test_batched_arithmetic_is_the_per_image_composition():
    """pool -> x / ||x|| -> cache logits of the batch against oracle.roi_oracle -> normalise -> oracle.cache_oracle image by image"""
    b = _batch()
    pr = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    rng = np.random.RandomState(5)
    S, C, NC = 48, b["C"], b["num_classes"]
    w = rng.randn(S, C).astype(np.float32)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    lab = (rng.uniform(size=(S, NC)) < 0.2).astype(np.float32)
    lens = np.maximum(lab.sum(0), 1).astype(np.float32)
    scale = rb.SCALES["1/16"]
    for i in range(b["B"]):
        lo, hi = pr["pair_off"][i], pr["pair_off"][i + 1]
        if hi == lo:
            continue
        ub = pr["union_boxes"][lo:hi]
        got = hb.pool(b["feat"][i], ub, P7, scale)
        ref = hb.reference(b["feat"][i], ub, P7, scale)
        want = roi_oracle.roi_align_mean(b["feat"][i], ub, 7, float(scale))
        k = ref["kept"]
        assert k.any()
        assert (np.abs(got.astype(np.float64) - want)[k] <= (ref["E"] + ref["roi_E"])[k]).all()
        gn, wn = got[k] / np.linalg.norm(got[k], axis=1, keepdims=True), want[k] / np.linalg.norm(want[k], axis=1, keepdims=True)
        a = cache_oracle.cache_logits(gn, w, -np.ones(S, np.float32), lab, lens)
        o = cache_oracle.cache_logits(wn, w, -np.ones(S, np.float32), lab, lens)
        # |d logits| <= sum_s |d phi| labels / lens, |d phi| <= |d feature| . |w| <= |d feature| (unit rows); d feature from E through the norm
        dn = 2.0 * np.linalg.norm((ref["E"] + ref["roi_E"])[k], axis=1) / np.linalg.norm(want[k], axis=1) + 1e-6
        assert (np.abs(a - o) <= dn[:, None] * (lab.sum(0) / lens)[None] + 1e-5).all()
