"""The test references of the DINO branch (tests/dino_bound.py, with oracle/cache_oracle.py for the cache models) against
tests/golden/g24_dino_branch.npz: the outputs of the reference's own statements - the network call and the normalisation of its rows,
the per-image cache logits, the global branch, the six-term sum, utils.build_dino_cache_model - executed on seeded inputs
(tests/golden/make_golden_dino_branch.py, README_dino_branch.md).  No GPU, and the reference tree is not read."""
import os
import sys

import numpy as np
import pytest
import torch

import dino_bound as db
import elem_bound as eb
import hoi_head_bound as hb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import dino_branch_cases as dc  # noqa: E402
import hoi_head_cases as hc  # noqa: E402
from hoigen_amd import cache_model  # noqa: E402
from oracle import cache_oracle  # noqa: E402

G = np.load(os.path.join(GOLDEN, "g24_dino_branch.npz"))
G14 = np.load(os.path.join(GOLDEN, "g14_hoi_head.npz"))
SCALE_NAMES = ("gen_logit_scale_H", "gen_logit_scale_O", "gen_logit_scale_U", "logit_scale_text", "clip_cache_logit", "dino_cache_logit")


def test_the_cases_regenerate_the_fixtures_network():
    """the seeded network on the seeded views gives the fixture's map (to the rounding of a convolution library, not to bits)"""
    net = dc.dino_net()
    with torch.no_grad():
        fmap = net.net(torch.from_numpy(dc.views()))
    assert tuple(fmap.shape) == (dc.B, dc.K_DINO, 2, 2)
    got = fmap.permute(0, 2, 3, 1).reshape(dc.B, 4, dc.K_DINO).numpy()
    assert np.allclose(got, G["map_nhwc"], rtol=1e-4, atol=1e-5)


def test_pooled_and_normalised_rows():
    """restatement against :1617-1618 on the fixture's own map.  The fixture's rows are fp32 too - a sum of HW terms in the library's
    order and one division; a sum of squares, a square root and a division - so each side is within the bound of the float64 value
    and the two are within twice the bound of each other."""
    x = G["map_nhwc"]
    want, B = db.pool_reference(x)
    assert eb.worst(G["pooled"], want, B) <= 1.0, "the fixture's own pooled rows are outside the bound of their float64 mean"
    got = db.pool_model(x)
    assert eb.worst(got, want, B) <= 1.0 and (np.abs(got.astype(np.float64) - G["pooled"]) <= 2 * B).all()
    want_n, Bn = eb.l2_reference(G["pooled"])
    assert eb.worst(G["features"], want_n, Bn) <= 1.0
    assert eb.worst(db.normalize_model(G["pooled"]), want_n, Bn) <= 1.0
    assert (np.abs(db.normalize_model(G["pooled"]).astype(np.float64) - G["features"]) <= 2 * Bn).all()


def six_terms(i, mutant=None, dino_bias=True):
    """the restatement's inputs of image i: (branch rows, per-image flags, scales, image of pair, scores x, y, labels x, y)"""
    w, c, im = hc.weights(), dc.caches(), hc.image(i)
    x, y = G14[f"x_keep_{i}"], G14[f"y_keep_{i}"]
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)      # noqa: E731
    h, o, u = unit(G14[f"pooled_single_{i}"][x]), unit(G14[f"pooled_single_{i}"][y]), unit(G14[f"pooled_union_{i}"])
    rows = [cache_oracle.cache_logits(f, w[f"w_{k}"], w[f"b_{k}"], w[f"label_{k}"], w[f"lens_{k}"]) for f, k in ((h, "H"), (o, "O"), (u, "U"))]
    rows.append(cache_oracle.linear_logits(u, w["w_text"]))
    rows.append(cache_oracle.cache_logits(unit(dc.feat_global()), c["global_cache"].T, c["global_bias"], c["global_values"], c["global_len"]))
    rows.append(cache_oracle.cache_logits(G["features"], c["dino_cache"].T, c["dino_bias"] if dino_bias else 0 * c["dino_bias"], c["dino_values"], c["dino_len"]))
    return rows, [False] * 4 + [True, True], [dc.SCALES[k] for k in SCALE_NAMES], np.full(len(x), i), im["scores"][x], im["scores"][y], im["labels"][x], im["labels"][y]


def o2t():
    t = np.zeros((hc.N_OBJ, hc.NC), np.uint8)
    for o, tar in enumerate(hc.weights()["obj2target"]):
        t[o, tar] = 1
    return t


def test_logits_like_the_interaction_head_fixture():
    """:1112-1115, :1133-1138 and the six-term sum :1206-1207, held the way tests/test_hoi_head_golden.py holds g14 (its rtol / atol)"""
    for i in range(dc.B):
        args = six_terms(i)
        assert np.allclose(args[0][5], G["dino_cache_logits"], rtol=1e-5, atol=1e-5)
        assert np.allclose(db.broadcast(args[0][4], args[3]), G[f"logits_global_{i}"], rtol=1e-5, atol=1e-5)
        lg = db.head(*args, o2t(), hc.HYPER_LAMBDA)[0]
        assert lg.shape == G[f"logits_{i}"].shape == (hc.HUMANS[i] * (hc.SIZES[i] - 1), hc.NC)
        assert np.allclose(lg, G[f"logits_{i}"], rtol=1e-5, atol=1e-5)


# (image_branch_summed_first moves only the last bits of an fp32 sum: it is held bit for bit by tests/test_dino_model.py and on the device,
# and a tolerance of 1e-5 cannot see it)
@pytest.mark.parametrize("mutant", [m for m in db.HEAD_MUTANTS if m != "image_branch_summed_first"])
def test_head_mutants_rejected_by_the_fixture(mutant):
    rejected = []
    for i in range(dc.B):
        if mutant == "image_bias_dropped":
            lg = db.head(*six_terms(i, dino_bias=False), o2t(), hc.HYPER_LAMBDA)[0]
        else:
            args = six_terms(i)
            args = (args[0], [False] * 5 + [True]) + args[2:]      # the DINO branch alone is the per-image one the mutants touch
            args[0][4] = db.broadcast(args[0][4], args[3])
            lg = db.head(*args, o2t(), hc.HYPER_LAMBDA, mutant=mutant)[0]
        if not np.allclose(lg, G[f"logits_{i}"], rtol=1e-5, atol=1e-5):
            rejected.append(i)
    assert rejected, f"{mutant} agrees with the fixture on every image"


def test_build_dino_cache_model_equals_the_references_keys_and_values():
    """utils.build_dino_cache_model executed (the fixture) against cache_model.build_dino_cache_model under the same torch.manual_seed:
    equal, the random keys of the two empty classes included"""
    feats, verbs = dc.build_inputs()
    torch.manual_seed(dc.SEED)
    keys, values = cache_model.build_dino_cache_model(torch.from_numpy(feats), verbs, dc.C_BUILD, dc.SHOT)
    assert torch.equal(keys, torch.from_numpy(G["cache_keys"])) and torch.equal(values, torch.from_numpy(G["cache_values"]))
    assert keys.shape == (dc.D_BUILD, dc.C_BUILD * dc.SHOT)
    assert float(np.abs(feats).max()) > 4.0 and np.allclose(np.linalg.norm(G["cache_keys"], axis=0), 1.0, atol=1e-6)      # raw rows in, unit keys out
