"""tests/golden/g20_detr_heads.npz (the reference's own class_embed, bbox_embed(...).sigmoid() and PostProcess in fp32 on hs_last of
g19_detr_transformer.npz, recorded by tests/golden/make_golden_detr_heads.py) against tests/detr_heads_bound.py on the CPU: the float64
`reference()` reproduces the fixture to 1e-5 relative (the reference's fp32 run sits at most 5.7e-7 from its own fp64 run, as the
generator prints: tests/golden/README_detr_heads.md) with every label equal, and the fp16 / fp32 restatement `model()` of the kernel is
inside `bounds()` of it, element by element, with the fixture's own fp32 distance from fp64 allowed on top.  CPU only."""
import os

import numpy as np

import detr_decoder_cases as dd
import detr_heads_bound as hb
import detr_heads_cases as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the fixture's largest distance from the reference's fp64 run, per output, as the generator prints it (README_detr_heads.md), times four
FIXTURE_ERR = dict(logits=4 * 2.62e-6, pred_boxes=4 * 2.77e-7, scores=4 * 1.21e-7, boxes=4 * 1.63e-4)


def case():
    g = hc.G20
    hs = np.load(os.path.join(GOLDEN, "g19_detr_transformer.npz"))["hs_last"]
    return hc.as_case(hc.weights(g["D"], g["C1"], g["wseed"]), hs[None], g["sizes"])


def test_the_reference_reproduces_the_fixture():
    fix, ref = np.load(os.path.join(GOLDEN, "g20_detr_heads.npz")), hb.reference(case())
    assert sorted(fix.files) == ["boxes", "labels", "logits", "pred_boxes", "scores"]
    assert fix["logits"].shape == (3, 100, 92) and fix["pred_boxes"].shape == (3, 100, 4) and fix["boxes"].shape == (3, 100, 4)
    assert fix["labels"].dtype == np.int64 and fix["scores"].dtype == np.float32
    for k, want in (("logits", ref["logits"][0]), ("pred_boxes", ref["pred_boxes"][0]), ("scores", ref["scores"][..., None]), ("boxes", ref["boxes"])):
        e, r = dd.rel_l2(want, fix[k].reshape(want.shape))
        print(f"{k}: float64 reference vs fixture rel L2 {e:.2e}, worst row {r:.2e}")
        assert e < 1e-5 and r < 1e-5
    assert np.array_equal(ref["labels"], fix["labels"])
    # the seeded decoder's queries end close to one another: three classes share the maxima; never the no-object column
    assert len(set(fix["labels"].reshape(-1).tolist())) >= 3 and fix["labels"].max() < 91


def test_the_restatement_is_inside_the_bound_of_the_fixture():
    c = case()
    fix, bnd, m = np.load(os.path.join(GOLDEN, "g20_detr_heads.npz")), hb.bounds(c), hb.model(c)
    for k in ("logits", "pred_boxes", "boxes"):
        got, b = (m[k][0], bnd[k][0]) if k != "boxes" else (m[k], bnd[k])
        r = hb.worst_ratio(got, fix[k].astype(np.float64), b + FIXTURE_ERR[k])
        print(f"{k}: restatement vs fixture worst |err| / bound {r:.3f}")
        assert r <= 1.0
    ref = hb.reference(c)
    amb, r, fails = hb.check_labels(dict(ref, prob=ref["prob"]), dict(bnd, prob=bnd["prob"] + FIXTURE_ERR["scores"]), m["labels"], m["scores"])
    print(f"labels: {amb:.1%} of the rows ambiguous; scores worst |err| / bound {r:.3f}")
    assert not fails and amb <= hb.MAX_AMBIGUOUS
    clear = m["labels"] == fix["labels"]
    assert clear.mean() >= 1 - amb
    e = dd.rel_l2(m["logits"][0].reshape(-1, 92), fix["logits"].reshape(-1, 92))[0]
    assert e < 1e-3, e


def test_weights_carry_the_detector_key_names():
    sd = hc.weights(128, 17, 20)
    assert sorted(sd) == sorted(["class_embed.weight", "class_embed.bias"] + [f"bbox_embed.layers.{i}.{k}" for i in range(3) for k in ("weight", "bias")])
    assert sd["class_embed.weight"].shape == (17, 128) and sd["bbox_embed.layers.2.weight"].shape == (4, 128) and sd["bbox_embed.layers.1.bias"].shape == (128,)
