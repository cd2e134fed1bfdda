"""The float64 restatement of tests/detr_neck_bound.py against the reference's own fp32 outputs (tests/golden/g21_detr_neck.npz, made by
tests/golden/make_golden_detr_neck.py from the reference's statements): src and pos to 1e-5, the mask equal; the fp16 / fp32 restatement
of the kernel inside its bound of that reference.  No GPU, no library."""
import os

import numpy as np

import detr_neck_bound as nb
import detr_neck_cases as nc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_float64_restatement_is_the_reference():
    g = np.load(os.path.join(GOLDEN, "g21_detr_neck.npz"))
    c = nc.g21_case()
    ref = nb.reference(c)
    assert g["src"].shape == (3, 63, 256) and g["src"].dtype == np.float32 and g["mask"].dtype == np.bool_
    for k in ("src", "pos"):
        d = float(np.abs(ref[k] - g[k]).max())
        print(f"DETR_NECK g21 {k}: float64 restatement against the reference's fp32 run, max abs {d:.2e} "
              f"(its fp32 run against fp64: {float(g[k + '_fp32_vs_fp64_max_abs']):.2e})")
        assert d < 1e-5
    assert np.array_equal(ref["mask"], g["mask"])
    assert g["mask"][0].sum() == 0 and g["mask"][1].any() and g["mask"][2].any()      # image 0 is full size, the others are padded


def test_the_kernels_restatement_is_inside_the_bound_of_the_fixtures_case():
    c = nc.g21_case()
    for nsplit in (1, 8):
        fails, ratios = nb.check(c, nb.model(c, nsplit), nsplit)
        assert not fails, fails
