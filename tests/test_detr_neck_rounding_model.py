"""The bound of tests/detr_neck_bound.py proved on the CPU: the restatement of the neck kernel (`model()`) stays inside the per-element
bound of the float64 reference for every feature and mask family, the exact families bit for bit, and each of twelve wrong kernels
(`MUTANTS`) is rejected by the bound, by an exact family or by the mask comparison on at least one of the cases the GPU test runs at
its small shapes.  No GPU, no library."""
import numpy as np
import pytest

import detr_neck_bound as nb
import detr_neck_cases as nc

SEED = 21
SHAPE = dict(B=2, Cin=128, H=7, W=9, D=128)      # 63 tokens an image: the second tile is ragged and a flat tiling would mix images


def _cases():
    out = []
    for i, feat in enumerate(nc.FEATURES):
        for j, mask in enumerate(nc.MASKS):
            out.append(nc.make_case(feat, mask, seed=SEED, normalize=(i + j) % 3 != 0, **SHAPE))
    return out


CASES = _cases()


def _double_index_case():
    """a grid height and an image height at which the index scale in double picks another source row than the scale in fp32"""
    for n_in in range(2, 1400):
        for n_out in (-(-n_in // 32) - 1, -(-n_in // 32), -(-n_in // 32) + 1):
            if n_out < 1:
                continue
            dbl = np.minimum(np.floor(np.arange(n_out) * (n_in / n_out)).astype(np.int64), n_in - 1)
            if not np.array_equal(dbl, nc.src_index(n_out, n_in)):
                return n_out, n_in
    return None


def test_restatement_is_inside_the_bound():
    top = {"src": 0.0, "pos": 0.0}
    for c in CASES:
        for nsplit in (1, 2):
            fails, ratios = nb.check(c, nb.model(c, nsplit), nsplit)
            assert not fails, (c["feature"], c["mask"], nsplit, fails)
            for k, v in ratios.items():
                top[k] = max(top[k], v)
    print(f"DETR_NECK_MODEL worst |err| / bound of the restatement: src {top['src']:.3f}, pos {top['pos']:.3f}")


def test_fully_padded_column_gives_zero_not_nan():
    c = next(c for c in CASES if c["mask"] == "dead_image" and c["normalize"])
    ref = nb.reference(c)
    assert ref["mask"][-1].all() and np.isfinite(ref["pos"]).all()
    half = c["D"] // 2
    assert np.array_equal(ref["pos"][-1][:, 0:half:2], np.zeros((c["H"] * c["W"], half // 2)))      # sin 0
    assert np.array_equal(ref["pos"][-1][:, 1:half:2], np.ones((c["H"] * c["W"], half // 2)))       # cos 0


@pytest.mark.parametrize("mutant", nb.MUTANTS)
def test_wrong_kernel_is_rejected(mutant):
    cases = CASES
    if mutant == "index_scale_double":
        found = _double_index_case()
        assert found is not None, "no size at which the two scales differ"
        H, Hi = found
        r = np.random.default_rng([SEED, H, Hi])
        c = nc.make_case("relu", "none", 1, 64, H, 1, 128, SEED)
        c["image_mask"] = (np.arange(Hi) % 2).astype(np.uint8).reshape(1, Hi, 1) * np.uint8(r.integers(1, 256))      # alternate rows padded
        c["Hi"], c["Wi"] = Hi, 1
        cases = [c]
    rejected = 0
    for c in cases:
        for nsplit in (1, 2):
            if c["Cin"] % (64 * nsplit):
                continue
            fails, _ = nb.check(c, nb.model(c, nsplit, mutant), nsplit)
            rejected += bool(fails)
    assert rejected, f"{mutant}: no case rejects it"
    print(f"DETR_NECK_MUTANT {mutant}: rejected by {rejected} case runs")
