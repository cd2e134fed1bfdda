"""tests/detector_views_model.py - hg_detector_views' tiling restated on the CPU - equals the oracle on every committed case, grouped
into the calls the GPU test runs, and equals Pillow's fixture; and the wrong kernels of its MUTANTS are each rejected by a committed
case: what tests/test_gpu_detector_views.py can tell apart."""
import os

import numpy as np
import pytest

import detector_views_cases as dc
import detector_views_model as dvm


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def run(setting, names, mutant=None, hmax=0, wmax=0):
    return dvm.restate_call([dc.image(setting, n) for n in names], *dc.SETTINGS[setting], hmax=hmax, wmax=wmax, mutant=mutant)


def differs(setting, names, mutant):
    """does the mutant change any output of this call against the oracle?"""
    try:
        sizes, u8, tensors, mask, clip = run(setting, names, mutant)
    except AssertionError:
        return True
    items = [dc.expected(setting, n) for n in names]
    if sizes != [e["size"] for e in items]:
        return True
    t, m = dc.batch_expected(items)
    return not (all(np.array_equal(u, e["u8"]) for u, e in zip(u8, items)) and np.array_equal(bits(tensors), bits(t)) and np.array_equal(mask, m)
                and all(np.array_equal(bits(c), bits(e["clip"])) for c, e in zip(clip, items)))


@pytest.mark.parametrize("setting", sorted(dc.SETTINGS))
def test_model_equals_the_oracle_on_every_call(setting):
    for names in dc.CALLS:
        sizes, u8, tensors, mask, clip = run(setting, names)
        items = [dc.expected(setting, n) for n in names]
        assert sizes == [e["size"] for e in items], names
        t, m = dc.batch_expected(items)
        for n, u, e, c in zip(names, u8, items, clip):
            assert np.array_equal(u, e["u8"]), (setting, n)
            assert np.array_equal(bits(c), bits(e["clip"])), (setting, n)
        assert np.array_equal(bits(tensors), bits(t)) and np.array_equal(mask, m), (setting, names)


def test_model_equals_pillow(golden_dir):
    g = np.load(os.path.join(golden_dir, "g17_detector_views.npz"))
    sizes, u8, _, _, clip = run("a", dc.NAMES)
    for n, s, u, c in zip(dc.NAMES, sizes, u8, clip):
        assert s == tuple(g[f"{n}_size"]) and np.array_equal(u, g[f"{n}_u8"]), n
        assert np.array_equal(bits(c), bits(dc.imagenet_planes(g[f"{n}_clip_u8"]))), n


def test_a_slice_of_a_larger_batch_pads_to_the_callers_extent():
    names = ("landscape", "thin")
    sizes, u8, tensors, mask, clip = run("a", names, hmax=70, wmax=300)      # more than one group of strips, several padding bands
    t, m = dc.batch_expected([dc.expected("a", n) for n in names], 70, 300)
    assert np.array_equal(bits(tensors), bits(t)) and np.array_equal(mask, m)


# the case that convicts each mutant, and why
CONVICTS = {
    "half_up": ("a", ("thin",)),                    # 66 * 5 / 132 = 2.5
    "v_first": ("a", ("landscape",)),
    "no_round": ("a", ("landscape",)),
    "clip_raw": ("a", ("landscape",)),
    "clip_consts": ("a", ("black",)),
    "mask_inverted": ("a", ("square",)),
    "stale_padding": ("a", ("portrait", "square", "identity")),
    "seam_tap": ("a", ("down12",)),                 # bands of two output rows, 20 seams
    "strip_short": ("a", ("w65",)),                 # a second strip of one column
}


@pytest.mark.parametrize("mutant", dvm.MUTANTS)
def test_wrong_kernels_are_rejected_by_the_committed_cases(mutant):
    setting, names = CONVICTS[mutant]
    assert any(set(names) <= set(call) for call in dc.CALLS) or len(names) == 1
    assert differs(setting, names, mutant), mutant
    assert not differs(setting, names, None)


def test_every_mutant_has_a_case():
    assert set(CONVICTS) == set(dvm.MUTANTS)
