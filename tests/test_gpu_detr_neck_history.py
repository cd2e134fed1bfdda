"""History independence of hg_detr_neck (hoigen_amd/csrc/hg_detr_neck.hip): the same call twice, and once more after a call of another
shape and split that grows and dirties the workspace, gives the same bits - for no split, the default rule and a split."""
import numpy as np
import pytest

import detr_neck_cases as nc
from hoigen_amd import _lib
from test_gpu_detr_neck import load, run, same_bits, set_split

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("split", (1, 0, 8))
def test_the_same_call_gives_the_same_bits_whatever_ran_before(split):
    lib = _lib.lib()
    ctx = lib.hg_create(0)
    assert ctx
    try:
        c = nc.make_case("outlier", "random", 2, 512, 7, 9, 256, 33)
        other = nc.make_case("cancel", "rect", 3, 512, 5, 13, 256, 34)
        load(ctx, c)
        set_split(ctx, split)
        first, second = run(ctx, c), run(ctx, c)
        load(ctx, other)
        set_split(ctx, 4)
        run(ctx, other)      # another shape and split: the partial sums of a larger call lie in the workspace now
        load(ctx, c)
        set_split(ctx, split)
        third = run(ctx, c)
        for got in (second, third):
            assert same_bits(got["src"], first["src"]) and same_bits(got["pos"], first["pos"]) and np.array_equal(got["mask"], first["mask"])
    finally:
        lib.hg_destroy(ctx)
