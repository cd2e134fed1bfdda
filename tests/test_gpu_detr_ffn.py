"""The DETR decoder's FFN with its tail through hg_test_detr_ffn (hoigen_amd/csrc/hg_detr_ffn.hip: the split over d_ff; the two GEMMs under
option detr_ffn = 1; detr_dec_tail_kernel) against the float64 reference and the per-element bound of tests/detr_ffn_bound.py: every
shape and family inside the bound on both paths, the exact families bit for bit the CPU restatement, NaN canaries around every output
intact, and a slice's partial sums a function of that slice alone."""
import numpy as np
import pytest
import torch

import detr_ffn_bound as fb
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

MS = (1, 31, 33, 100, 257)
HG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def run(ctx, c, option, want_partials=True):
    """-> (y [M, D], partials [n_sl, M, D] or None) numpy; the canary rows around both are checked"""
    lib = _lib.lib()
    assert lib.hg_set_option(ctx, b"detr_ffn", option) == 0
    M, D, F = c["M"], c["D"], c["F"]
    n_sl = F // fb.SLICE
    dev = {k: torch.from_numpy(c[k]).cuda() for k in ("x", "w1", "b1", "w2", "b2", "g3", "be3")}
    y = torch.full((M + 16, D), float("nan"), device="cuda")
    parts = torch.full((n_sl * M + 16, D), float("nan"), device="cuda") if want_partials and option != 1 else None
    rc = lib.hg_test_detr_ffn(ctx, dev["x"].data_ptr(), dev["w1"].data_ptr(), dev["b1"].data_ptr(), dev["w2"].data_ptr(), dev["b2"].data_ptr(),
                              dev["g3"].data_ptr(), dev["be3"].data_ptr(), M, D, F, y[8:].data_ptr(),
                              parts[8:].data_ptr() if parts is not None else None, None)
    assert rc == 0, lib.hg_last_error(ctx)
    torch.cuda.synchronize()
    y = y.cpu()
    assert torch.isnan(y[:8]).all() and torch.isnan(y[8 + M:]).all(), "rows around y were written"
    assert torch.isfinite(y[8:8 + M]).all()
    if parts is not None:
        parts = parts.cpu()
        assert torch.isnan(parts[:8]).all() and torch.isnan(parts[8 + n_sl * M:]).all(), "rows around the partial sums were written"
        parts = parts[8:8 + n_sl * M].reshape(n_sl, M, D).numpy()
    return y[8:8 + M].numpy(), parts


@pytest.mark.parametrize("D,F", [(D, F) for D in (128, 256) for F in (128, 256, 2048)])
def test_every_shape_and_family_inside_the_bound_on_both_paths(ctx, D, F):
    fails, top = [], {1: 0.0, 2: 0.0}
    for M in MS:
        for family in fb.FAMILIES:
            c = fb.make_case(family, M, D, F, seed=11)
            s, y, _ = fb.reference(c)
            exact = fb.model(c) if family in fb.EXACT_FAMILIES else None
            for option in (2, 1):
                Es, Ey, _ = fb.bounds(c, split=option == 2)
                got, parts = run(ctx, c, option)
                r = fb.worst_ratio(got, y, Ey)
                top[option] = max(top[option], r)
                if not r <= 1.0:
                    fails.append(f"{family} M {M} option {option}: stream worst |err| / bound {r:.3f}")
                if parts is not None:      # the kernel before the reduce: the pre-norm sum from its partial sums, in float64
                    pre = c["x"].astype(np.float64) + c["b2"] + parts.astype(np.float64).sum(0)
                    rs = fb.worst_ratio(pre, s, Es)
                    if not rs <= 1.0:
                        fails.append(f"{family} M {M}: pre-norm sum worst |err| / bound {rs:.3f}")
                if exact is not None:
                    if parts is not None and not np.array_equal(parts.view(np.int32), exact[0].view(np.int32)):
                        fails.append(f"{family} M {M}: the partial sums are not the exact ones bit for bit")
                    if not np.array_equal(got.view(np.int32), exact[2].view(np.int32)):
                        fails.append(f"{family} M {M} option {option}: the stream is not the restatement's bit for bit "
                                     f"({int((got.view(np.int32) != exact[2].view(np.int32)).sum())} elements)")
    print(f"DETR_FFN_RATIO D {D} d_ff {F}: worst |err| / bound, split kernel {top[2]:.3f}, two GEMMs {top[1]:.3f}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("D,F", [(128, 256), (256, 2048)])
def test_a_slice_of_partial_sums_depends_on_that_slice_only(ctx, D, F):
    for M in (33, 100):
        c = fb.make_case("randn", M, D, F, seed=12)
        _, parts = run(ctx, c, 2)
        for sl in (0, F // fb.SLICE - 1):
            u = slice(sl * fb.SLICE, (sl + 1) * fb.SLICE)
            one = dict(c, w1=np.ascontiguousarray(c["w1"][u]), b1=np.ascontiguousarray(c["b1"][u]), w2=np.ascontiguousarray(c["w2"][:, u]), F=fb.SLICE)
            _, p1 = run(ctx, one, 2)
            assert np.array_equal(p1[0].view(np.int32), parts[sl].view(np.int32)), (M, sl)


def test_the_default_rule_and_the_refusals(ctx):
    lib = _lib.lib()
    c = fb.make_case("randn", 100, 256, 256, seed=13)
    y2, _ = run(ctx, c, 2, want_partials=False)
    y0, p0 = run(ctx, c, 0)      # 100 rows: the rule picks the split kernel (partials exist), with the bits of option 2
    assert p0 is not None and np.array_equal(y0.view(np.int32), y2.view(np.int32))
    x = torch.zeros(8, 384, device="cuda")
    y = torch.full((8, 384), float("nan"), device="cuda")
    w = torch.zeros(384 * 128, device="cuda")
    assert lib.hg_set_option(ctx, b"detr_ffn", 2) == 0
    args = [x.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr()]
    assert lib.hg_test_detr_ffn(ctx, *args, 8, 384, 128, y.data_ptr(), None, None) == HG_ERR_INVALID      # d_model 384: no split kernel
    assert lib.hg_set_option(ctx, b"detr_ffn", 1) == 0
    assert lib.hg_test_detr_ffn(ctx, *args, 8, 384, 128, y.data_ptr(), y.data_ptr(), None) == HG_ERR_INVALID      # partials on the GEMM path
    for bad in ((0, 256, 128), (8, 200, 128), (8, 256, 100)):
        assert lib.hg_test_detr_ffn(ctx, *args, *bad, y.data_ptr(), None, None) == HG_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    assert lib.hg_set_option(ctx, b"detr_ffn", 3) == HG_ERR_INVALID
    assert lib.hg_set_option(ctx, b"detr_ffn", 0) == 0
