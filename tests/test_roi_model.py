"""CPU side of the two RoI-align rules (tests/roi_bound.py): the vectorised fp32 restatement is oracle/roi_oracle.py bit for bit; it stays
inside the float64 rule's bound E on every committed case (ratios printed as ROI_RATIO lines, the table is in roi_bound's docstring); the
float64 definition equals the closed form on affine maps; the `ints` family is exact; every mutant is rejected by at least one rule; and
the build leaves no fused multiply-add in the kernel beyond those of its divisions.

File total on the build machine: about 10 s; the slowest test is the float64 reference of the 24 x 24 x 1024 map (6 s)."""
import numpy as np
import pytest

import roi_bound as rb
from oracle import roi_oracle as ro

RULE2 = [c["name"] for c in rb.CASES if c["rule2"]]
# mutant -> the committed cases asked to reject it
SHOWN_BY = {"no_half_pixel": "c4_5x9_p7", "fixed_grid": "c4_5x9_p7", "count_no_max": "c4_5x9_p7", "cutoff_hm1": "c4_5x9_p7",
            "no_clamp": "c4_5x9_p7", "weights_swapped": "c4_5x9_p7", "channels_256": "one_box", "mean_pw_ph": "c4_5x9_p7",
            "pairwise_mean": "outlier_24x24", "fma_sum": "outlier_24x24"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("name", ["c4_5x9_p7", "cuts_14x14_p7", "affine_5x9_p2", "ints_p1"])
def test_restatement_is_the_oracle(name):
    c = rb.BY_NAME[name]
    want = ro.roi_align(rb.feat_of(c), c["boxes"], c["P"], c["scale"])
    assert np.array_equal(bits(rb.expected(name)[0]), bits(want))


def test_shapes_are_covered():
    cs = rb.CASES
    assert {(c["H"], c["W"]) for c in cs} == {(14, 14), (24, 24), (5, 9)}
    assert {c["C"] for c in cs} == {4, 255, 256, 257, 768, 1024}
    assert {c["P"] for c in cs} == {1, 2, 7, 14}
    assert {float(c["scale"]) for c in cs} == {float(np.float32(1 / 16)), float(np.float32(1 / 14))}
    assert {len(c["boxes"]) for c in cs} >= {1, 45}
    assert any(c["H"] == 24 and c["C"] == 1024 and c["P"] == 7 and float(c["scale"]) == float(np.float32(1 / 14)) for c in cs)


@pytest.mark.parametrize("name", RULE2)
def test_restatement_is_inside_the_float64_bound(name):
    c = rb.BY_NAME[name]
    ref = rb.reference(name)
    pooled, mean = rb.expected(name)
    r = rb.ratios(ref, pooled, mean)
    n_random = c["n_random"]
    print(f"\nROI_RATIO {name} restatement: pooled {r['pooled']:.3f} mean {r['mean']:.3f} ({int(ref['kept'].sum())} of {len(c['boxes'])} boxes kept)")
    assert r["pooled"] <= 1.0 and r["mean"] <= 1.0, r
    if n_random:
        lost = int((~ref["kept"][:n_random]).sum())
        assert lost <= 0.05 * n_random, f"{lost} of {n_random} random boxes are too close to a discontinuity"


def test_degenerate_boxes_give_zero():
    """zero width, x2 < x1 and boxes wholly outside the map: no sample contributes, count is max(.., 1): exactly 0"""
    pooled, mean = rb.expected("c4_5x9_p7")
    assert not pooled[40:44].any() and not mean[40:44].any()
    ref = rb.reference("c4_5x9_p7")
    assert not ref["pooled"][40:44].any()
    assert np.abs(pooled[44]).max() > 0          # the huge box is not


def test_huge_box_has_an_8x8_grid():
    c = rb.BY_NAME["vitl_24x24_1024"]
    _, _, bh, _, gh = rb._coord_error(c["boxes"][44, 1], c["boxes"][44, 3], c["scale"], c["P"], c["H"])
    assert gh == 8, (bh, gh)


def test_boxes_on_the_cuts_are_on_the_cuts():
    for name in ("cuts_14x14_p7", "cuts_24x24_p2"):
        c = rb.BY_NAME[name]
        H, P = c["H"], c["P"]
        got = []
        for b in c["boxes"]:
            y, _, bh, _, gh = rb._coord_error(b[1], b[3], c["scale"], P, H)
            got.append((float(y.min()), float(y.max()), bh, gh))
        assert got[0][0] == -1.0 and got[1][1] == float(H)
        assert [g[2:] for g in got[2:]] == [(1.0, 1), (2.0, 2), (3.0, 3)]
        assert not rb.reference(name)["kept"].any()          # rule 2 does not judge them; rule 1 does


def test_definition_is_the_closed_form_on_affine_maps():
    """a bin of an affine map is the map at the bin's centre when every sample lies inside [0, H - 1] x [0, W - 1]"""
    for name in ("affine_14x14", "affine_5x9_p2"):
        c = rb.BY_NAME[name]
        co = rb.affine_coeffs(c["C"], c["H"], c["W"])
        ref = rb.reference(name)
        P, s, seen = c["P"], float(c["scale"]), 0
        for i, b in enumerate(c["boxes"].astype(np.float64)):
            x1, y1, x2, y2 = b * s - 0.5
            if not (x1 >= 0 and y1 >= 0 and x2 <= c["W"] - 1 and y2 <= c["H"] - 1 and x2 > x1 and y2 > y1):
                continue
            cx = x1 + (np.arange(P) + 0.5) * (x2 - x1) / P
            cy = y1 + (np.arange(P) + 0.5) * (y2 - y1) / P
            want = co[:, 0, None, None] * cx[None, None, :] + co[:, 1, None, None] * cy[None, :, None] + co[:, 2, None, None]
            assert np.abs(ref["pooled"][i] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
            seen += 1
        assert seen >= 2, name


@pytest.mark.parametrize("name", ["ints_p1", "ints_p2"])
def test_ints_family_is_exact(name):
    """the precondition holds and the restatement is the float64 result rounded once, bit for bit (mean included)"""
    c = rb.BY_NAME[name]
    rb.exactness(rb.feat_of(c), c["boxes"], c["P"], c["scale"])
    ref = rb.reference(name)
    pooled, mean = rb.expected(name)
    assert (ref["pooled"].astype(np.float32).astype(np.float64) == ref["pooled"]).all()
    assert np.array_equal(pooled, ref["pooled"].astype(np.float32)) and np.array_equal(mean, ref["mean"].astype(np.float32))
    assert np.abs(pooled).max() > 0


def test_every_mutant_is_listed():
    assert sorted(SHOWN_BY) == sorted(rb.MUTANTS)


@pytest.mark.parametrize("mutant", rb.MUTANTS)
def test_mutant_is_rejected(mutant):
    """rule 1 (bits against the restatement) or rule 2 (float64 bound) must fail; pairwise_mean and fma_sum are correct arithmetic in
    another order: they must PASS rule 2 and fail rule 1 - which is why the bit rule exists"""
    name = SHOWN_BY[mutant]
    c = rb.BY_NAME[name]
    pooled, mean = rb.restate(rb.feat_of(c), c["boxes"], c["P"], c["scale"], mutant)
    want_p, want_m = rb.expected(name)
    rule1 = not (np.array_equal(bits(pooled), bits(want_p)) and np.array_equal(bits(mean), bits(want_m)))
    r = rb.ratios(rb.reference(name), pooled, mean)
    rule2 = not (r["pooled"] <= 1.0 and r["mean"] <= 1.0)
    print(f"\nROI_MUTANT {mutant} on {name}: rule 1 {'rejects' if rule1 else 'accepts'}, rule 2 {'rejects' if rule2 else 'accepts'} "
          f"(pooled {r['pooled']:.3g} mean {r['mean']:.3g})")
    assert rule1 or rule2
    if mutant in rb.BITS_ONLY:
        assert rule1 and not rule2
    elif mutant != "mean_pw_ph":
        assert rule2, "a wrong algorithm must not need the bit rule"


def test_the_build_does_not_fuse_the_kernels_operations():
    """hg_preproc.hip compiled with build.sh's own flags: in roi_align_kernel (and in the double-precision weight-table kernel) the only
    fused multiply-adds left are the five of each division's expansion.  Under the library's -ffp-contract=fast alone the backend fuses
    b * scale - 0.5 and sh + ph * bh whatever the source's `fp contract(off)` says, and the kernel is no longer the restatement bit for
    bit (tests/test_gpu_roi_exact.py is what found it).  Both the way the flags are read (the literal lines of build.sh) and the count of
    five fused operations per division are tied to the current build script and toolchain: a reformatted build.sh or a compiler that
    expands a division differently fails this test for a reason of its own, and the test is then to be re-read, not the kernel."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile

    from asm_blocks import kernel_body

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "hoigen_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    script = open(os.path.join(csrc, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    extra = re.search(r'\[ \$f = hg_preproc \] && X="([^"]*)"', script)
    assert extra and "$HIPCC $FLAGS $X -c" in script, "build.sh no longer gives hg_preproc.hip flags of its own"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "hg_preproc.s")
        r = subprocess.run([hipcc] + flags + extra.group(1).split() + ["-S", "--cuda-device-only", os.path.join(csrc, "hg_preproc.hip"), "-o", out],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        txt = open(out).read()
    for kernel, ty in (("roi_align_kernel", "f32"), ("preproc_tables_kernel", "f64")):
        name = re.search(r"^(_ZN2hg\d+%s\w*):" % kernel, txt, re.M).group(1)
        body = kernel_body(txt, name)
        fused = len(re.findall(r"\bv_(?:fma|fmac|pk_fma)_%s" % ty, body))
        divisions = len(re.findall(r"\bv_div_fixup_%s" % ty, body))
        print(f"\nROI_BUILD {kernel}: {fused} fused {ty} operations, {divisions} divisions")
        assert divisions > 0 and fused == 5 * divisions, (kernel, fused, divisions)
