"""CPU side of the crop pre-processing rule (tests/preproc_cases.py): the oracle against Pillow itself at the sizes the goldens lack, the
restatement of the three kernels against the oracle on every committed case, the preconditions that make the cases worth running, and
the mutants - each must change at least one output byte of the committed cases.

File total on the build machine: about 12 s; the slowest single test takes under 2 s."""
import numpy as np
import pytest

import preproc_cases as pc
from oracle import preprocess_oracle as po

# mutant -> the committed cases asked to show it
SHOWN_BY = {"tables_256": ["step257", "step336_stretch", "plain336"], "crop_half_up": ["geo31"], "pad_ceil": ["pad31"], "ksv_stride": ["mixed31_stretch"],
            "no_rebase": ["geo31"], "bg_swapped": ["pad31"], "outside_bg": ["pad31"], "clip_wraps": ["geo31_step"],
            "weights_trunc": ["geo31"], "identity_axis": ["mixed31_stretch", "mixed97_stretch"]}


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_restatement_is_the_oracle(name):
    want_u8, want_f = pc.expected(name)
    got_u8, got_f = pc.restate(name)
    assert np.array_equal(got_u8, want_u8)
    assert np.array_equal(got_f.view(np.int32), want_f.view(np.int32)), "the 3 x 256 table is not the oracle's fp32 expression bit for bit"


def test_every_mutant_is_listed():
    assert sorted(SHOWN_BY) == sorted(pc.MUTANTS)


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_mutant_changes_bytes(mutant):
    changed = {n: int((pc.restate(n, mutant)[0] != pc.expected(n)[0]).sum()) for n in SHOWN_BY[mutant]}
    print(f"\nPREPROC_MUTANT {mutant}: bytes changed {changed}")
    assert all(v > 0 for v in changed.values()), changed


def test_sizes_and_options_are_covered():
    cases = pc.CASES
    assert {c["n_px"] for c in cases} == set(pc.SIZES)
    assert sum(c["n_px"] == 518 for c in cases) == 1
    for c in cases:
        assert c["n_px"] < 336 or len(c["boxes"]) <= 4, c["name"]
    assert {len(c["boxes"]) for c in cases} >= {1, 33}
    for key in ("pad_square", "stretch", "imagenet_norm", "return_u8"):
        assert {c[key] for c in cases} == {False, True}, key
    assert any(c["pad_square"] and len(set(c["background"])) == 3 for c in cases)
    # both trips of the tables loop (and a third at 518) have indices to fill
    assert {(c["n_px"] + 255) // 256 for c in cases} == {1, 2, 3}
    for name in ("step257", "plain336", "step336_stretch", "plain518"):
        n = pc.BY_NAME[name]["n_px"]
        for h in pc.geometry(name):
            arr = pc.fill_tables(h, n)
            for base, ks in ((0, h["ks_h"]), (2 * n + n * h["ks_h"], h["ks_v"])):
                counts = arr[base + 1:base + 2 * n:2]
                kk = arr[base + 2 * n:base + 2 * n + n * ks].reshape(n, ks)
                assert (counts[256:] > 0).all() and (kk[256:] != 0).any(1).all(), (name, "indices 256 .. are not populated")


def test_centre_crop_parities():
    """(resized - n_px) odd with an even and with an odd integer half: round-half-to-even differs from half-up on the first only"""
    halves = set()
    for name in ("geo31", "geo97"):
        for h in pc.geometry(name):
            for d in (h["nw"] - pc.BY_NAME[name]["n_px"], h["nh"] - pc.BY_NAME[name]["n_px"]):
                if d % 2:
                    halves.add((name, (d // 2) % 2))
    assert halves == {("geo31", 0), ("geo31", 1), ("geo97", 0), ("geo97", 1)}, halves


def test_identity_pass_on_each_axis():
    """cw == n_px with ch != n_px and the reverse: the table of the equal axis is the identity (one weight of 1 << 22 on the pixel
    itself) and the oracle skips that pass altogether - the bytes agree (test_restatement_is_the_oracle)"""
    for name, n in (("mixed31_stretch", 31), ("mixed97_stretch", 97)):
        seen = set()
        for h in pc.geometry(name):
            for axis, (src, dst, other_src, other_dst) in enumerate(((h["sw"], h["nw"], h["sh"], h["nh"]), (h["sh"], h["nh"], h["sw"], h["nw"]))):
                if src == dst == n and other_src != other_dst:
                    arr = pc.fill_tables(h, n)
                    ks = h["ks_v"] if axis else h["ks_h"]
                    base = 2 * n + n * h["ks_h"] if axis else 0
                    first = h["top"] if axis else h["left"]
                    assert first == 0
                    kk = arr[base + 2 * n:base + 2 * n + n * ks].reshape(n, ks)
                    b = arr[base:base + 2 * n].reshape(n, 2)
                    centre = np.arange(n) - b[:, 0]
                    assert (kk[np.arange(n), centre] == 1 << pc.PREC).all() and (kk != 0).sum() == n
                    seen.add(axis)
        assert seen == {0, 1}, (name, seen)


def test_clip8_saturates_at_both_ends_in_both_passes():
    """counted in the restatement, which test_restatement_is_the_oracle proves equal to the oracle on the same case"""
    for name in ("geo31_step", "mixed97_stretch", "step257", "step336_stretch"):
        stats = {}
        pc.restate(name, stats=stats)
        print(f"\nPREPROC_SATURATION {name}: {stats}")
        assert all(stats[k] > 0 for k in ("h_below", "h_above", "v_below", "v_above")), (name, stats)


def test_table_strides_differ_inside_one_call():
    """ks_h != ks_v in a box, and strongly different from its neighbours': an offset worked out with the wrong ks lands in another
    array"""
    for name in ("mixed31_stretch", "geo31"):
        g = pc.geometry(name)
        ks = [(h["ks_h"], h["ks_v"]) for h in g]
        assert any(a != b for a, b in ks)
        assert any(abs(ks[i][0] - ks[i + 1][0]) >= 40 for i in range(len(ks) - 1)), ks
    ks = [(h["ks_h"], h["ks_v"]) for h in pc.geometry("mixed31_stretch")]
    assert any(a - b >= 40 for a, b in ks) and any(b - a >= 40 for a, b in ks), ks


def test_scratch_offsets_need_their_rounding():
    for name in ("geo31", "n33_at_31", "geo257"):
        assert any(b % 16 for b in pc.scratch_bytes(name)[:-1]), name


PIL_BOXES = [(3, 4, 4, 40), (0, 5, 40, 7), (-30, -20, 487, 331), (7, 9, 10, 12), (100, 100, 325, 324), (50, 60, 200, 290), (-10, 50, 30, 90)]


@pytest.mark.parametrize("n_px", [336, 257, 31])
@pytest.mark.parametrize("stretch", [False, True])
def test_oracle_is_pillow_at_the_new_sizes(n_px, stretch):
    """1-pixel-wide, 2-row, leaving the image on all sides, an upscale, and three ordinary boxes of the noise image"""
    Image = pytest.importorskip("PIL.Image")
    img = pc.image("noise")
    pil = Image.fromarray(img)
    want = []
    for b in PIL_BOXES:
        c = pil.crop(b)
        if stretch:
            c = c.resize((n_px, n_px), Image.BICUBIC)
        else:
            nw, nh = po.resized_size(c.size[0], c.size[1], n_px)
            c = c.resize((nw, nh), Image.BICUBIC)
            left, top = int(round((nw - n_px) / 2.0)), int(round((nh - n_px) / 2.0))
            c = c.crop((left, top, left + n_px, top + n_px))
        want.append(np.asarray(c))
    got, _ = po.preprocess_boxes(img, PIL_BOXES, n_px, stretch=stretch)
    assert np.array_equal(got, np.stack(want))
