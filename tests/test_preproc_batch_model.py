"""tests/preproc_batch_model.py - the CPU restatement of hg_preproc_batch.hip in its structure (device geometry, bands, row buffer,
window) - against tests/preproc_cases.py: every committed case byte for byte, in calls of several images; the module's own cases against
the oracle; and the proof that the cases reject each of its mutants.  No GPU, no library."""
import numpy as np
import pytest

import preproc_batch_model as pbm
import preproc_cases as pc


@pytest.fixture(scope="module")
def restated():
    """every call through the restatement, once: {call index: (u8, status, slices, seen)}"""
    out = {}
    for i, names in enumerate(pbm.CALLS):
        seen = {}
        out[i] = pbm.restate_named_call(names, seen=seen) + (seen,)
    return out


def test_every_committed_case_is_in_some_call_and_some_calls_have_two_images():
    named = [n for names in pbm.CALLS for n in names]
    assert sorted(named) == sorted([c["name"] for c in pc.CASES + pbm.OWN])
    assert {"geo31", "geo31_step", "one_box_31"} <= set(pbm.CALLS[0]) and ["pad31", "pad31_step"] in pbm.CALLS and ["geo257", "step257"] in pbm.CALLS
    assert sum(len(pbm.call_inputs(n)[0]) > 1 for n in pbm.CALLS) >= 3


@pytest.mark.parametrize("i", range(len(pbm.CALLS)), ids=["+".join(n) for n in pbm.CALLS])
def test_restatement_equals_the_oracle_byte_for_byte(restated, i):
    u8, status, slices, _ = restated[i]
    for name, sl in slices.items():
        want_u8, want_f, want_status = pbm.expected(name)
        assert np.array_equal(status[sl], want_status), name
        assert np.array_equal(u8[sl], want_u8), (name, int((u8[sl] != want_u8).sum()))
        got_f = pbm.planes(u8[sl], status[sl], pbm.case(name)["imagenet_norm"])
        assert np.array_equal(got_f.view(np.int32), want_f.view(np.int32)), name


def test_constants_and_sizes_are_those_of_the_kernels_header():
    """the restatement's limits, band height, window rows, status bits and its LDS / row-buffer / table sizes, read from
    hoigen_amd/csrc/hg_preproc_geom.h: a kernel and a restatement that drift apart fail here"""
    c = pbm.header_constants()
    assert (c["PREB_MAX_IMAGES"], c["PREB_MAX_N"], c["PREB_MAX_NPX"], c["PREB_MAX_TAPS"], c["PREB_MAX_COORD"]) == \
           (pbm.MAX_IMAGES, pbm.MAX_N, pbm.MAX_NPX, pbm.MAX_TAPS, pbm.MAX_COORD)
    assert (c["PREB_BAND"], c["PREB_WIN_ROWS"], c["PREB_HDR"]) == (pbm.BAND, pbm.WIN_ROWS, pbm.HDR)
    assert (c["PREB_HCACHE_NPX"], c["PREB_HCACHE_TAPS"]) == (pbm.HCACHE_NPX, pbm.HCACHE_TAPS)
    assert (c["PREB_EMPTY"], c["PREB_TAPS"], c["PREB_IMAGE"]) == (pbm.EMPTY, pbm.TAPS, pbm.IMAGE)
    f = pbm.header_functions()
    for n_px in range(1, pbm.MAX_NPX + 1):
        assert f["preb_max_cols"](n_px) == pbm.max_cols(n_px) and f["preb_win_stride"](n_px) == pbm.win_stride(n_px)
        assert f["preb_rowbuf_bytes"](n_px) == pbm.rowbuf_bytes(n_px) and f["preb_lds_bytes"](n_px) == pbm.lds_bytes(n_px)
        assert f["preb_axis_words"](n_px) == n_px * (2 + pbm.MAX_TAPS) and f["preb_hcache_words"](n_px) == pbm.hcache_words(n_px)
        assert pbm.lds_bytes(n_px) <= 160 * 1024
    assert pbm.WIN_ROWS >= pbm.MAX_TAPS + 1 and pbm.BAND * (pbm.MAX_TAPS + 2) * 4 % 16 == 0


def test_the_cases_reach_every_path_of_the_kernel(restated):
    seen = [s for *_, s in restated.values()]
    assert max(s["max_rows"] for s in seen) >= 65 and max(s["max_rows"] for s in seen) <= pbm.WIN_ROWS      # a full window
    assert min(s["min_bh"] for s in seen) == 1 and any(s["min_bh"] == pbm.BAND for s in seen)                 # shrunk and full bands
    assert max(s["trips"] for s in seen) >= 2                                                                  # the row buffer refilled
    assert pbm.lds_bytes(pbm.MAX_NPX) <= 160 * 1024


def test_an_unaligned_image_base_changes_nothing(restated):
    """the row buffer's `lead` follows the image's address: bases 5 and 15 modulo 16 give the bytes of base 0"""
    i = next(k for k, names in enumerate(pbm.CALLS) if "geo31" in names)
    for addr in (5, 15):
        assert np.array_equal(pbm.restate_named_call(pbm.CALLS[i], addr=addr)[0], restated[i][0])


def test_geometry_is_the_host_geometry_of_the_per_image_call():
    for c in pc.CASES + pbm.OWN:
        for b in c["boxes"]:
            h, status = pbm.geometry(b, 0, 1, c["n_px"], pbm.flags_of(c))
            if tuple(int(v) for v in b) == pbm.ABOVE_BOX:
                assert status == pbm.TAPS and not any(h[:13]) and not any(h[14:20])
                continue
            assert status == 0 and pbm.as_dict(h) == pc.header(b, c["n_px"], c["pad_square"], c["stretch"])
            assert 1 <= h[12] <= pbm.BAND and 0 <= h[19] <= pbm.max_cols(c["n_px"])


def test_limit_boxes_sit_at_the_limit():
    assert pbm.geometry(pbm.LIMIT_BOX, 0, 1, 31, 0)[0][8:10] == [65, 65]
    assert pc._taps(497, 31) == 67
    h = pbm.geometry(pbm.TALL_BOX, 0, 1, 31, 0)[0]
    assert h[15] == 33943 and pbm.geometry(pbm.TALL_BOX, 0, 1, 31, 0, mutant="target_fp32")[0][15] == 33944


def test_statuses():
    g = lambda box, im=0, B=2: pbm.geometry(box, im, B, 31, 0)[1]
    assert g((5, 5, 5, 9)) == pbm.EMPTY and g((5, 5, 9, 5)) == pbm.EMPTY and g((9, 5, 5, 9)) == pbm.EMPTY
    assert g((0, 0, 10, 10), 2) == pbm.IMAGE and g((0, 0, 10, 10), -1) == pbm.IMAGE and g((5, 5, 5, 9), 2) == pbm.EMPTY | pbm.IMAGE
    assert g(pbm.ABOVE_BOX) == pbm.TAPS and g(pbm.ABOVE_BOX, 7) == pbm.TAPS | pbm.IMAGE
    assert g((0, 0, (1 << 20) + 1, 10)) == pbm.TAPS and g((-(1 << 31), 0, (1 << 31) - 1, 10)) == pbm.TAPS
    u8, status = pbm.restate_call([pc.image("step")], [(0, 0, 9, 9), (5, 5, 5, 9), (0, 0, 9, 9)], [0, 0, 1], 31)
    assert status.tolist() == [0, pbm.EMPTY, pbm.IMAGE] and u8[0].any() and not u8[1:].any()
    assert np.isnan(pbm.planes(u8, status, False)[1:]).all() and not np.isnan(pbm.planes(u8, status, False)[0]).any()


# the case whose call rejects each mutant: at least one byte of it changes (the unmutated restatement is the oracle's: above)
REJECTED_BY = {"band_seam": "geo31", "no_rebase": "geo31", "crop_half_up": "geo31", "image_by_crop": "geo31", "target_fp32": "own31_limit",
               "taps_ge": "own31_limit", "refused_writes": "own31_limit"}


@pytest.mark.parametrize("mutant", pbm.MUTANTS)
def test_mutant_is_rejected(restated, mutant):
    i = next(k for k, names in enumerate(pbm.CALLS) if REJECTED_BY[mutant] in names)
    u8, status, _ = pbm.restate_named_call(pbm.CALLS[i], mutant=mutant)
    changed = int((u8 != restated[i][0]).sum())
    assert changed > 0, f"{mutant}: no byte of {pbm.CALLS[i]} changes"
    if mutant == "taps_ge":
        assert status.tolist() != restated[i][1].tolist()
