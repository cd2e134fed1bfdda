"""hg_detector_views (hg_detector_views.hip) on the GPU, bit for bit: every case of tests/detector_views_cases.py at both settings, grouped
into calls of 1, 3 and 7 images in two orders, against the oracle (oracle/preprocess_oracle.py) and, at setting `a`, against Pillow's own
output (tests/golden/g17_detector_views.npz); the CLIP view against CropPreprocessor.batch on the resized images; an image's outputs
independent of batch, order and call split; padding 0 / mask 1; sentinels in front of and behind every output untouched; one
full-scale call at (800, 1333, 224); a small call after a large one on the stale workspace; refusals that launch nothing; the façade
against the raw call, 70 images included.

    uint8   array_equal          fp32   array_equal as int32 bit patterns

tests/test_detector_views_model.py proves on the CPU which wrong kernels these cases reject."""
import ctypes
import os

import numpy as np
import pytest
import torch

import detector_views_cases as dc
from hoigen_amd import _lib, detector_views, preprocess

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 1024                     # sentinel elements in front of and behind every output
F_SENT, B_SENT = 7.25, 0x5C


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def raw_call(images, size, max_size, clip_px, hmax=0, wmax=0, own_u8=True, expect_rc=0, null_image=None, B=None):
    """hg_detector_views through ctypes, every output between sentinels (asserted untouched).  images: uint8 numpy [H, W, 3].
    -> (sizes, u8 list or None, tensors [B, 3, hm, wm], mask [B, hm, wm], clip [B, 3, n, n] or None) as numpy; with expect_rc != 0 the
    call must return it and leave every buffer, sized for `images` without the refused ones, as it was."""
    dev = [torch.from_numpy(np.array(im)).to(DEV) for im in images]
    nb = len(dev)
    hs, ws = [im.shape[0] for im in images], [im.shape[1] for im in images]
    if expect_rc:
        sizes, hm, wm, total = [(8, 8)] * nb, max(hmax, 8), max(wmax, 8), 256 * nb
    else:
        sizes, hm, wm, off = detector_views.view_shapes(hs, ws, size, max_size)
        hm, wm, total = (hmax or hm), (wmax or wm), int(off[nb])
    n = clip_px if 0 < clip_px <= 518 else 8
    t = torch.full((2 * GUARD + nb * 3 * hm * wm,), F_SENT, dtype=torch.float32, device=DEV)
    m = torch.full((2 * GUARD + nb * hm * wm,), B_SENT, dtype=torch.uint8, device=DEV)
    c = torch.full((2 * GUARD + nb * 3 * n * n,), F_SENT, dtype=torch.float32, device=DEV)
    u = torch.full((2 * GUARD + total,), B_SENT, dtype=torch.uint8, device=DEV)
    ptrs = [im.data_ptr() for im in dev]
    if null_image is not None:
        ptrs[null_image] = None
    a = _lib.hg_detector_views_args(
        (ctypes.c_void_p * nb)(*ptrs), (ctypes.c_int32 * nb)(*hs), (ctypes.c_int32 * nb)(*ws), nb if B is None else B, size, max_size, clip_px,
        hmax, wmax, u[GUARD:].data_ptr() if own_u8 else None, t[GUARD:].data_ptr(), m[GUARD:].data_ptr(), c[GUARD:].data_ptr() if clip_px else None)
    rc = _lib.lib().hg_detector_views(_lib.ctx(0), ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t, m, c, u = t.cpu().numpy(), m.cpu().numpy(), c.cpu().numpy(), u.cpu().numpy()
    if expect_rc:
        assert rc == expect_rc, (rc, _lib.lib().hg_last_error(_lib.ctx(0)))
        assert (t == F_SENT).all() and (m == B_SENT).all() and (c == F_SENT).all() and (u == B_SENT).all(), "a refused call wrote something"
        return _lib.lib().hg_last_error(_lib.ctx(0)).decode()
    _lib.check(0, rc, "hg_detector_views")
    for buf, sent, what in ((t, F_SENT, "detr"), (m, B_SENT, "mask"), (c, F_SENT, "clip"), (u, B_SENT, "resized_u8")):
        assert (buf[:GUARD] == sent).all() and (buf[-GUARD:] == sent).all(), f"a sentinel of {what} was written"
    if not clip_px:
        assert (c == F_SENT).all()
    if not own_u8:
        assert (u == B_SENT).all()
    u8 = [u[GUARD + int(off[b]):GUARD + int(off[b]) + oh * ow * 3].reshape(oh, ow, 3) for b, (oh, ow) in enumerate(sizes)] if own_u8 else None
    return (sizes, u8, t[GUARD:-GUARD].reshape(nb, 3, hm, wm), m[GUARD:-GUARD].reshape(nb, hm, wm),
            c[GUARD:-GUARD].reshape(nb, 3, n, n) if clip_px else None)


def check_against(items, got, hmax=None, wmax=None, what=""):
    sizes, u8, tensors, mask, clip = got
    assert sizes == [e["size"] for e in items], what
    want_t, want_m = dc.batch_expected(items, hmax, wmax)
    for i, e in enumerate(items):
        if u8 is not None:
            assert np.array_equal(u8[i], e["u8"]), (what, i, "resized bytes")
        if clip is not None:
            assert np.array_equal(bits(clip[i]), bits(e["clip"])), (what, i, "clip view")
    assert np.array_equal(bits(tensors), bits(want_t)), (what, "detr planes / zero padding")
    assert np.array_equal(mask, want_m), (what, "mask")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g17_detector_views.npz"))


SEEN = {}      # (setting, name) -> [(u8, planes inside (oh, ow), clip)] of every call the image was in


@pytest.mark.parametrize("names", dc.CALLS, ids=["+".join(n) for n in dc.CALLS])
@pytest.mark.parametrize("setting", sorted(dc.SETTINGS))
def test_bit_for_bit_against_the_oracle_and_pillow(setting, names, golden):
    got = raw_call([dc.image(setting, n) for n in names], *dc.SETTINGS[setting])
    items = [dc.expected(setting, n) for n in names]
    check_against(items, got, what=(setting, names))
    sizes, u8, tensors, mask, clip = got
    for i, n in enumerate(names):
        oh, ow = sizes[i]
        SEEN.setdefault((setting, n), []).append((u8[i], tensors[i, :, :oh, :ow].copy(), clip[i]))
        if setting == "a":
            assert sizes[i] == tuple(golden[f"{n}_size"]) and np.array_equal(u8[i], golden[f"{n}_u8"]), n
            assert np.array_equal(bits(clip[i]), bits(dc.imagenet_planes(golden[f"{n}_clip_u8"]))), n
    # the CLIP view is CropPreprocessor's of the resized images
    n_px = dc.SETTINGS[setting][2]
    ref = preprocess.CropPreprocessor(n_px, stretch=True, imagenet_norm=True).batch([torch.from_numpy(u.copy()).to(DEV) for u in u8])
    assert np.array_equal(bits(ref.cpu().numpy()), bits(clip)), (setting, names)


def test_an_images_outputs_do_not_depend_on_batch_order_or_split():
    """the two orders put every image into calls of other sizes, at other positions, beside other images and under other paddings"""
    if len(SEEN) < len(dc.NAMES) * len(dc.SETTINGS):      # (run alone: make the calls)
        for setting in sorted(dc.SETTINGS):
            for names in dc.CALLS:
                sizes, u8, tensors, mask, clip = raw_call([dc.image(setting, n) for n in names], *dc.SETTINGS[setting])
                for i, n in enumerate(names):
                    SEEN.setdefault((setting, n), []).append((u8[i], tensors[i, :, :sizes[i][0], :sizes[i][1]].copy(), clip[i]))
    for key, runs in SEEN.items():
        assert len(runs) >= 2, key
        for r in runs[1:]:
            assert np.array_equal(r[0], runs[0][0]) and np.array_equal(bits(r[1]), bits(runs[0][1])) and np.array_equal(bits(r[2]), bits(runs[0][2])), key
    # one image alone, the same image twice in one call, and without a CLIP view or a buffer for the resized bytes
    im, e = dc.image("b", "landscape"), dc.expected("b", "landscape")
    check_against([e, e], raw_call([im, im], *dc.SETTINGS["b"]), what="twice")
    size, max_size, _ = dc.SETTINGS["b"]
    check_against([e], raw_call([im], size, max_size, 0, own_u8=False), what="no clip, no u8")


def test_a_slice_of_a_larger_batch_pads_to_the_callers_extent():
    names = ("landscape", "thin")
    got = raw_call([dc.image("a", n) for n in names], *dc.SETTINGS["a"], hmax=70, wmax=300)      # two groups of strips, padding bands
    check_against([dc.expected("a", n) for n in names], got, 70, 300, what="slice")


def test_full_scale_call_then_a_small_one_on_the_stale_workspace():
    """480 x 640 and 640 x 427 at (800, 1333, 224): hmax 1199, wmax 1066; then a call of small images whose tables, boxes and resized
    bytes land in the workspace the large call left full"""
    imgs = [dc.full_image(0), dc.full_image(1)]
    items = [dc.expected_full(0), dc.expected_full(1)]
    got = raw_call(imgs, *dc.FULL)
    assert got[2].shape == (2, 3, 1199, 1066) and got[0] == [(800, 1066), (1199, 800)]
    check_against(items, got, what="full scale")
    ref = preprocess.CropPreprocessor(224, stretch=True, imagenet_norm=True).batch([torch.from_numpy(u.copy()).to(DEV) for u in got[1]])
    assert np.array_equal(bits(ref.cpu().numpy()), bits(got[4]))
    check_against(items, raw_call(imgs, *dc.FULL, own_u8=False), what="full scale, resized bytes in the workspace")
    names = dc.CALLS[2]
    small = raw_call([dc.image("a", n) for n in names], *dc.SETTINGS["a"], own_u8=False)
    check_against([dc.expected("a", n) for n in names], small, what="small after large")


def test_refusals_return_invalid_and_launch_nothing():
    ok, size, max_size, n = dc.image("a", "landscape"), *dc.SETTINGS["a"]
    inv = -1
    assert "image 1 (1 x 200, h x w): an output side of 0" in raw_call([ok, np.zeros((1, 200, 3), np.uint8), ok], size, max_size, n, expect_rc=inv)
    assert "image 2" in raw_call([ok, ok, np.zeros((700, 700, 3), np.uint8)], size, 0, n, expect_rc=inv)                  # 17.5 : 1, 71 taps
    assert "above 2048" in raw_call([np.zeros((4, 400, 3), np.uint8)], size, 0, n, expect_rc=inv)
    assert "image 0 is null" in raw_call([ok, ok], size, max_size, n, expect_rc=inv, null_image=0)
    assert "B must be" in raw_call([ok], size, max_size, n, expect_rc=inv, B=0)
    assert "B must be" in raw_call([ok], size, max_size, n, expect_rc=inv, B=65)
    assert "clip_px" in raw_call([ok], size, max_size, 519, expect_rc=inv)
    assert "size" in raw_call([ok], 0, max_size, n, expect_rc=inv)
    assert "hmax, wmax" in raw_call([ok], size, max_size, n, hmax=39, wmax=300, expect_rc=inv)
    assert "hmax, wmax" in raw_call([ok], size, max_size, n, hmax=40, wmax=2049, expect_rc=inv)
    # (50, 50) -> (200, 200) is within 16 x 13 = 208; (30, 47) -> (191, 299) is not
    assert "image 1: its resized image (191 x 299)" in raw_call([np.zeros((50, 50, 3), np.uint8), ok], 200, 300, 13, expect_rc=inv)
    # and the context is as good as before
    check_against([dc.expected("a", "landscape")], raw_call([ok], size, max_size, n), what="after the refusals")


def test_facade_equals_the_raw_call_and_splits_70_images():
    size, max_size, n = dc.SETTINGS["a"]
    dv = detector_views.DetectorViews(size, max_size, n)
    names = dc.CALLS[2]
    raw = raw_call([dc.image("a", x) for x in names], size, max_size, n)
    tensors, mask, clip, sizes, u8 = dv([torch.from_numpy(dc.image("a", x).copy()).to(DEV) for x in names], return_u8=True)
    assert mask.dtype == torch.bool and tensors.dtype == torch.float32 and sizes == raw[0]
    assert np.array_equal(bits(tensors.cpu().numpy()), bits(raw[2])) and np.array_equal(mask.cpu().numpy().view(np.uint8), raw[3])
    assert np.array_equal(bits(clip.cpu().numpy()), bits(raw[4])) and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(u8, raw[1]))
    # 70 images: two calls writing slices of the one output; the padded extent is that of all 70 (`max_h` is only among the last six)
    order = [x for x in dc.NAMES if x not in ("down12", "max_h")]
    many = [order[i % len(order)] for i in range(64)] + ["max_h", "thin", "max_h", "landscape", "white", "w65"]
    assert max(dc.expected("a", x)["size"][0] for x in many[:64]) < dc.expected("a", "max_h")["size"][0]
    res = dv([torch.from_numpy(dc.image("a", x).copy()).to(DEV) for x in many], return_u8=True)
    torch.cuda.synchronize()
    got = (res[3], [t.cpu().numpy() for t in res[4]], res[0].cpu().numpy(), res[1].cpu().numpy().view(np.uint8), res[2].cpu().numpy())
    assert got[2].shape[0] == 70
    check_against([dc.expected("a", x) for x in many], got, what="70 images")
    # no CLIP view
    t0, m0, c0, s0 = detector_views.DetectorViews(size, max_size, 0)([torch.from_numpy(dc.image("a", "portrait").copy()).to(DEV)])
    assert c0 is None and s0 == [(62, 40)] and np.array_equal(bits(t0.cpu().numpy()[0]), bits(dc.expected("a", "portrait")["planes"])) and not m0.any()
