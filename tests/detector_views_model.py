"""CPU restatement of hg_detector_views (hoigen_amd/csrc/hg_detector_views.hip, hg_detector_views_geom.h) in ITS structure, for
tests/test_detector_views_model.py.  A plain module: no fixtures, no GPU, no library.

    out_size(), band_rows()   dv_out_size, dv_band_rows: the size rule and a workgroup's band height from the vertical scale
    tables()                  dv_tables_kernel: bounds and 22-bit weights of both axes (oracle/preprocess_oracle.py::precompute_coeffs is
                              Pillow's precompute_coeffs / normalize_coeffs_8bpc, which hg_preproc_geom.h's preb_fill_index restates)
    restate_call()            dv_resample_kernel over its grid (group of STRIPS strips, band, image): per strip of STRIP columns the
                              horizontal pass of the source rows [rlo, rlo + nr) into a WINDOW of WIN_ROWS uint8 rows, the vertical pass
                              from the window with its slot guard, the table look-up, the mask, and the padding right of and below
                              the image; then the CLIP leg by tests/preproc_batch_model.py::restate_call on the resized images.
                              The window and every output start full of stale values, as LDS and a caller's buffers do.

Mutants (`MUTANTS`) that tests/test_detector_views_model.py proves change at least one committed case:

    half_up         the size rule's round() as floor(x + 0.5)
    v_first         vertical pass before the horizontal one
    no_round        no uint8 rounding between the passes (one shift and clamp at the end)
    clip_raw        the CLIP view taken from the raw image
    clip_consts     CLIP's constants in the detector view's table
    mask_inverted   mask 1 inside the image
    stale_padding   the padding not written
    seam_tap        a band's window one row short: its last row's last tap dropped at the seam
    strip_short     a strip whose horizontal pass stops one source column early: its last column's last tap dropped
"""
import math

import numpy as np

import detector_views_cases as dc
import preproc_batch_model as pbm
from oracle import preprocess_oracle as po

PREC = 22
MAX_IMAGES, MAX_SIDE, MAX_TAPS, BAND, STRIP, STRIPS, WIN_ROWS, VW_WORDS = 64, 2048, 65, 32, 64, 4, 72, 512
ZERO_SIDE, SIDE_ABOVE, TAPS, INPUT = 1, 2, 3, 4
MUTANTS = ("half_up", "v_first", "no_round", "clip_raw", "clip_consts", "mask_inverted", "stale_padding", "seam_tap", "strip_short")
STALE_U8, STALE_F32, STALE_MASK = 0xAA, np.float32(7.25), 0x5C


def taps(n_in, n_out):
    sc = n_in / n_out
    return int(math.ceil(2.0 * max(sc, 1.0))) * 2 + 1


def out_size(h, w, size, max_size, mutant=None):
    """dv_out_size -> (reason, oh, ow): reason 0, or why hg_detector_view_shapes refuses the image"""
    if h < 1 or w < 1:
        return INPUT, 0, 0
    if max_size > 0:
        mn, mx = float(min(w, h)), float(max(w, h))
        if mx / mn * float(size) > float(max_size):
            v = float(max_size) * mn / mx
            size = int(math.floor(v + 0.5)) if mutant == "half_up" else int(round(v))
    if (w <= h and w == size) or (h <= w and h == size):
        dh, dw = float(h), float(w)
    elif w < h:
        dw, dh = float(size), math.floor(float(size * h) / float(w))
    else:
        dh, dw = float(size), math.floor(float(size * w) / float(h))
    if dh < 1.0 or dw < 1.0:
        return ZERO_SIDE, 0, 0
    if dh > MAX_SIDE or dw > MAX_SIDE:
        return SIDE_ABOVE, 0, 0
    oh, ow = int(dh), int(dw)
    if taps(w, ow) > MAX_TAPS or taps(h, oh) > MAX_TAPS:
        return TAPS, oh, ow
    return 0, oh, ow


def view_shapes(heights, widths, size, max_size):
    """hg_detector_view_shapes -> (rc, sizes, hmax, wmax, u8_off): rc -1 with (hmax, wmax) = (image, reason) at the first refusal"""
    if len(heights) < 1 or not 1 <= size <= MAX_SIDE or not 0 <= max_size <= MAX_SIDE:
        return -1, [], -1, INPUT, []
    sizes, off = [], [0]
    for b, (h, w) in enumerate(zip(heights, widths)):
        why, oh, ow = out_size(h, w, size, max_size)
        if why:
            return -1, sizes, b, why, off
        sizes.append((oh, ow))
        off.append(off[-1] + (oh * ow * 3 + 255) // 256 * 256)
    return 0, sizes, max(s[0] for s in sizes), max(s[1] for s in sizes), off


def band_rows(in_h, out_h):
    sc = in_h / out_h
    fs = max(sc, 1.0)
    f = (float(WIN_ROWS) - 4.0 * fs - 2.0) / sc
    bh = BAND if f >= float(BAND - 1) else int(f) + 1
    bh = max(bh, 1)
    ks = taps(in_h, out_h)
    while bh > 1 and bh * ks > VW_WORDS:
        bh -= 1
    return bh


def n_bands(in_h, out_h, hmax):
    bh = band_rows(in_h, out_h)
    return (out_h + bh - 1) // bh + (hmax - out_h + BAND - 1) // BAND


def tables(H, W, oh, ow):
    hb, hk = po.precompute_coeffs(W, ow)
    vb, vk = po.precompute_coeffs(H, oh)
    assert hk.shape[1] == taps(W, ow) and vk.shape[1] == taps(H, oh)
    return hb, hk.astype(np.int64), vb, vk.astype(np.int64)


def lut(clip_consts=False):
    m, sd = (po.CLIP_MEAN, po.CLIP_STD) if clip_consts else (po.IMAGENET_MEAN, po.IMAGENET_STD)
    u = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return np.stack([(u - np.float32(m[c])) / np.float32(sd[c]) for c in range(3)])


def _clip8(acc):
    return np.clip(acc >> PREC, 0, 255)


def _image(img, oh, ow, hmax, wmax, u8, planes, mask, mutant):
    """dv_resample_kernel's workgroups of one image: writes u8 [oh, ow, 3], planes [3, hmax, wmax], mask [hmax, wmax] in place"""
    H, W = img.shape[:2]
    hb, hk, vb, vk = tables(H, W, oh, ow)
    ksv = vk.shape[1]
    table = lut(mutant == "clip_consts")
    bh = band_rows(H, oh)
    nb = (oh + bh - 1) // bh
    group = STRIP * STRIPS
    src = img.astype(np.int64)
    half = 1 << (PREC - 1)
    for band in range(n_bands(H, oh, hmax)):
        own = band < nb
        r0 = band * bh if own else oh + (band - nb) * BAND
        assert r0 < hmax
        r1 = min(r0 + bh, oh) if own else min(r0 + BAND, hmax)
        for g0 in range(0, wmax, group):
            g1 = min(g0 + group, wmax)
            ge = (min(g1, ow) if own else g0)
            if ge > g0:
                assert (r1 - r0) * ksv <= VW_WORDS
                rlo = int(vb[r0, 0])
                nr = int(vb[r1 - 1, 0] + vb[r1 - 1, 1]) - rlo
                assert 0 <= nr <= WIN_ROWS and rlo + nr <= H, (H, oh, r0, r1, nr)
                if mutant == "seam_tap":
                    nr -= 1
                for x0 in range(g0, ge, STRIP):
                    xe = min(x0 + STRIP, ge)
                    win = np.full((WIN_ROWS, STRIP, 3), STALE_U8, np.int64)
                    col_end = int(hb[xe - 1, 0] + hb[xe - 1, 1]) - (1 if mutant == "strip_short" else 0)
                    if mutant == "v_first":      # the whole wrong order, on the strip's columns: vertical on the raw rows, then horizontal
                        for yo in range(r0, r1):
                            first, cnt = int(vb[yo, 0]), int(vb[yo, 1])
                            rows = _clip8(half + np.tensordot(vk[yo, :cnt], src[first:first + cnt], 1))      # [W, 3]
                            for xo in range(x0, xe):
                                f, c = int(hb[xo, 0]), int(hb[xo, 1])
                                u = _clip8(half + np.tensordot(hk[xo, :c], rows[f:f + c], 1))
                                u8[yo, xo] = u
                                planes[:, yo, xo] = table[np.arange(3), u]
                                mask[yo, xo] = 0
                        continue
                    for q in range(nr):      # horizontal pass: source row rlo + q -> window row q
                        for xo in range(x0, xe):
                            f, c = int(hb[xo, 0]), int(hb[xo, 1])
                            c = min(c, col_end - f)
                            acc = half + np.tensordot(hk[xo, :c], src[rlo + q, f:f + c], 1)
                            win[q, xo - x0] = acc if mutant == "no_round" else _clip8(acc)
                    for yo in range(r0, r1):      # vertical pass from the window, slots beyond the band's rows dropped
                        first, cnt = int(vb[yo, 0]) - rlo, int(vb[yo, 1])
                        acc = np.full((xe - x0, 3), half, np.int64)
                        for j in range(cnt):
                            if 0 <= first + j < nr:
                                if mutant == "no_round":      # the window holds the unshifted sums: weights applied to unrounded rows
                                    acc += (win[first + j, :xe - x0] * vk[yo, j]) >> PREC
                                else:
                                    acc += win[first + j, :xe - x0] * vk[yo, j]
                        u = _clip8(acc)
                        u8[yo, x0:xe] = u
                        planes[:, yo, x0:xe] = table[np.arange(3)[:, None], u.T]
                        mask[yo, x0:xe] = 1 if mutant == "mask_inverted" else 0
            p0 = max(ge, g0)
            if mutant != "stale_padding":
                planes[:, r0:r1, p0:g1] = 0.0
                mask[r0:r1, p0:g1] = 0 if mutant == "mask_inverted" else 1


def restate_call(images, size, max_size, clip_px, hmax=0, wmax=0, mutant=None):
    """hg_detector_views -> (sizes, u8 list, tensors fp32 [B, 3, hmax, wmax], mask uint8 [B, hmax, wmax], clip fp32 [B, 3, n, n] or None)"""
    assert mutant is None or mutant in MUTANTS, mutant
    B = len(images)
    assert 1 <= B <= MAX_IMAGES
    sizes = []
    for im in images:
        why, oh, ow = out_size(im.shape[0], im.shape[1], size, max_size, mutant)
        assert why == 0, (im.shape, why)
        sizes.append((oh, ow))
    hm, wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if hmax or wmax:
        assert hmax >= hm and wmax >= wm
        hm, wm = hmax, wmax
    tensors = np.full((B, 3, hm, wm), STALE_F32, np.float32)
    mask = np.full((B, hm, wm), STALE_MASK, np.uint8)
    u8 = [np.full((oh, ow, 3), STALE_U8, np.uint8) for oh, ow in sizes]
    for b, im in enumerate(images):
        _image(im, sizes[b][0], sizes[b][1], hm, wm, u8[b], tensors[b], mask[b], mutant)
    clip = None
    if clip_px:
        src = images if mutant == "clip_raw" else u8
        boxes = [(0, 0, s.shape[1], s.shape[0]) for s in src]
        cu8, status = pbm.restate_call(list(src), boxes, list(range(B)), clip_px, flags=2 | 4)
        assert not status.any()
        clip = pbm.planes(cu8, status, True)
    return sizes, u8, tensors, mask, clip
