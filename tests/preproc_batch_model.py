"""CPU restatement of the batched crop pre-processing (hoigen_amd/csrc/hg_preproc_batch.hip, hg_preproc_geom.h) in ITS structure, for
tests/test_preproc_batch_model.py and tests/test_gpu_preproc_batch.py.  A plain module: no fixtures, no GPU, no library.

    geometry()      preb_geometry: the 24-word header and the status of one crop, from the box alone - band height (word 12), the columns
                    [col_lo, col_lo + n_cols) of the virtual source a row can need (18, 19), status (20), image (21)
    restate_call()  prebatch_tables_kernel's table slots per axis, then prebatch_resample_kernel: bands of header word 12 output rows; per
                    band the source rows [rlo, rhi) in trips of rows_per_trip through a row BUFFER of raw image bytes (16-byte chunks
                    from the 16-byte boundary below the row's first byte: `lead`), the horizontal pass into a WINDOW of PREB_WIN_ROWS
                    uint8 rows at slot = source row - rlo, the vertical pass from the window with its slot guard.  Buffer and window
                    start every band full of 0xAA, as LDS starts full of whatever the workgroup before left there.

What it is held to: tests/preproc_cases.py - `expected(name)` of every committed case byte for byte, with the cases grouped into CALLS of
several images as the GPU test runs them - and the cases of its own below.  Mutants (`MUTANTS`) that the test proves change at least one
byte of a case:

    band_seam        a band's last source row taken from its last output row but one
    no_rebase        window slot = source row, not source row - rlo (slots beyond the band's rows read as 0: the kernel's guard)
    target_fp32      resize target int(fp32(n_px * long) / fp32(short))
    crop_half_up     centre-crop offset floor(d / 2 + 0.5) for round-half-to-even
    taps_ge          the tap limit compared with >=: a box of exactly PREB_MAX_TAPS taps refused
    image_by_crop    the image table indexed by the crop number (modulo B), not by crop_image
    refused_writes   a crop above the tap limit not refused: resampled with its tables cut at the limit

Cases of its own (`OWN`): `own224` - n_px 224, a box that leaves `noise` on all four sides at a downscale of 4.02; `own31_limit` - a box of
exactly 65 taps on both axes (496 / 31 = 16), one of 67 (497 / 31: refused, status 2, zero bytes), and a 495 x 542 009 box centred on the
image whose resize target 31 * 542 009 / 495 = 33 943.99 is 33 943 in double and 33 944 in fp32.  Their expectations come from the oracle
(oracle/preprocess_oracle.py), except the tall box: the oracle materialises the crop, so that one is held to preproc_cases.restate_box,
the restatement of the per-image kernels, which tests/test_preproc_model.py pins to the oracle.
"""
import functools
import math
import os
import re

import numpy as np

import preproc_cases as pc
from oracle import preprocess_oracle as po

PREC = 22
MAX_IMAGES, MAX_N, MAX_NPX, MAX_TAPS, MAX_COORD, BAND, WIN_ROWS, HDR = 64, 4096, 518, 65, 1 << 20, 16, 72, 24
EMPTY, TAPS, IMAGE = 1, 2, 4
HCACHE_NPX, HCACHE_TAPS = 336, 13
MUTANTS = ("band_seam", "no_rebase", "target_fp32", "crop_half_up", "taps_ge", "image_by_crop", "refused_writes")
STALE = 0xAA

LIMIT_BOX, ABOVE_BOX, TALL_BOX = (-20, -20, 476, 476), (-20, -20, 477, 477), (-20, -270854, 475, 271155)
OWN = [
    pc._case("own224", 224, "noise", [(-300, -300, 600, 600)]),
    pc._case("own31_limit", 31, "noise", [LIMIT_BOX, ABOVE_BOX, TALL_BOX, (100, 100, 190, 160)]),
]
OWN_BY_NAME = {c["name"]: c for c in OWN}

GEOM_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hoigen_amd", "csrc", "hg_preproc_geom.h")


def header_constants():
    """every `static constexpr int PREB_... = ...` of hg_preproc_geom.h -> {name: value}"""
    out = {}
    for decl in re.findall(r"static constexpr int ([^;]+);", open(GEOM_H).read()):
        for part in decl.split(","):
            name, value = part.split("=")
            out[name.strip()] = int(eval(value, {"__builtins__": {}}, dict(out)))
    return out


def header_functions():
    """the one-line sizing functions `preb_...(int n_px) { return ...; }` of hg_preproc_geom.h as Python functions of n_px (C's integer
    division restated as //): the kernel's own LDS and workspace formulas, whatever their layout in the file"""
    consts, fns = header_constants(), {}
    for name, expr in re.findall(r"HG_GEOM_FN\s+(?:int|size_t)\s+(preb_\w+)\(int n_px\)\s*\{\s*return\s+(.*?);\s*\}", open(GEOM_H).read()):
        code = compile(expr.replace("(size_t)", "").replace("/", "//"), name, "eval")
        fns[name] = (lambda code: lambda n_px: int(eval(code, {"__builtins__": {}}, dict(consts, n_px=n_px, **fns))))(code)
    return fns


def case(name):
    return pc.BY_NAME.get(name) or OWN_BY_NAME[name]


def max_cols(n_px):
    return 16 * n_px + 49


def win_stride(n_px):
    return (n_px * 3 + 15) // 16 * 16


def rowbuf_bytes(n_px):
    return (max_cols(n_px) * 3 + 32 + 15) // 16 * 16


def hcache_words(n_px):
    """words of LDS for a crop's horizontal weights (kept there when n_px * ks_h fits: the same values, nearer)"""
    return ((n_px * HCACHE_TAPS if n_px <= HCACHE_NPX else 0) + 3) // 4 * 4


def lds_bytes(n_px):
    return 3 * 256 * 4 + BAND * (MAX_TAPS + 2) * 4 + WIN_ROWS * 4 + 64 + rowbuf_bytes(n_px) + WIN_ROWS * win_stride(n_px) + hcache_words(n_px) * 4


def flags_of(c):
    return (1 if c["pad_square"] else 0) | (2 if c["stretch"] else 0) | (4 if c["imagenet_norm"] else 0)


# ---- preb_geometry ------------------------------------------------------------------------------------------------------------------
def geometry(box, image, B, n_px, flags, background=0, mutant=None):
    """-> (h[24], status)"""
    h = [0] * HDR
    status = 0
    x0, y0, x1, y1 = (int(v) for v in box)
    if image < 0 or image >= B:
        status |= IMAGE
    cw, ch = x1 - x0, y1 - y0
    if cw <= 0 or ch <= 0:
        status |= EMPTY
    elif any(abs(v) > MAX_COORD for v in (x0, y0, x1, y1)):
        status |= TAPS
    h[13], h[21] = background, image
    if not status & (EMPTY | TAPS):
        sw, sh, px, py = cw, ch, 0, 0
        if (flags & 1) and cw != ch:
            if cw > ch:
                py = (cw - ch) // 2
            else:
                px = (ch - cw) // 2
            sw = sh = max(cw, ch)
        div = (lambda a, b: int(np.float32(a) / np.float32(b))) if mutant == "target_fp32" else (lambda a, b: int(a / b))
        if flags & 2:
            nw = nh = n_px
        elif sw <= sh:
            nw, nh = n_px, div(n_px * sh, sw)
        else:
            nw, nh = div(n_px * sw, sh), n_px
        if mutant == "crop_half_up":
            left, top = math.floor((nw - n_px) / 2.0 + 0.5), math.floor((nh - n_px) / 2.0 + 0.5)
        else:
            left, top = round((nw - n_px) / 2.0), round((nh - n_px) / 2.0)
        ks_h, ks_v = pc._taps(sw, nw), pc._taps(sh, nh)
        over = (ks_h >= MAX_TAPS or ks_v >= MAX_TAPS) if mutant == "taps_ge" else (ks_h > MAX_TAPS or ks_v > MAX_TAPS)
        if over and mutant == "refused_writes":
            ks_h, ks_v, over = min(ks_h, MAX_TAPS), min(ks_v, MAX_TAPS), False
        if over:
            status |= TAPS
        else:
            row_lo = pc._first_tap(sh, nh, top)
            n_rows = pc._end_tap(sh, nh, top + n_px - 1) - row_lo
            col_lo = pc._first_tap(sw, nw, left)
            n_cols = pc._end_tap(sw, nw, left + n_px - 1) - col_lo
            sc = sh / nh
            fs = 1.0 if sc < 1.0 else sc
            f = (WIN_ROWS - 4.0 * fs - 2.0) / sc
            bh = BAND if f >= BAND - 1 else max(int(f) + 1, 1)
            if n_cols > max_cols(n_px) or n_cols < 0 or n_rows < 0:
                status |= TAPS
            elif not status:
                h[0:13] = [x0, y0, cw, ch, px, py, sw, sh, ks_h, ks_v, row_lo, n_rows, bh]
                h[14:20] = [nw, nh, left, top, col_lo, n_cols]
    h[20] = status
    return h, status


def as_dict(h):
    """the header as preproc_cases.header names it"""
    keys = {"x0": 0, "y0": 1, "cw": 2, "ch": 3, "px": 4, "py": 5, "sw": 6, "sh": 7, "ks_h": 8, "ks_v": 9, "row_lo": 10, "n_rows": 11,
            "nw": 14, "nh": 15, "left": 16, "top": 17}
    return {k: h[i] for k, i in keys.items()}


def axis_tables(h, n_px):
    """prebatch_tables_kernel: per axis (bounds [n_px][2], kk [n_px][ks]) - preb_fill_index is preproc_tables_kernel's arithmetic
    (tests/test_preproc_batch_host.py holds the header's text to preproc_cases.fill_tables word for word)"""
    d = as_dict(h)
    arr = pc.fill_tables(d, n_px)
    ksh, ksv = d["ks_h"], d["ks_v"]
    hb = arr[:2 * n_px].reshape(n_px, 2)
    hk = arr[2 * n_px:2 * n_px + n_px * ksh].reshape(n_px, ksh)
    base = 2 * n_px + n_px * ksh
    vb = arr[base:base + 2 * n_px].reshape(n_px, 2)
    vk = arr[base + 2 * n_px:].reshape(n_px, ksv)
    return hb, hk, vb, vk


def _clip8(acc):
    return np.clip(acc >> PREC, 0, 255)


def _taps_of(bounds, kk, limit):
    """(index, weight) of tap j for every output index, weight 0 beyond the count (and beyond `limit` taps: refused_writes)"""
    cnt = np.minimum(bounds[:, 1], limit)
    for j in range(int(cnt.max()) if cnt.size else 0):
        yield j, bounds[:, 0] + j, np.where(j < cnt, kk[:, min(j, kk.shape[1] - 1)], 0)


def resample_crop(img, h, n_px, addr=0, mutant=None, seen=None):
    """prebatch_resample_kernel for one accepted crop -> uint8 [n_px, n_px, 3].  `addr`: the image's base address modulo 16."""
    H, W = img.shape[:2]
    flat = img.reshape(-1)
    x0, y0, cw, ch, px, py = h[0:6]
    bg = np.array([h[13] & 255, (h[13] >> 8) & 255, (h[13] >> 16) & 255], np.int64)
    bh, col_lo, n_cols = h[12], h[18], h[19]
    hb, hk, vb, vk = axis_tables(h, n_px)
    limit = MAX_TAPS
    cxs, cxe = max(col_lo - px, 0), min(col_lo + n_cols - px, cw)
    ixs, ixe = max(x0 + cxs, 0), min(x0 + cxe, W)
    n_in = max(ixe - ixs, 0)
    lstride = (n_in * 3 + 15) // 16 * 16 + 16
    rbytes, wstride = rowbuf_bytes(n_px), win_stride(n_px)
    per_trip = rbytes // lstride
    assert per_trip >= 1
    out = np.zeros((n_px, n_px, 3), np.uint8)
    cols = col_lo + np.arange(n_cols)                 # virtual columns a row can need
    cx = cols - px
    col_in_crop = (cx >= 0) & (cx < cw)
    ix = x0 + cx
    col_in_img = col_in_crop & (ix >= ixs) & (ix < ixe)
    for band in range((n_px + bh - 1) // bh):
        r0, r1 = band * bh, min(band * bh + bh, n_px)
        last = max(r0, r1 - 2) if mutant == "band_seam" else r1 - 1
        rlo = int(vb[r0, 0])
        nr = int(vb[last, 0] + vb[last, 1]) - rlo
        if mutant is None:
            assert 0 <= nr <= WIN_ROWS, (nr, h)
        nr = min(nr, WIN_ROWS)
        if seen is not None:
            seen["max_rows"] = max(seen.get("max_rows", 0), nr)
            seen["trips"] = max(seen.get("trips", 0), -(-nr // per_trip))
            seen["min_bh"] = min(seen.get("min_bh", BAND), bh)
        win = np.full((WIN_ROWS, wstride), STALE, np.int64)
        for b0 in range(0, nr, per_trip):
            rb = min(nr - b0, per_trip)
            rowbuf = np.full(rbytes, STALE, np.int64)
            V = np.zeros((rb, n_cols, 3), np.int64)
            for q in range(rb):
                cy = rlo + b0 + q - py
                iy = y0 + cy
                row_in_crop = 0 <= cy < ch
                row_in_img = row_in_crop and 0 <= iy < H
                lead = 0
                if row_in_img and n_in:
                    off = (iy * W + ixs) * 3
                    lead = (addr + off) & 15
                    nch = -(-(lead + n_in * 3) // 16)            # the 16-byte chunks that hold a byte of the row; those across an end
                    assert nch * 16 <= lstride                   # of the image are read byte by byte, 0 outside
                    idx = off - lead + np.arange(nch * 16)
                    ok = (idx >= 0) & (idx < flat.size)
                    rowbuf[q * lstride:q * lstride + nch * 16] = np.where(ok, flat[np.clip(idx, 0, flat.size - 1)], 0)
                if not row_in_crop:
                    V[q] = bg
                else:
                    V[q] = np.where(col_in_crop[:, None], 0, bg)
                    if row_in_img and n_in:
                        src = q * lstride + lead + (ix[col_in_img] - ixs) * 3
                        assert src.size == 0 or (src.min() >= 0 and src.max() + 2 < (q + 1) * lstride)
                        V[q, col_in_img] = rowbuf[src[:, None] + np.arange(3)]
            acc = np.full((rb, n_px, 3), 1 << (PREC - 1), np.int64)
            for j, first, k in _taps_of(hb, hk, limit):
                acc += V[:, np.clip(first - col_lo, 0, max(n_cols - 1, 0))] * k[None, :, None]
            win[b0:b0 + rb, :n_px * 3] = _clip8(acc).reshape(rb, n_px * 3)
        rows = np.arange(r0, r1)
        acc = np.full((r1 - r0, n_px * 3), 1 << (PREC - 1), np.int64)
        for j, first, k in _taps_of(vb[rows], vk[rows], limit):
            slot = first - (0 if mutant == "no_rebase" else rlo)
            ok = (slot >= 0) & (slot < nr)                       # the kernel's guard
            acc += np.where(ok[:, None], win[np.clip(slot, 0, WIN_ROWS - 1), :n_px * 3], 0) * k[:, None]
        out[r0:r1] = _clip8(acc).reshape(r1 - r0, n_px, 3)
    return out


def restate_call(images, boxes, crop_image, n_px, flags=0, background=(0, 0, 0), mutant=None, addr=0, seen=None):
    """hg_preprocess_batch: images a list of uint8 [H, W, 3]; boxes [n][4]; crop_image [n] -> (uint8 [n, n_px, n_px, 3], status [n]).
    A refused crop has zero bytes (and NaN planes: planes())."""
    assert mutant is None or mutant in MUTANTS, mutant
    B = len(images)
    bg = (background[0] & 255) | ((background[1] & 255) << 8) | ((background[2] & 255) << 16)
    u8 = np.zeros((len(boxes), n_px, n_px, 3), np.uint8)
    status = np.zeros(len(boxes), np.int32)
    for i, (box, im) in enumerate(zip(boxes, crop_image)):
        h, status[i] = geometry(box, int(im), B, n_px, flags, bg, mutant)
        if status[i]:
            continue                                             # before anything is indexed
        img = images[i % B] if mutant == "image_by_crop" else images[h[21]]
        u8[i] = resample_crop(img, h, n_px, addr, mutant, seen)
    return u8, status


def planes(u8, status, imagenet_norm):
    out = pc.planes(u8, imagenet_norm)
    out[np.asarray(status) != 0] = np.nan
    return out


# ---- calls of several images: the committed cases grouped by (n_px, flags, background), and the module's own ----------------------
def _calls():
    groups = {}
    for c in pc.CASES + OWN:
        groups.setdefault((c["n_px"], flags_of(c), tuple(c["background"])), []).append(c["name"])
    return list(groups.values())


CALLS = _calls()


def call_inputs(names):
    """-> (image names of the call's table, boxes [n, 4] int32, crop_image [n] int32, slices {case name: slice of the crops})"""
    imgs, boxes, owner, slices, at = [], [], [], {}, 0
    for nme in names:
        c = case(nme)
        if c["image"] not in imgs:
            imgs.append(c["image"])
        boxes.append(c["boxes"])
        owner += [imgs.index(c["image"])] * len(c["boxes"])
        slices[nme] = slice(at, at + len(c["boxes"]))
        at += len(c["boxes"])
    return imgs, np.concatenate(boxes).astype(np.int32), np.asarray(owner, np.int32), slices


@functools.lru_cache(maxsize=None)
def expected(name):
    """(uint8 [n, n_px, n_px, 3], float32 [n, 3, n_px, n_px], status [n]) of a case.  Cached: leave unchanged."""
    if name in pc.BY_NAME:
        u8, f = pc.expected(name)
        return u8, f, np.zeros(u8.shape[0], np.int32)
    c = OWN_BY_NAME[name]
    img = pc.image(c["image"])
    u8 = np.zeros((len(c["boxes"]), c["n_px"], c["n_px"], 3), np.uint8)
    status = np.zeros(len(c["boxes"]), np.int32)
    for i, b in enumerate(c["boxes"]):
        b = tuple(int(v) for v in b)
        if b == ABOVE_BOX:
            status[i] = TAPS
        elif b == TALL_BOX:
            u8[i] = pc.restate_box(img, b, c["n_px"], c["pad_square"], c["background"], c["stretch"])
        else:
            u8[i] = po.preprocess_boxes(img, np.asarray([b], np.int32), c["n_px"], c["pad_square"], c["background"], c["stretch"],
                                        c["imagenet_norm"])[0][0]
    f = planes(u8, status, c["imagenet_norm"])
    for a in (u8, f, status):
        a.setflags(write=False)
    return u8, f, status


def restate_named_call(names, mutant=None, addr=0, seen=None):
    c = case(names[0])
    imgs, boxes, owner, slices = call_inputs(names)
    u8, status = restate_call([pc.image(i) for i in imgs], boxes, owner, c["n_px"], flags_of(c), c["background"], mutant, addr, seen)
    return u8, status, slices
