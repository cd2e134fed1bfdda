"""What the crop pre-processing kernels (hg_preproc.hip: preproc_tables_kernel, preproc_h_kernel, preproc_v_kernel, and the geometry
hg_preprocess_crops works out on the host) are held to: oracle/preprocess_oracle.py - integer arithmetic, pinned bit for bit to Pillow
by tests/test_preproc_model.py where PIL imports - and the rule

    uint8 crops   array_equal
    fp32 planes   array_equal with the oracle's fp32 expression ((u / 255) - mean) / sd, two IEEE divisions

at every committed case.  A plain module beside the tests (tests/test_preproc_model.py, tests/test_gpu_preproc_exact.py import it): no
fixtures, no GPU, no library.

`restate()` is the CPU restatement of the three kernels in THEIR structure: the 24-word header of the host, one flat int32 table per box
laid out h_bounds | h_kk[ks_h] | v_bounds | v_kk[ks_v], the horizontal pass over the rows [row_lo, row_lo + n_rows) of the virtual source
into a uint8 scratch, the vertical pass that rebases its bounds by row_lo.  With the mutants (`MUTANTS`) that
tests/test_preproc_model.py proves change at least one output byte of the committed cases:

    tables_256        tables filled for i < 256 only (the tables loop's second trip missing; the entries stay zero)
    crop_half_up      centre-crop offset floor(d / 2 + 0.5) for round-half-to-even
    pad_ceil          square-padding offset ceil((side - short) / 2)
    ksv_stride        the horizontal pass strides h_kk by ks_v
    no_rebase         vertical bounds not rebased by row_lo (rows outside the scratch read as 0)
    bg_swapped        background channels read in the order B, G, R
    outside_bg        pixels of the crop outside the image take the background, not 0
    clip_wraps        (acc >> 22) & 255 for the saturating clip
    weights_trunc     fixed-point weights rounded toward zero
    identity_axis     a pass skipped when the OTHER axis is the identity (source side equal to target side)

Cases (`CASES`): `noise` is a seeded 301 x 457 uint8 noise image, `step` a 120 x 160 image of 0 / 255 blocks three pixels wide under
a ramp of step edges, whose bicubic overshoot saturates clip8 at both ends in both passes (asserted).  The breadth of geometry sits at
n_px 31 / 97 / 257, where the oracle costs milliseconds per box; n_px 224 .. 518 carry at most four boxes a case (the oracle's cost
grows with the resized side: a 1-pixel-wide box 296 pixels high would be resized to 336 x 99 456 before the centre crop and take seconds, so such boxes sit at 31).
"""
import functools
import math

import numpy as np

from oracle import preprocess_oracle as po

PREC = 22
MUTANTS = ("tables_256", "crop_half_up", "pad_ceil", "ksv_stride", "no_rebase", "bg_swapped", "outside_bg", "clip_wraps",
           "weights_trunc", "identity_axis")
BG = (122, 116, 104)          # three distinct channel values


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "noise":
        return np.random.RandomState(7).randint(0, 256, size=(301, 457, 3)).astype(np.uint8)
    assert name == "step"
    yy, xx = np.mgrid[0:120, 0:160]
    img = np.where(((yy // 3) + (xx // 3)) % 2 == 0, 255, 0)
    img = np.stack([img, np.where(xx < 80, 0, 255), np.where(yy % 40 < 20, 255, 0)], -1)
    return np.ascontiguousarray(img.astype(np.uint8))


def _case(name, n_px, img, boxes, pad=False, bg=(0, 0, 0), stretch=False, imagenet=False, u8=True):
    return {"name": name, "n_px": n_px, "image": img, "boxes": np.asarray(boxes, np.int32).reshape(-1, 4), "pad_square": pad,
            "background": bg, "stretch": stretch, "imagenet_norm": imagenet, "return_u8": u8}


def _n33():
    rng = np.random.RandomState(33)
    out = []
    for _ in range(33):
        x0, y0 = rng.randint(-20, 440), rng.randint(-20, 290)
        out.append((x0, y0, x0 + rng.randint(1, 90), y0 + rng.randint(1, 90)))
    return out


GEO = [(7, 9, 10, 12),               # upscale x 10
       (-20, -40, 352, 340),         # downscale x 12 (372 x 380: ks 49 / 51), leaves the image on three sides
       (10, 10, 41, 100),            # cw == 31, ch != 31
       (10, 10, 100, 41),            # ch == 31, cw != 31
       (10, 10, 41, 42),             # resized - n_px = 1: the half is 0.5
       (10, 10, 41, 44),             # resized - n_px = 3: the half is 1.5
       (50, 60, 81, 91),             # n_px x n_px
       (3, 4, 4, 300), (0, 5, 457, 6),                                            # 1 x N, N x 1
       (500, 400, 530, 440), (-50, -50, -10, -5),                                 # wholly outside
       (-10, 50, 30, 90), (440, 50, 470, 100), (100, -12, 150, 20), (100, 280, 140, 320)]   # across each edge
PAD = [(20, 30, 61, 50), (20, 30, 60, 50), (20, 30, 40, 71), (20, 30, 40, 70),    # cw > ch by 21 / 20, ch > cw by 21 / 20
       (-5, 290, 40, 310), (7, 9, 8, 40)]
MIXED = [(7, 9, 10, 12), (-20, 100, 352, 140), (200, -40, 240, 332), (9, 7, 12, 10), (0, 0, 31, 97), (0, 0, 97, 31)]
STEP = [(0, 0, 160, 120), (10, 10, 100, 41), (30, 20, 61, 110), (75, 35, 90, 50)]

CASES = [
    _case("geo31", 31, "noise", GEO),
    _case("geo31_step", 31, "step", STEP),
    _case("pad31", 31, "noise", PAD, pad=True, bg=BG),
    _case("pad31_step", 31, "step", STEP, pad=True, bg=BG),
    _case("mixed31_stretch", 31, "noise", MIXED, stretch=True, imagenet=True),
    _case("n33_at_31", 31, "noise", _n33(), u8=False),
    _case("one_box_31", 31, "noise", [(100, 100, 190, 160)]),
    _case("geo97", 97, "noise", [(7, 9, 10, 12), (0, 0, 457, 301), (10, 10, 107, 200), (10, 10, 200, 107), (10, 10, 107, 108),
                                 (10, 10, 107, 110), (5, 5, 102, 102), (440, 280, 470, 320)]),
    _case("mixed97_stretch", 97, "step", STEP + [(-10, -10, 170, 130), (20, 10, 117, 43), (20, 10, 53, 107)], stretch=True, imagenet=True),
    _case("pad97", 97, "noise", PAD, pad=True, bg=BG, u8=False),
    _case("plain224", 224, "noise", [(100, 100, 325, 324), (-30, 20, 200, 331)], u8=False),
    _case("pad255", 255, "noise", [(20, 30, 61, 50), (0, 0, 255, 300)], pad=True, bg=BG),
    _case("stretch256", 256, "step", [(0, 0, 160, 120), (30, 20, 61, 110)], stretch=True, imagenet=True),
    _case("geo257", 257, "noise", [(7, 9, 10, 12), (10, 10, 267, 300), (10, 10, 300, 267), (100, 20, 357, 277), (3, 4, 4, 40),
                                   (440, 50, 470, 100)]),
    _case("step257", 257, "step", STEP[:3]),
    _case("pad257_stretch", 257, "noise", [(20, 30, 61, 50), (20, 30, 40, 71), (-20, -40, 352, 340)], pad=True, bg=BG, stretch=True),
    _case("plain336", 336, "noise", [(100, 100, 325, 324), (7, 9, 10, 12), (10, -10, 346, 290), (0, 0, 457, 301)]),
    _case("step336_stretch", 336, "step", STEP[:3], stretch=True, imagenet=True),
    _case("pad336", 336, "noise", [(20, 30, 61, 50), (20, 30, 40, 71)], pad=True, bg=BG, u8=False),
    _case("plain518", 518, "noise", [(100, 100, 325, 324), (0, 0, 457, 301)]),
]
BY_NAME = {c["name"]: c for c in CASES}
SIZES = (31, 97, 224, 255, 256, 257, 336, 518)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(uint8 [n, n_px, n_px, 3], float32 [n, 3, n_px, n_px]) of the oracle.  Cached: leave unchanged."""
    c = BY_NAME[name]
    u8, f = po.preprocess_boxes(image(c["image"]), c["boxes"], c["n_px"], c["pad_square"], c["background"], c["stretch"],
                                c["imagenet_norm"])
    u8.setflags(write=False)
    f.setflags(write=False)
    return u8, f


# ---- the host's geometry (hg_preprocess_crops) ------------------------------------------------------------------------------------
def _fs(i, o):
    sc = i / o
    return sc, (1.0 if sc < 1.0 else sc)


def _taps(i, o):
    return int(math.ceil(2.0 * _fs(i, o)[1])) * 2 + 1


def _first_tap(i, o, idx):
    sc, fs = _fs(i, o)
    return max(int((idx + 0.5) * sc - 2.0 * fs + 0.5), 0)


def _end_tap(i, o, idx):
    sc, fs = _fs(i, o)
    return min(int((idx + 0.5) * sc + 2.0 * fs + 0.5), i)


def header(box, n_px, pad_square, stretch, mutant=None):
    x0, y0, x1, y1 = (int(v) for v in box)
    cw, ch = x1 - x0, y1 - y0
    sw, sh, px, py = cw, ch, 0, 0
    if pad_square and cw != ch:
        up = 1 if mutant == "pad_ceil" else 0
        if cw > ch:
            py = (cw - ch + up) // 2
        else:
            px = (ch - cw + up) // 2
        sw = sh = max(cw, ch)
    if stretch:
        nw = nh = n_px
    elif sw <= sh:
        nw, nh = n_px, int(n_px * sh / sw)
    else:
        nw, nh = int(n_px * sw / sh), n_px
    if mutant == "crop_half_up":
        left, top = math.floor((nw - n_px) / 2.0 + 0.5), math.floor((nh - n_px) / 2.0 + 0.5)
    else:
        left, top = round((nw - n_px) / 2.0), round((nh - n_px) / 2.0)
    row_lo = _first_tap(sh, nh, top)
    return {"x0": x0, "y0": y0, "cw": cw, "ch": ch, "px": px, "py": py, "sw": sw, "sh": sh, "ks_h": _taps(sw, nw), "ks_v": _taps(sh, nh),
            "row_lo": row_lo, "n_rows": _end_tap(sh, nh, top + n_px - 1) - row_lo, "nw": nw, "nh": nh, "left": left, "top": top}


# ---- preproc_tables_kernel ----------------------------------------------------------------------------------------------------------
def fill_tables(h, n_px, mutant=None):
    """the flat table of one box: h_bounds[n_px][2] | h_kk[n_px][ks_h] | v_bounds[n_px][2] | v_kk[n_px][ks_v]"""
    arr = np.zeros(n_px * (4 + h["ks_h"] + h["ks_v"]), np.int64)
    for axis in (0, 1):
        in_size, out_size = (h["sh"], h["nh"]) if axis else (h["sw"], h["nw"])
        first, ks = (h["top"], h["ks_v"]) if axis else (h["left"], h["ks_h"])
        base = 2 * n_px + n_px * h["ks_h"] if axis else 0
        kk0 = base + 2 * n_px
        scale = in_size / out_size
        filterscale = 1.0 if scale < 1.0 else scale
        support, ss = 2.0 * filterscale, 1.0 / filterscale
        for i in range(min(n_px, 256) if mutant == "tables_256" else n_px):
            center = ((first + i) + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size) - xmin
            w = [po._bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            for x in range(min(ks, xmax)):
                v = w[x] / ww if ww != 0.0 else w[x]
                if mutant == "weights_trunc":
                    arr[kk0 + i * ks + x] = int(v * (1 << PREC))
                else:
                    arr[kk0 + i * ks + x] = int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC))
            arr[base + 2 * i], arr[base + 2 * i + 1] = xmin, xmax
    return arr


def _clip8(acc, mutant):
    v = acc >> PREC
    return (v & 255) if mutant == "clip_wraps" else np.clip(v, 0, 255)


def _virtual_rows(img, h, bg, mutant):
    """rows [row_lo, row_lo + n_rows) of the virtual source (the crop pasted into src_w x src_h of background): int64 [n_rows, sw, 3]"""
    H, W = img.shape[:2]
    cy = h["row_lo"] + np.arange(h["n_rows"]) - h["py"]
    cx = np.arange(h["sw"]) - h["px"]
    in_crop = ((cy >= 0) & (cy < h["ch"]))[:, None] & ((cx >= 0) & (cx < h["cw"]))[None]
    iy, ix = h["y0"] + cy, h["x0"] + cx
    in_img = in_crop & ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None]
    pix = img[np.clip(iy, 0, H - 1)][:, np.clip(ix, 0, W - 1)].astype(np.int64)
    bgv = np.asarray(bg[::-1] if mutant == "bg_swapped" else bg, np.int64)
    outside = bgv if mutant == "outside_bg" else np.zeros(3, np.int64)
    return np.where(in_crop[..., None], np.where(in_img[..., None], pix, outside), bgv)


def restate_box(img, box, n_px, pad_square=False, background=(0, 0, 0), stretch=False, mutant=None, stats=None):
    """one box through the three kernels -> uint8 [n_px, n_px, 3].  stats: a dict that receives the extreme accumulators of both passes"""
    h = header(box, n_px, pad_square, stretch, mutant)
    arr = fill_tables(h, n_px, mutant)
    V = _virtual_rows(img, h, background, mutant)
    o = np.arange(n_px)
    # horizontal pass
    if mutant == "identity_axis" and h["sh"] == h["nh"] and h["sw"] != h["nw"]:
        tmp = V[:, np.clip(h["left"] + o, 0, h["sw"] - 1)]
        acc_h = tmp << PREC
    else:
        first, cnt = arr[2 * o], arr[2 * o + 1]
        stride = h["ks_v"] if mutant == "ksv_stride" else h["ks_h"]
        acc_h = np.full((h["n_rows"], n_px, 3), 1 << (PREC - 1), np.int64)
        for j in range(int(cnt.max()) if n_px else 0):
            k = np.where(j < cnt, arr[np.minimum(2 * n_px + o * stride + j, arr.size - 1)], 0)
            acc_h += V[:, np.clip(first + j, 0, h["sw"] - 1)] * k[None, :, None]
        tmp = _clip8(acc_h, mutant)
    # vertical pass
    vbase = 2 * n_px + n_px * h["ks_h"]
    if mutant == "identity_axis" and h["sw"] == h["nw"] and h["sh"] != h["nh"]:
        out = tmp[np.clip(h["top"] + o - h["row_lo"], 0, h["n_rows"] - 1)]
        acc_v = out << PREC
    else:
        first, cnt = arr[vbase + 2 * o] - (0 if mutant == "no_rebase" else h["row_lo"]), arr[vbase + 2 * o + 1]
        acc_v = np.full((n_px, n_px, 3), 1 << (PREC - 1), np.int64)
        for j in range(int(cnt.max()) if n_px else 0):
            k = np.where(j < cnt, arr[vbase + 2 * n_px + o * h["ks_v"] + j], 0)
            r = first + j
            rows = np.where(((r >= 0) & (r < h["n_rows"]))[:, None, None], tmp[np.clip(r, 0, h["n_rows"] - 1)], 0)
            acc_v += rows * k[:, None, None]
        out = _clip8(acc_v, mutant)
    if stats is not None:
        for key, a in (("h", acc_h), ("v", acc_v)):
            stats[key + "_below"] = stats.get(key + "_below", 0) + int((a < 0).sum())
            stats[key + "_above"] = stats.get(key + "_above", 0) + int((a >= (256 << PREC)).sum())
    return out.astype(np.uint8)


def restate(name, mutant=None, stats=None):
    """the case through the restatement -> (uint8 [n, n_px, n_px, 3], float32 [n, 3, n_px, n_px])"""
    assert mutant is None or mutant in MUTANTS, mutant
    c = BY_NAME[name]
    img = image(c["image"])
    u8 = np.stack([restate_box(img, b, c["n_px"], c["pad_square"], c["background"], c["stretch"], mutant, stats) for b in c["boxes"]])
    return u8, planes(u8, c["imagenet_norm"])


def planes(u8, imagenet_norm):
    """the kernel's 3 x 256 table applied to uint8 [n, n_px, n_px, 3]: ((u / 255) - mean) / sd in fp32 -> [n, 3, n_px, n_px]"""
    m, sd = (po.IMAGENET_MEAN, po.IMAGENET_STD) if imagenet_norm else (po.CLIP_MEAN, po.CLIP_STD)
    lut = (np.arange(256, dtype=np.float32)[None] / np.float32(255.0) - np.asarray(m, np.float32)[:, None]) / np.asarray(sd, np.float32)[:, None]
    out = np.empty((u8.shape[0], 3) + u8.shape[1:3], np.float32)
    for ch in range(3):
        out[:, ch] = lut[ch][u8[..., ch]]
    return out


# ---- what the cases must exercise (tests assert these) ----------------------------------------------------------------------------
def geometry(name):
    c = BY_NAME[name]
    return [header(b, c["n_px"], c["pad_square"], c["stretch"]) for b in c["boxes"]]


def scratch_bytes(name):
    c = BY_NAME[name]
    return [h["n_rows"] * c["n_px"] * 3 for h in geometry(name)]
