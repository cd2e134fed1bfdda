"""The committed cases of the detector's two views of a batch (hg_detector_views), for tests/test_detector_views_*.py,
tests/test_gpu_detector_views.py and tests/golden/make_golden_detector_views.py.  A plain module: no fixtures, no GPU, no library.

Two settings (size, max_size, clip_px): `a` = (40, 66, 16) and `b` = (48, 80, 31).  Every case is an image of (h, w) below, `noise`
(seeded, per case) unless its name says otherwise; the sizes are written for a setting's size S:

    landscape, portrait, square     (30, 47), (47, 30), (33, 33)
    identity                        (S, S + 15): the short side already equals size -> the image itself
    max_w, max_h                    (30, 90), (90, 30): max_size limits the long side
    thin                            (5, 132): max_size * 5 / 132 = 2.5 at `a`, Python's round gives 2 -> (2, 52); half-up would give 3
    down12                          (12 S, 12 S + 20): a downscale of 12, 49 taps, a band of two output rows
    w63, w64, w65                   (2 S, 126 / 128 / 130) -> (S, 63 / 64 / 65): the strip width of the kernel - 1, + 0, + 1
    h31, h32, h33                   (62 / 64 / 66, 2 M) -> (31 / 32 / 33, M): the band height of the kernel - 1, + 0, + 1, max_size-limited
    up_band                         (16, 33) at `a`, (16, 40) at `b` -> (32, M): an upscale whose one band is exactly full
    step                            (30, 47): 0 | 255 across a vertical and a horizontal edge: both ends of clip8 after each pass
    black, white                    (20, 27) of 0 and of 255
The strip width and band height are asserted against the library's own constants in tests/test_detector_views_host.py.

`expected(setting, name)` is the ORACLE's result (oracle/preprocess_oracle.py::resize_bicubic, twice; ToTensor + Normalize in fp32), cached;
`CALLS[setting]` groups the cases into calls of 1, 3 and 7 images, once in the order above and once reversed."""
import functools

import numpy as np

from oracle import preprocess_oracle as po

SETTINGS = {"a": (40, 66, 16), "b": (48, 80, 31)}
FULL = (800, 1333, 224)                      # the reference's own setting: one call of a 480 x 640 and a 640 x 427 image (GPU test)
FULL_SHAPES = [(480, 640), (640, 427)]
STRIP, BAND = 64, 32                         # DV_STRIP, DV_BAND of hoigen_amd/csrc/hg_detector_views_geom.h


def shapes(setting):
    S, M, _ = SETTINGS[setting]
    return {"landscape": (30, 47), "portrait": (47, 30), "square": (33, 33), "identity": (S, S + 15), "max_w": (30, 90), "max_h": (90, 30),
            "thin": (5, 132), "down12": (12 * S, 12 * S + 20),
            "w63": (2 * S, 2 * STRIP - 2), "w64": (2 * S, 2 * STRIP), "w65": (2 * S, 2 * STRIP + 2),
            "h31": (2 * BAND - 2, 2 * M), "h32": (2 * BAND, 2 * M), "h33": (2 * BAND + 2, 2 * M), "up_band": (16, M // 2),
            "step": (30, 47), "black": (20, 27), "white": (20, 27)}


NAMES = list(shapes("a"))


@functools.lru_cache(maxsize=None)
def image(setting, name):
    h, w = shapes(setting)[name]
    if name == "black":
        return np.zeros((h, w, 3), np.uint8)
    if name == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if name == "step":
        im = np.zeros((h, w, 3), np.uint8)
        im[:, w // 2:] = 255
        im[h // 2:, :, 1] ^= 255
        return im
    rng = np.random.RandomState(1000 * (1 + sorted(SETTINGS).index(setting)) + NAMES.index(name))
    im = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    im.setflags(write=False)
    return im


def out_size(h, w, size, max_size, half_up=False):
    """get_size_with_aspect_ratio (detr/datasets/transforms_clip.py:142-161) restated; max_size 0: None -> (oh, ow)"""
    if max_size:
        mn, mx = float(min(w, h)), float(max(w, h))
        if mx / mn * size > max_size:
            v = max_size * mn / mx
            size = int(np.floor(v + 0.5)) if half_up else int(round(v))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def imagenet_planes(u8):
    """ToTensor + Normalize with the ImageNet constants: uint8 [h, w, 3] -> float32 [3, h, w]"""
    m, sd = np.asarray(po.IMAGENET_MEAN, np.float32), np.asarray(po.IMAGENET_STD, np.float32)
    return np.ascontiguousarray(((u8.astype(np.float32) / np.float32(255.0) - m) / sd).transpose(2, 0, 1))


def oracle_views(img, size, max_size, clip_px):
    """-> dict(size (oh, ow), u8 [oh, ow, 3], planes fp32 [3, oh, ow], clip_u8 [n, n, 3], clip fp32 [3, n, n]) of one image"""
    oh, ow = out_size(img.shape[0], img.shape[1], size, max_size)
    u8 = np.ascontiguousarray(po.resize_bicubic(img, ow, oh))
    out = {"size": (oh, ow), "u8": u8, "planes": imagenet_planes(u8)}
    if clip_px:
        out["clip_u8"] = np.ascontiguousarray(po.resize_bicubic(u8, clip_px, clip_px))
        out["clip"] = imagenet_planes(out["clip_u8"])
    return out


@functools.lru_cache(maxsize=None)
def expected(setting, name):
    out = oracle_views(image(setting, name), *SETTINGS[setting])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def full_image(i):
    h, w = FULL_SHAPES[i]
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 120 * np.sin(xx / 7.0 + c) * np.cos(yy / 11.0 - c) for c in range(3)], -1)
    return np.clip(base + np.random.RandomState(77 + i).randint(-40, 40, size=(h, w, 3)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def expected_full(i):
    return oracle_views(full_image(i), *FULL)


def _calls():
    out = []
    for order in (NAMES, NAMES[::-1]):
        at, k = 0, 0
        while at < len(order):
            n = (1, 3, 7)[k % 3]
            out.append(tuple(order[at:at + n]))
            at, k = at + n, k + 1
    return out


CALLS = _calls()      # the same grouping at both settings


def batch_expected(items, hmax=None, wmax=None):
    """nested_tensor_from_tensor_list (detr/util/misc.py:307-329) of the oracle's views: items a list of oracle_views dicts ->
    (tensors fp32 [B, 3, hmax, wmax], mask uint8 [B, hmax, wmax])"""
    hm = max(e["size"][0] for e in items) if hmax is None else hmax
    wm = max(e["size"][1] for e in items) if wmax is None else wmax
    t = np.zeros((len(items), 3, hm, wm), np.float32)
    m = np.ones((len(items), hm, wm), np.uint8)
    for i, e in enumerate(items):
        oh, ow = e["size"]
        t[i, :, :oh, :ow] = e["planes"]
        m[i, :oh, :ow] = 0
    return t, m
