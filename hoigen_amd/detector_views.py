"""The detector's two views of a batch from raw images, in one call on the device (``hg_detector_views``).

Counterpart of what the reference's ``DataFactory.__getitem__``, its collate and ``UPT.forward`` do per image on the host
(utils_tip_cache_and_union_finetune.py:109-114, :193-196; upt...:1593, :1613):
    ``RandomResize([800], max_size=1333)``      detr/datasets/transforms_clip.py:139-170 (a Pillow BICUBIC resize)
    ``IResize([n, n])`` of that resized image    transforms_clip.py:279-288
    ``ToTensor`` + ImageNet ``Normalize``, twice utils_tip_cache_and_union_finetune.py:86-89
    ``nested_tensor_from_tensor_list``           detr/util/misc.py:307-329
The decoded uint8 images are uploaded once; the resized bytes, the padded fp32 batch with its mask and the CLIP view come back bit for
bit as Pillow and torch give them, with no host wait and nothing copied back.  The sizes are worked out on the host
(``hg_detector_view_shapes``: pure host code, usable without a device through ``view_shapes``).  There is no CPU fallback: CPU tensors
raise ``RuntimeError``.
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

REASONS = {1: "an output side of 0", 2: "an output side above 2048", 3: "more than 65 resampling taps on an axis (a downscale above 16)",
           4: "a height or width below 1"}


def view_shapes(heights: Sequence[int], widths: Sequence[int], size: int = 800, max_size: int = 1333):
    """``get_size_with_aspect_ratio`` (transforms_clip.py:142-161) of every image, on the host: returns
    ``(sizes [(oh, ow), ...], hmax, wmax, u8_off int64 [B + 1])``; ``max_size`` 0 or ``None`` means none.  Raises ``ValueError`` naming the
    first image the native side refuses."""
    B = len(heights)
    if B != len(widths) or B < 1:
        raise ValueError("one height and one width per image, at least one image")
    C = _lib.C
    hs, ws = (C.c_int32 * B)(*[int(h) for h in heights]), (C.c_int32 * B)(*[int(w) for w in widths])
    out, off = (C.c_int32 * (2 * B))(), (C.c_int64 * (B + 1))()
    hm, wm = C.c_int32(), C.c_int32()
    rc = _lib.lib().hg_detector_view_shapes(hs, ws, B, int(size), int(max_size or 0), out, C.byref(hm), C.byref(wm), off)
    if rc:
        if hm.value < 0:
            raise ValueError(f"size must be 1 .. {_lib.HG_DV_MAX_SIDE} and max_size 0 .. {_lib.HG_DV_MAX_SIDE} (got {size}, {max_size})")
        raise ValueError(f"image {hm.value} ({heights[hm.value]} x {widths[hm.value]}, h x w): {REASONS.get(wm.value, '?')}")
    return [(out[2 * b], out[2 * b + 1]) for b in range(B)], hm.value, wm.value, np.array(off[:], np.int64)


def scale_targets(targets, orig_sizes, sizes):
    """The target side of ``resize`` (transforms_clip.py:175-204), on the host: for target ``t`` of an image of ``orig_sizes[i] = (h, w)``
    resized to ``sizes[i] = (oh, ow)``, ``boxes``, ``boxes_h`` and ``boxes_o`` are multiplied by
    ``as_tensor([rw, rh, rw, rh])`` with ``rw = float(ow) / float(w)``, ``rh = float(oh) / float(h)``, and ``size = tensor([oh, ow])``.
    Returns new dicts; the other entries are passed on as they are."""
    out = []
    for t, (h, w), (oh, ow) in zip(targets, orig_sizes, sizes):
        rw, rh = float(ow) / float(w), float(oh) / float(h)
        t = dict(t)
        for k in ("boxes", "boxes_h", "boxes_o"):
            if k in t:
                t[k] = t[k] * torch.as_tensor([rw, rh, rw, rh])
        t["size"] = torch.tensor([oh, ow])
        out.append(t)
    return out


class DetectorViews:
    """``DetectorViews(size=800, max_size=1333, clip_px=224)(images) -> (tensors, mask, clip, sizes)``.

    ``images``: a list of uint8 [H, W, 3] (RGB) tensors of any sizes on one HIP device.  ``tensors`` float32 [B, 3, hmax, wmax] and
    ``mask`` bool [B, hmax, wmax] (True in the padding) are the ``NestedTensor`` the detector takes; ``clip`` float32
    [B, 3, clip_px, clip_px] is the CLIP view of the resized images (``None`` with ``clip_px=0``); ``sizes`` the list of ``(oh, ow)``.
    ``return_u8=True`` appends the resized images, a list of uint8 [oh, ow, 3] views of one buffer.  More than 64 images run as several
    calls that write slices of the one output."""

    def __init__(self, size: int = 800, max_size: int = 1333, clip_px: int = 224):
        self.size, self.max_size, self.clip_px = int(size), int(max_size or 0), int(clip_px)
        if not 0 <= self.clip_px <= _lib.HG_DV_MAX_CLIP_PX:
            raise ValueError(f"clip_px must be 0 .. {_lib.HG_DV_MAX_CLIP_PX}")

    def __call__(self, images, return_u8: bool = False):
        images = list(images)
        for im in images:
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                raise TypeError("every image must be a uint8 tensor [H, W, 3]")
            if im.device.type != "cuda":
                raise RuntimeError("hoigen_amd: the detector's views are made only on a HIP device (there is no CPU fallback)")
        if not images:
            raise ValueError("no images")
        dev = images[0].device
        if any(im.device != dev for im in images):
            raise RuntimeError("hoigen_amd: the images of one batch must live on one device")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        B, n = len(images), self.clip_px
        sizes, hmax, wmax, off = view_shapes([im.shape[0] for im in images], [im.shape[1] for im in images], self.size, self.max_size)
        tensors = torch.empty(B, 3, hmax, wmax, dtype=torch.float32, device=dev)
        mask = torch.empty(B, hmax, wmax, dtype=torch.uint8, device=dev)
        clip = torch.empty(B, 3, n, n, dtype=torch.float32, device=dev) if n else None
        u8 = torch.empty(int(off[B]), dtype=torch.uint8, device=dev) if return_u8 else None
        keep = [im.contiguous() for im in images]
        lib, handle, C = _lib.lib(), _lib.ctx(idx), _lib.C
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for i0 in range(0, B, _lib.HG_DV_MAX_IMAGES):
                i1 = min(i0 + _lib.HG_DV_MAX_IMAGES, B)
                k = i1 - i0
                a = _lib.hg_detector_views_args(
                    (C.c_void_p * k)(*[im.data_ptr() for im in keep[i0:i1]]), (C.c_int32 * k)(*[im.shape[0] for im in keep[i0:i1]]),
                    (C.c_int32 * k)(*[im.shape[1] for im in keep[i0:i1]]), k, self.size, self.max_size, n, hmax, wmax,
                    u8[int(off[i0]):].data_ptr() if return_u8 else None, tensors[i0:i1].data_ptr(), mask[i0:i1].data_ptr(),
                    clip[i0:i1].data_ptr() if n else None)
                _lib.check(idx, lib.hg_detector_views(handle, C.byref(a), stream), "hg_detector_views")
        res = (tensors, mask.view(torch.bool), clip, sizes)
        if return_u8:
            res += ([u8[int(off[b]):int(off[b]) + oh * ow * 3].view(oh, ow, 3) for b, (oh, ow) in enumerate(sizes)],)
        return res
