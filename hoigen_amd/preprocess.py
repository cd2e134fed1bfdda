"""Device-side crop pre-processing in front of ``encode_image``.

Counterpart of the reference's PIL pipeline
    ``image.crop(box)``                               pre_images/crop_images.py:204-219
    ``expand2square(crop, background)`` (optional)    utils_tip_cache_and_union_finetune.py:201-212
    ``_transform(n_px)`` = Resize(BICUBIC) / CenterCrop / ToTensor / Normalize    clipnet/clip.py:75-82
for all boxes of one image in three kernel launches (``hg_preprocess_crops``), producing the fp32
``[n, 3, n_px, n_px]`` batch ``encode_image`` consumes.  The resampling reproduces Pillow's 8-bit
``ImagingResample`` bit for bit: the native side works out the crop geometry on the host, a kernel fills the
fixed-point weight tables (IEEE double, the formulas of Pillow's ``precompute_coeffs`` /
``normalize_coeffs_8bpc``) and two kernels do the integer accumulation.  There is no CPU fallback: CPU tensors
raise ``RuntimeError``.

``CropPreprocessor.batch`` does the same for the crops of a batch of images in one call (``hg_preprocess_batch``, two launches): the
boxes stay in device memory, the geometry is worked out per crop on the device and the intermediate of the separable resize stays in
LDS, so the host neither waits nor copies anything back.  With ``stretch=True, imagenet_norm=True`` and no boxes it is the detector's
CLIP view of every image of a batch (utils_tip_cache_and_union_finetune.py:105-114) - of the images ``RandomResize([800], 1333)`` has
already resized: ``detector_views.DetectorViews`` makes those and this view of them from the raw images in one call.
"""
from typing import Sequence

import numpy as np
import torch

from . import _lib


class CropPreprocessor:
    """``CropPreprocessor(n_px)(image_u8, boxes) -> float32 [n, 3, n_px, n_px]`` on the image's device.

    ``image_u8``: uint8 tensor [H, W, 3] (RGB) on a HIP device; ``boxes``: integer (x0, y0, x1, y1) per crop in
    PIL convention (may leave the image: the outside is 0).  ``pad_square=True`` applies ``expand2square`` with
    ``background`` before the resize.  ``return_u8=True`` also returns the resized uint8 crops [n, n_px, n_px, 3].
    """

    def __init__(self, n_px: int = 224, pad_square: bool = False, background: Sequence[int] = (0, 0, 0),
                 stretch: bool = False, imagenet_norm: bool = False):
        """``stretch``: ``IResize([n_px, n_px])`` of the detector's CLIP view (both sides to n_px, no centre crop;
        detr/datasets/transforms_clip.py:279-288); ``imagenet_norm``: ImageNet mean/std
        (utils_tip_cache_and_union_finetune.py:86-89) instead of CLIP's (clipnet/clip.py:81)."""
        self.n_px, self.pad_square, self.background = int(n_px), bool(pad_square), tuple(background)
        self.flags = (1 if pad_square else 0) | (2 if stretch else 0) | (4 if imagenet_norm else 0)

    def __call__(self, image_u8: torch.Tensor, boxes, return_u8: bool = False):
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 or image_u8.dim() != 3 \
                or image_u8.shape[2] != 3:
            raise TypeError("image must be a uint8 tensor [H, W, 3]")
        if image_u8.device.type != "cuda":
            raise RuntimeError("hoigen_amd: crop pre-processing runs only on a HIP device (there is no CPU fallback)")
        boxes = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes)
        boxes = boxes.reshape(-1, 4)
        n, npx = boxes.shape[0], self.n_px
        dev = image_u8.device
        out = torch.empty(n, 3, npx, npx, dtype=torch.float32, device=dev)
        u8 = torch.empty(n, npx, npx, 3, dtype=torch.uint8, device=dev) if return_u8 else None
        if n:
            if ((boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])).any():
                raise ValueError("empty crop box")
            bx = np.ascontiguousarray(boxes, dtype=np.int32)
            bg = (int(self.background[0]) & 255) | ((int(self.background[1]) & 255) << 8) | \
                 ((int(self.background[2]) & 255) << 16)
            img = image_u8.contiguous()
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            with torch.cuda.device(dev):
                rc = _lib.lib().hg_preprocess_crops(_lib.ctx(idx), img.data_ptr(), img.shape[0], img.shape[1],
                                                    bx.ctypes.data, n, npx, self.flags, bg,
                                                    out.data_ptr(), u8.data_ptr() if return_u8 else None,
                                                    torch.cuda.current_stream().cuda_stream)
            _lib.check(idx, rc, "hg_preprocess_crops")
        return (out, u8) if return_u8 else out

    STATUS_REASONS = ((1, "empty crop box"), (2, "more than 65 resampling taps on an axis (a downscale above 16), or a box coordinate "
                                                 "outside +-2**20"), (4, "image index outside the call"))

    def batch(self, images, boxes=None, return_u8: bool = False, check: bool = True, out=None):
        """The crops of a batch of images in one call (``hg_preprocess_batch``): ``images`` a list of uint8 [H, W, 3] device tensors of
        any sizes, ``boxes`` a list with one [n_b, 4] integer array or tensor (host or device) per image, or ``None`` for the whole
        image, one crop each (with ``stretch=True, imagenet_norm=True`` the detector's CLIP view of the batch).  Returns
        float32 [sum n_b, 3, n_px, n_px] in image order (``return_u8``: and the uint8 crops).  Nothing is copied back from the device
        unless ``check``: then the per-crop status is read in one copy and a refused crop raises ``ValueError``; with ``check=False`` the
        int32 status tensor is returned as the last element (0: done; bit 0 empty box, bit 1 tap limit, bit 2 image index) and a refused
        crop is NaN / 0.  Every crop has the bits of the per-image call.  ``out``: the tensors to write into instead of new ones, a tuple
        ``(planes float32 [n, 3, n_px, n_px], crops uint8 [n, n_px, n_px, 3] or None, status int32 [n])``, contiguous, on the images' device
        (views of larger buffers are fine); they are what is returned."""
        images = list(images)
        for im in images:
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                raise TypeError("every image must be a uint8 tensor [H, W, 3]")
            if im.device.type != "cuda":
                raise RuntimeError("hoigen_amd: crop pre-processing runs only on a HIP device (there is no CPU fallback)")
        if boxes is None:
            boxes = [np.array([[0, 0, im.shape[1], im.shape[0]]], np.int32) for im in images]
        boxes = list(boxes)
        if len(boxes) != len(images):
            raise ValueError("one box array per image")
        if not images:
            raise ValueError("no images")
        dev = images[0].device
        if any(im.device != dev for im in images):
            raise RuntimeError("hoigen_amd: the images of one batch must live on one device")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        npx = self.n_px
        counts, parts = [], []
        for b in boxes:
            if isinstance(b, torch.Tensor):
                b = b.reshape(-1, 4)
                if b.is_floating_point():
                    raise TypeError("boxes must be integers (records.pil_box rounds as PIL does)")
                b = b.to(device=dev, dtype=torch.int32)      # a host tensor is uploaded; a device tensor stays where it is
            else:
                b = np.ascontiguousarray(np.asarray(b).reshape(-1, 4))
                if b.size and b.dtype.kind not in "iu":
                    raise TypeError("boxes must be integers (records.pil_box rounds as PIL does)")
                b = b.astype(np.int32)
            counts.append(int(b.shape[0]))
            parts.append(b)
        n = sum(counts)
        if out is None:
            out = torch.empty(n, 3, npx, npx, dtype=torch.float32, device=dev)
            u8 = torch.empty(n, npx, npx, 3, dtype=torch.uint8, device=dev) if return_u8 else None
            status = torch.zeros(n, dtype=torch.int32, device=dev)
        else:
            out, u8, status = out
            want = [(out, torch.float32, (n, 3, npx, npx)), (status, torch.int32, (n,))] + ([(u8, torch.uint8, (n, npx, npx, 3))] if return_u8 else [])
            for t, dtype, shape in want:
                if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"out: a contiguous {dtype} tensor of shape {shape} on {dev} is needed")
        crop_of = np.repeat(np.arange(len(images)), counts)            # image of every crop
        if n:
            host = [p for p in parts if not isinstance(p, torch.Tensor)]
            if len(host) == len(parts):      # one upload for the whole batch
                bx = torch.from_numpy(np.concatenate(parts, axis=0)).to(dev)
            else:
                bx = torch.cat([p if isinstance(p, torch.Tensor) else torch.from_numpy(p).to(dev) for p in parts], dim=0).contiguous()
            bg = (int(self.background[0]) & 255) | ((int(self.background[1]) & 255) << 8) | ((int(self.background[2]) & 255) << 16)
            keep = [im.contiguous() for im in images]
            start = np.concatenate([[0], np.cumsum(counts)])
            lib, handle = _lib.lib(), _lib.ctx(idx)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream().cuda_stream
                # calls of at most 64 images and 4096 crops, each writing its slice of the one output
                i0 = 0
                while i0 < len(keep):
                    i1 = i0 + 1
                    while i1 < len(keep) and i1 - i0 < _lib.HG_PRE_MAX_IMAGES and start[i1 + 1] - start[i0] <= _lib.HG_PRE_MAX_N:
                        i1 += 1
                    B = i1 - i0
                    ptrs = (_lib.C.c_void_p * B)(*[im.data_ptr() for im in keep[i0:i1]])
                    hs = (_lib.C.c_int32 * B)(*[im.shape[0] for im in keep[i0:i1]])
                    ws = (_lib.C.c_int32 * B)(*[im.shape[1] for im in keep[i0:i1]])
                    local = torch.from_numpy((crop_of[start[i0]:start[i1]] - i0).astype(np.int32)).to(dev)
                    for c0 in range(int(start[i0]), int(start[i1]), _lib.HG_PRE_MAX_N):      # (one image with more than 4096 boxes)
                        c1 = min(c0 + _lib.HG_PRE_MAX_N, int(start[i1]))
                        a = _lib.hg_preprocess_batch_args(
                            ptrs, hs, ws, B, bx[c0:c1].data_ptr(), local[c0 - int(start[i0]):].data_ptr(), c1 - c0, npx, self.flags, bg,
                            out[c0:c1].data_ptr(), u8[c0:c1].data_ptr() if return_u8 else None, status[c0:c1].data_ptr())
                        _lib.check(idx, lib.hg_preprocess_batch(handle, _lib.C.byref(a), stream), "hg_preprocess_batch")
                    i0 = i1
            if check:
                st = status.cpu().numpy()
                bad = np.nonzero(st)[0]
                if bad.size:
                    i = int(bad[0])
                    why = "; ".join(r for bit, r in self.STATUS_REASONS if st[i] & bit)
                    raise ValueError(f"{why}: crop {i} (box {i - int(start[crop_of[i]])} of image {int(crop_of[i])}); "
                                     f"{bad.size} of {n} crops refused")
        res = (out, u8) if return_u8 else (out,)
        if not check:
            res = res + (status,)
        return res[0] if len(res) == 1 else res
