"""roi_align_kernel (hg_preproc.hip) through roi.roi_align (and hg_roi_align itself where both outputs are asked for at once), held to the
two rules of tests/roi_bound.py on every committed case:

  rule 1   pooled map and mean bit for bit against the fp32 restatement in torchvision's published operation order (hg_preproc.hip is
           compiled with -ffp-contract=off for exactly this) - every box, those on the discontinuities included;
  rule 2   every pooled element and every mean within the derived bound E of the float64 definition, for the boxes the screen keeps;
           the `ints` family as the float64 result rounded once, bit for bit.

Maps 14 x 14, 24 x 24 (the 1024-channel local map of ViT-L/14@336px at spatial scale 1 / 14) and 5 x 9; C 4 .. 1024 on both sides of
the 256-lane channel loop; P 1, 2, 7, 14; 0, 1 and 45 boxes; pooled only, mean only, and both from one launch.  Lines ROI_RATIO carry
the kernel's worst |err| / E; tests/test_roi_model.py proves on the CPU which wrong kernels the rules reject.

File total on an MI355X: about 4 s, half of it the float64 reference of the 24 x 24 x 1024 map on the CPU."""
import numpy as np
import pytest
import torch

import roi_bound as rb
from hoigen_amd import _lib
from hoigen_amd.roi import roi_align

pytestmark = pytest.mark.gpu
CANARY = 0x7FC0DEAD          # a quiet NaN with a payload


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def differing(got, want, what):
    bad = bits(got) != bits(want)
    if not bad.any():
        return None
    i = tuple(np.argwhere(bad)[0].tolist())
    return f"{what}: {int(bad.sum())} of {bad.size} elements are not the restatement's bits; first at {i}: {got[i]!r} for {want[i]!r}"


def both_outputs(feat, boxes, P, scale):
    """one launch with both outputs, each between a canary row in front and behind -> (pooled, mean, canaries intact)"""
    C, H, W = feat.shape
    n = boxes.shape[0]
    dev = feat.device
    pooled = torch.full((n + 2, C * P * P), CANARY, dtype=torch.int32, device=dev)
    mean = torch.full((n + 2, C), CANARY, dtype=torch.int32, device=dev)
    idx = dev.index or 0
    rc = _lib.lib().hg_roi_align(_lib.ctx(idx), feat.data_ptr(), C, H, W, boxes.data_ptr(), n, float(scale), P, pooled[1:].data_ptr(),
                                 mean[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(idx, rc, "hg_roi_align")
    torch.cuda.synchronize()
    intact = all(bool((t[0] == CANARY).all()) and bool((t[n + 1] == CANARY).all()) for t in (pooled, mean))
    return pooled[1:n + 1].view(torch.float32).reshape(n, C, P, P), mean[1:n + 1].view(torch.float32), intact


@pytest.mark.parametrize("name", [c["name"] for c in rb.CASES])
def test_both_rules(name):
    c = rb.BY_NAME[name]
    dev = torch.device("cuda:0")
    feat = torch.from_numpy(rb.feat_of(c)).to(dev)
    boxes = torch.from_numpy(c["boxes"]).to(dev)
    P, scale = c["P"], c["scale"]
    want_p, want_m = rb.expected(name)
    pooled = roi_align(feat, boxes, P, float(scale)).cpu().numpy()
    mean = roi_align(feat.unsqueeze(0), boxes, (P, P), float(scale), aligned=True, reduce_mean=True).cpu().numpy()
    p2, m2, intact = both_outputs(feat, boxes, P, scale)
    failures = [f for f in (differing(pooled, want_p, "pooled only"), differing(mean, want_m, "mean only"),
                            differing(p2.cpu().numpy(), want_p, "both: pooled"), differing(m2.cpu().numpy(), want_m, "both: mean")) if f]
    if not intact:
        failures.append("a row in front of or behind an output was written")
    if c["rule2"]:
        ref = rb.reference(name)
        r = rb.ratios(ref, pooled, mean)
        print(f"\nROI_RATIO {name} kernel: pooled {r['pooled']:.3f} mean {r['mean']:.3f} ({int(ref['kept'].sum())} of {len(c['boxes'])} boxes kept)")
        if not (r["pooled"] <= 1.0 and r["mean"] <= 1.0):
            failures.append(f"float64 rule: worst |err| / E pooled {r['pooled']:.3f} mean {r['mean']:.3f}")
        if c["family"] == "ints":
            if not (np.array_equal(pooled, ref["pooled"].astype(np.float32)) and np.array_equal(mean, ref["mean"].astype(np.float32))):
                failures.append("the exact family is not the float64 result rounded once")
    assert not failures, failures


def test_no_boxes():
    dev = torch.device("cuda:0")
    feat = torch.from_numpy(rb.make_map("randn", 257, 14, 14)).to(dev)
    none = torch.zeros(0, 4, device=dev)
    assert roi_align(feat, none, 7, 1 / 16).shape == (0, 257, 7, 7)
    assert roi_align(feat, none, 7, 1 / 16, reduce_mean=True).shape == (0, 257)
    p, m, intact = both_outputs(feat, none, 7, rb.SCALES["1/16"])
    assert p.shape == (0, 257, 7, 7) and m.shape == (0, 257) and intact
