"""hg_load_priors / hg_region_priors through the C ABI (and the façade of hoigen_amd.proposals once), held to tests/props_bound.py:

  rule 1   counts, keep, the survivor lists, the gathered boxes / scores / labels, the mask, every fp32 word of T and of the priors
           (pad rows included) bit for bit against the fp32 restatement
  rule 2   the priors within the derived bound of the float64 definition
  rule 3   the integer outputs equal the float64 definition's, but for the images the screen sets aside (at most 5 % of a family:
           tests/test_props_model.py holds the families to that)
  NaN-pattern canaries in front of and behind every output, and in the unwritten tail of every survivor list; a B-image call == B
  one-image calls; update() visible in the next call; a non-finite image confined to itself; every refusal; HOIHead fed from the
  façade's lists == HOIHead fed from plain lists.

Shapes (props_bound.FAMILIES): Q = 0, 1, 2, 63, 64, 65, 100, 128, 129, 512 ragged in one call; B = 1, 3, 8, 10, 64; 2, 3 and 81 classes;
E = 512 and 768; hidden 96, 128 and 256; cap 8, 30 and 64 rows (1, 2 and 4 row groups).  Lines PROPS_RATIO carry the worst |err| / E.
File total on an MI355X: a few seconds, most of it the restatement on the CPU."""
import functools

import numpy as np
import pytest
import torch

import props_bound as pb
from hoigen_amd import _lib, interaction, proposals
from hoigen_amd.cache_model import CacheLogits

pytestmark = pytest.mark.gpu
CANARY = 0x7FC0DEAD
PAD = 64      # canary words on either side of an output (a multiple of 4: out_boxes stays 16-byte aligned)
DEV = "cuda:0"


def state_dict(wt, dev=DEV):
    t = lambda k: torch.from_numpy(wt[k]).to(dev)
    return {"layers.0.weight": t("w0"), "layers.0.bias": t("b0"), "layers.1.weight": t("w1"), "layers.1.bias": t("b1"),
            "layers.2.weight": t("w2"), "layers.2.bias": t("b2")}, t("emb")


def load(wt):
    return proposals.InstancePriors(*state_dict(wt))


class Out:
    """an output buffer between two canary pads"""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def pads_intact(self):
        h = self.buf.cpu().numpy()
        return bool((h[:PAD] == CANARY).all() and (h[PAD + self.n:] == CANARY).all())

    def numpy(self, shape):
        return self.buf[PAD:PAD + self.n].cpu().numpy().view(self.dtype).reshape(shape)


def call(case, slot, own_buffers=True, **override):
    """one hg_region_priors call -> (rc, outputs as numpy like props_bound.restate's, canaries intact); own_buffers = False leaves
    keep and the gathered boxes / scores / labels to the library's workspace (their buffers here must come back untouched)"""
    p, B, Qt = dict(case["params"], **override), case["B"], int(case["q_off"][-1])
    cap = 2 * p["max_instances"]
    scores = torch.from_numpy(case["scores"]).to(DEV)
    labels = torch.from_numpy(case["labels"].astype(np.int32)).to(DEV)
    boxes = torch.from_numpy(case["boxes"]).to(DEV).contiguous()
    hid = case["weights"]["w0"].shape[0]
    ncls = case["weights"]["emb"].shape[0]
    want = slot >= 0
    o = dict(counts=Out(4 * B, np.int32), keep=Out(B * cap, np.int32), boxes=Out(4 * B * cap, np.float32), scores=Out(B * cap, np.float32),
             labels=Out(B * cap, np.int32), survivors=Out(Qt, np.int32), priors=Out(B * cap * pb.OUT, np.float32),
             mask=Out((B * cap + 3) // 4, np.uint8), table=Out(ncls * hid, np.float32))
    a = _lib.hg_region_priors_args()
    a.scores, a.labels, a.boxes = scores.data_ptr(), labels.data_ptr(), boxes.data_ptr()
    off_c = (_lib.C.c_int32 * (B + 1))(*[int(v) for v in case["q_off"]])
    size_c = (_lib.C.c_float * max(2 * B, 1))(*[float(v) for v in case["image_sizes"].reshape(-1)])
    a.q_off, a.image_sizes, a.B = off_c, size_c, B
    a.box_score_thresh, a.nms_thresh = p["box_score_thresh"], p["nms_thresh"]
    a.human_idx, a.min_instances, a.max_instances, a.prior_slot = p["human_idx"], p["min_instances"], p["max_instances"], slot
    a.counts = o["counts"].ptr
    if own_buffers:
        a.keep, a.out_boxes, a.out_scores, a.out_labels = o["keep"].ptr, o["boxes"].ptr, o["scores"].ptr, o["labels"].ptr
    a.survivors = o["survivors"].ptr
    if want:
        a.priors, a.mask, a.table_out = o["priors"].ptr, o["mask"].ptr, o["table"].ptr
    rc = _lib.lib().hg_region_priors(_lib.ctx(0), _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc:
        return rc, None, all(v.pads_intact() for v in o.values())
    counts = o["counts"].numpy((B, 4))
    surv_all = o["survivors"].numpy((Qt,))
    survivors, tails = [], True
    for b in range(B):
        lo, hi = int(case["q_off"][b]), int(case["q_off"][b + 1])
        survivors.append(surv_all[lo:lo + counts[b, 3]].copy())
        tails &= bool((surv_all[lo + counts[b, 3]:hi].view(np.uint32) == CANARY).all())
    got = dict(counts=counts, keep=o["keep"].numpy((B, cap)), boxes=o["boxes"].numpy((B, cap, 4)), scores=o["scores"].numpy((B, cap)),
               labels=o["labels"].numpy((B, cap)), survivors=survivors)
    if want:
        got.update(priors=o["priors"].numpy((B, cap, pb.OUT)), mask=o["mask"].numpy((-1,))[:B * cap].reshape(B, cap),
                   table=o["table"].numpy((ncls, hid)))
    return rc, got, tails and all(o[k].pads_intact() for k in o) and all(want or (o[k].numpy((-1,)).view(np.uint32) == CANARY).all()
                                                                           for k in ("priors", "table"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, restatement, float64 definition).  Cached: leave unchanged."""
    case = pb.constructed()[0] if name == "constructed" else pb.family(name)
    return case, pb.restate(case), pb.definition(case)


@pytest.mark.parametrize("name", tuple(pb.FAMILIES) + ("constructed",))
def test_family(name):
    case, exp, defn = expected(name)
    pri = load(case["weights"])
    try:
        rc, got, intact = call(case, pri.slot)
    finally:
        pri.close()
    assert rc == 0 and intact
    skip = range(case["B"]) if name == "constructed" else ()      # (built ON the thresholds: held to the known answers below)
    worst = pb.judge(got, case, exp, defn, skip_rule3=skip)
    print(f"PROPS_RATIO {name} {worst:.3f}")
    if name == "constructed":
        _, index, known = pb.constructed()
        for n, keep in known.items():
            b = index[n]
            assert list(got["keep"][b][:got["counts"][b][0]]) == keep, n


def test_selected_instances_in_the_workspace():
    """keep / out_boxes / out_scores / out_labels NULL: the priors are the same bits, the caller's buffers stay untouched, and one of
    the four alone is refused"""
    case, exp, _ = expected("b3_ragged_2cls")
    pri = load(case["weights"])
    try:
        rc, got, intact = call(case, pri.slot, own_buffers=False)
        assert rc == 0 and intact
        assert np.array_equal(got["counts"], exp["counts"]) and same_bits(got["priors"], exp["priors"]) and np.array_equal(got["mask"], exp["mask"])
        for k in ("keep", "labels", "boxes", "scores"):
            assert (got[k].view(np.uint32) == CANARY).all(), k
        a = _lib.hg_region_priors_args()
        a.B, a.max_instances, a.min_instances, a.prior_slot = 1, 15, 3, -1
        off_c = (_lib.C.c_int32 * 2)(0, 0)
        buf = torch.zeros(64, dtype=torch.int32, device=DEV)
        a.q_off, a.counts, a.keep = off_c, buf.data_ptr(), buf.data_ptr()
        assert _lib.lib().hg_region_priors(_lib.ctx(0), _lib.C.byref(a), None) == -1
        assert b"together" in _lib.lib().hg_last_error(_lib.ctx(0))
    finally:
        pri.close()


def test_proposals_only():
    case, exp, _ = expected("b3_ragged_2cls")
    rc, got, intact = call(case, -1)
    assert rc == 0 and intact
    for k in ("counts", "keep", "labels"):
        assert np.array_equal(got[k], exp[k]), k
    for k in ("boxes", "scores"):
        assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), k


@pytest.mark.parametrize("name", ("q_edges_81", "b3_ragged_2cls", "cap64_hid256"))
def test_batch_equals_images_one_by_one(name):
    case, exp, _ = expected(name)
    pri = load(case["weights"])
    try:
        rc, whole, intact = call(case, pri.slot)
        assert rc == 0 and intact
        for b in range(case["B"]):
            rc, one, intact = call(pb.case_images(case, [b]), pri.slot)
            assert rc == 0 and intact
            for k in ("counts", "keep", "labels", "mask"):
                assert np.array_equal(one[k][0], whole[k][b]), (k, b)
            for k in ("boxes", "scores", "priors"):
                assert np.array_equal(one[k][0].view(np.uint32), whole[k][b].view(np.uint32)), (k, b)
            assert np.array_equal(one["survivors"][0], whole["survivors"][b])
    finally:
        pri.close()


def test_update_is_visible_in_the_next_call():
    case, exp, _ = expected("b3_ragged_2cls")
    other = dict(case, weights=pb.make_weights(512, 96, 2, seed=99))
    pri = load(case["weights"])
    try:
        rc, got, _ = call(case, pri.slot)
        assert rc == 0 and np.array_equal(got["priors"].view(np.uint32), exp["priors"].view(np.uint32))
        pri.update(*state_dict(other["weights"]))
        rc, got, intact = call(other, pri.slot)
        exp2 = pb.restate(other)
        assert rc == 0 and intact
        assert np.array_equal(got["table"].view(np.uint32), exp2["table"].view(np.uint32))
        assert np.array_equal(got["priors"].view(np.uint32), exp2["priors"].view(np.uint32))
        assert not np.array_equal(got["priors"], exp["priors"])
    finally:
        pri.close()


def test_non_finite_image_is_confined():
    case, exp, _ = expected("b3_ragged_2cls")
    bad = dict(case, scores=case["scores"].copy(), boxes=case["boxes"].copy())
    bad["scores"][case["q_off"][1] + 2] = np.nan            # image 1
    pri = load(case["weights"])
    try:
        rc, got, intact = call(bad, pri.slot)
        assert rc == 0 and intact
        assert tuple(got["counts"][1]) == (0, 0, 1, 0)
        assert (got["keep"][1] == -1).all() and (got["labels"][1] == -1).all() and not got["boxes"][1].any() and got["mask"][1].all()
        none = np.zeros(0, np.int64)                        # a pad row of this slot: the MLP of a zero row
        pad = pb.prior_rows(none.astype(np.float32), np.zeros((0, 4), np.float32), none, 1, 1, 1, case["weights"], exp["table"])[0][0]
        assert np.array_equal(got["priors"][1].view(np.uint32), np.broadcast_to(pad, got["priors"][1].shape).view(np.uint32))
        for b in (0, 2):
            for k in ("counts", "keep", "labels", "mask", "boxes", "scores", "priors"):
                assert same_bits(got[k][b], exp[k][b]), (k, b)
        bad["scores"] = case["scores"]
        bad["boxes"][case["q_off"][2] + 1, 3] = np.inf      # image 2, a coordinate
        rc, got, intact = call(bad, pri.slot)
        assert rc == 0 and intact and [int(s) for s in got["counts"][:, 2]] == [0, 0, 1]
        assert np.array_equal(got["priors"][0].view(np.uint32), exp["priors"][0].view(np.uint32))
        # the façade names the image
        front = proposals.DetectorFrontEnd(proposals.RegionProposals(**case["params"]), pri)
        with pytest.raises(RuntimeError, match="image 2 .*non-finite"):
            front(results_of(bad), bad["image_sizes"])
        # a label outside the embedding table: status bit 1, confined the same way
        lab = dict(case, labels=case["labels"].copy())
        lab["labels"][0] = 2
        rc, got, intact = call(lab, pri.slot)
        assert rc == 0 and intact and [int(s) for s in got["counts"][:, 2]] == [2, 0, 0] and got["counts"][0, 0] == 0
        assert np.array_equal(got["keep"][1:], exp["keep"][1:])
    finally:
        pri.close()


def test_refusals():
    case, _, _ = expected("b3_ragged_2cls")
    lib, ctx = _lib.lib(), _lib.ctx(0)
    pri = load(case["weights"])
    try:
        one = pb.case_images(case, [0])
        im = lambda q: (np.full(q, 0.5, np.float32), np.zeros(q, np.int64), np.tile(np.array([[0, 0, 1, 1]], np.float32), (q, 1)))
        assert call(one, pri.slot, max_instances=33)[0] == -1
        assert b"max_instances" in lib.hg_last_error(ctx)
        assert call(one, pri.slot, max_instances=32)[0] == 0
        assert call(one, pri.slot, min_instances=16)[0] == -1 and call(one, pri.slot, max_instances=0, min_instances=0)[0] == -1
        big = pb.pack([im(513)], [(10.0, 10.0)], case["params"], case["weights"])
        assert call(big, pri.slot)[0] == -1 and b"513 detections" in lib.hg_last_error(ctx)
        many = pb.pack([im(1)] * 65, [(10.0, 10.0)] * 65, case["params"], case["weights"])
        assert call(many, pri.slot)[0] == -1 and b"65 images" in lib.hg_last_error(ctx)
        assert call(pb.pack([im(1)] * 64, [(10.0, 10.0)] * 64, case["params"], case["weights"]), pri.slot)[0] == 0
        free = next(s for s in range(_lib.HG_MAX_PRIOR_SLOTS) if s != pri.slot)
        assert call(one, free)[0] == -3 and call(one, _lib.HG_MAX_PRIOR_SLOTS)[0] == -1
        # hg_load_priors: each limit, one beyond
        sd, emb = state_dict(case["weights"])
        keep = [sd[f"layers.{i}.{k}"] for i in range(3) for k in ("weight", "bias")] + [emb]
        for field, value in (("E", 1025), ("hidden", 257), ("out", 32), ("out", 128), ("n_obj_classes", 257), ("E", 0)):
            w = _lib.hg_prior_weights()
            w.E, w.hidden, w.out, w.n_obj_classes = 512, 96, 64, 2
            w.w0, w.b0, w.w1, w.b1, w.w2, w.b2, w.object_embedding = (_lib.tensor(t) for t in keep)
            setattr(w, field, value)
            assert lib.hg_load_priors(ctx, free, _lib.C.byref(w)) == -1, (field, value)
        assert lib.hg_load_priors(ctx, _lib.HG_MAX_PRIOR_SLOTS, _lib.C.byref(w)) == -1
        rc, got, intact = call(case, pri.slot)      # the loaded slot is untouched by all that
        assert rc == 0 and intact
    finally:
        pri.close()


def results_of(case, label_dtype=torch.int64):
    out = []
    for b in range(case["B"]):
        lo, hi = case["q_off"][b], case["q_off"][b + 1]
        out.append(dict(scores=torch.from_numpy(case["scores"][lo:hi]).to(DEV), labels=torch.from_numpy(case["labels"][lo:hi]).to(DEV).to(label_dtype),
                        boxes=torch.from_numpy(case["boxes"][lo:hi]).to(DEV)))
    return out


@pytest.mark.parametrize("label_dtype", (torch.int64, torch.int32))
def test_facade(label_dtype):
    case, exp, _ = expected("b3_ragged_2cls")
    pri = load(case["weights"])
    try:
        front = proposals.DetectorFrontEnd(proposals.RegionProposals(**case["params"]), pri)
        region_props, (priors, mask) = front(results_of(case, label_dtype), torch.from_numpy(case["image_sizes"]))
        max_n = int(exp["counts"][:, 0].max())
        assert priors.shape == (case["B"], max_n, 64) and mask.shape == (case["B"], max_n) and mask.dtype == torch.bool
        assert np.array_equal(priors.cpu().numpy().view(np.uint32), exp["priors"][:, :max_n].view(np.uint32))
        assert np.array_equal(mask.cpu().numpy(), exp["mask"][:, :max_n] != 0)
        for b, rp in enumerate(region_props):
            n = exp["counts"][b][0]
            assert rp["labels"].dtype == label_dtype and rp["boxes"].shape == (n, 4) and rp["scores"].shape == (n,)
            assert np.array_equal(rp["labels"].cpu().numpy(), exp["labels"][b][:n]) and rp["n_human"] == exp["counts"][b][1]
            assert np.array_equal(rp["boxes"].cpu().numpy(), exp["boxes"][b][:n]) and np.array_equal(rp["scores"].cpu().numpy(), exp["scores"][b][:n])
            assert np.array_equal(rp["keep"].cpu().numpy(), exp["keep"][b][:n])
        only, none = proposals.DetectorFrontEnd(proposals.RegionProposals(**case["params"]))(results_of(case), case["image_sizes"])
        assert none is None and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(only, region_props))
    finally:
        pri.close()


def test_hoi_head_fed_from_the_front_end_equals_plain_lists():
    case, exp, _ = expected("b3_ragged_2cls")
    B, C, H, W, NC = case["B"], 64, 14, 14, 12
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = torch.randn(NC, C, generator=g)
    branch = CacheLogits((w / w.norm(dim=1, keepdim=True)).to(DEV))
    obj2target = (torch.rand(2, NC, generator=g) < 0.5).to(torch.uint8)
    sizes = torch.full((B, 2), 224.0)
    try:
        head = interaction.HOIHead([("union", branch, 1.0)], obj2target, case["params"]["human_idx"], NC)
        region_props, _ = proposals.DetectorFrontEnd(proposals.RegionProposals(**case["params"]))(results_of(case), sizes)
        boxes = [dict(p, boxes=p["boxes"] * (224.0 / 900.0)) for p in region_props]      # inside the 224-pixel image the map stands for
        plain = [{k: p[k] for k in ("boxes", "scores", "labels")} for p in boxes]
        a = head(None, feat, sizes, boxes)
        b = head(None, feat, sizes, plain)
        assert sum(len(x) for x in a[0]) > 0
        for la, lb in zip(a, b):
            for ta, tb in zip(la, lb):
                assert torch.equal(ta, tb) or (torch.isnan(ta) == torch.isnan(tb)).all() and torch.equal(torch.nan_to_num(ta), torch.nan_to_num(tb))
    finally:
        branch.close()
