"""hg_hoi_detections through the C ABI (and the façade of hoigen_amd.evaluation), held to tests/detections_bound.py:

  rule 1   det_off, the seven entry arrays, det_label, det_gt, every fp32 word of det_max_iou and of the recovered ground-truth boxes and
           the status bit for bit against the fp32 restatement
  rule 3   labels and det_gt equal the float64 definition's, but for the images the screen sets aside (at most 5 % of a family:
           tests/test_detections_model.py holds the families to that)
  NaN-pattern canaries in front of and behind every output and in the unwritten tail beyond det_off[B]; the constructed images; a B-image
  call == B one-image calls; compaction only; cap one short; every limit refused; HOIDetections == HOIHead.postprocess on a real HOIHead
  call; HOIEvaluator over three batches == the host restatement.

Shapes (detections_bound.FAMILIES): NC = 1, 24, 63, 64, 65, 117, 600; pairs an image 0, 1, 2, 63, 64, 65 and 2 016 ragged in one call; B = 1,
3, 8, 64; ground-truth pairs an image 0, 1, 2, 63, 64, 65, 256; both gt_formats; with and without conversion; b64_scan's 2 016 workgroup sums
cross det_scan_kernel's 256-sum block boundary seven times.  File total on an MI355X: a few seconds, most of it the restatement on the CPU."""
import functools

import numpy as np
import pytest
import torch

import detections_bound as db
from hoigen_amd import _lib, evaluation, interaction
from hoigen_amd.cache_model import CacheLogits

pytestmark = pytest.mark.gpu
CANARY = 0x7FC0DEAD
PAD = 64
DEV = "cuda:0"
OUT_KEYS = dict(det_pair="pair", det_verb="verb", det_h="h", det_o="o", det_object="object", det_score="score", det_interaction="interaction",
                det_label="label", det_gt="gt", det_max_iou="max_iou")
FLOATS = ("score", "label", "max_iou")
ASSOC = ("det_label", "det_gt", "det_max_iou", "gt_boxes_out")


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

    def numpy(self):
        return self.buf[PAD:PAD + self.n].cpu().numpy().view(self.dtype)

    def untouched(self):
        return bool((self.numpy().view(np.uint32) == CANARY).all())


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).to(DEV)


def call(case, cap=None, assoc=True, omit=(), B=None, **override):
    """one hg_hoi_detections call -> (rc, the outputs as detections_bound.restate names them, canaries intact, Out objects)"""
    B = case["B"] if B is None else B
    Pt, NC, Gt = int(case["pair_off"][-1]), case["NC"], int(case["gt_off"][-1])
    total = int(db.compact(case)["det_off"][-1])
    cap = total + 7 if cap is None else cap
    keep = [dev(case["prior"]), dev(case["scores"]), dev(case["pair_h"], np.int32), dev(case["pair_o"], np.int32), dev(case["objects"], np.int32),
            dev(case["boxes"]), dev(case["gt_h"]), dev(case["gt_o"]), dev(case["gt_hoi"], np.int32)]
    conv = dev(case["conversion"], np.int32) if case.get("conversion") is not None else None
    o = {k: Out(cap, np.float32 if v in FLOATS else np.int32) for k, v in OUT_KEYS.items()}
    o.update(det_off=Out(B + 1, np.int32), gt_boxes_out=Out(8 * Gt, np.float32), status=Out(B, np.int32))
    a = _lib.hg_hoi_detections_args()
    a.prior, a.scores, a.pair_h, a.pair_o, a.objects, a.boxes, a.gt_boxes_h, a.gt_boxes_o, a.gt_hoi = (t.data_ptr() for t in keep)
    I32 = _lib.C.c_int32
    pair_c, box_c = (I32 * (B + 1))(*[int(v) for v in case["pair_off"][:B + 1]]), (I32 * (B + 1))(*[int(v) for v in case["box_off"][:B + 1]])
    gt_c, size_c = (I32 * (B + 1))(*[int(v) for v in case["gt_off"][:B + 1]]), (I32 * max(2 * B, 1))(*[int(v) for v in case["gt_sizes"].reshape(-1)[:2 * B]])
    a.pair_off, a.box_off, a.B, a.num_classes = pair_c, box_c, B, NC
    if conv is not None:
        a.conversion, a.n_obj_classes = conv.data_ptr(), conv.shape[0]
    if assoc:
        a.gt_off, a.gt_sizes = gt_c, size_c
    a.gt_format, a.min_iou, a.cap = case["gt_format"], case["min_iou"], cap
    for k, v in o.items():
        if k not in omit and (assoc or k not in ASSOC):
            setattr(a, k, v.ptr)
    for k, v in override.items():
        setattr(a, k, v)
    rc = _lib.lib().hg_hoi_detections(_lib.ctx(0), _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = all(v.pads_intact() for v in o.values())
    if rc:
        return rc, None, intact, o
    det_off = o["det_off"].numpy()
    n = min(int(det_off[-1]), cap)
    got = dict(det_off=det_off, status=o["status"].numpy())
    for k, v in OUT_KEYS.items():
        full = o[k].numpy()
        got[v] = full[:n]
        if k not in omit and (assoc or k not in ASSOC):
            intact &= bool((full[n:].view(np.uint32) == CANARY).all())      # the unwritten tail beyond det_off[B]
    got["gt_boxes"] = o["gt_boxes_out"].numpy().reshape(2, Gt, 4)
    return rc, got, intact, o


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, restatement, float64 definition).  Cached: leave unchanged."""
    case = db.constructed()[0] if name == "constructed" else db.family(name)
    return case, db.restate(case), db.definition(case)


@pytest.mark.parametrize("name", tuple(db.FAMILIES) + ("constructed",))
def test_family(name):
    case, exp, defn = expected(name)
    rc, got, intact, _ = call(case)
    assert rc == 0 and intact
    skip = range(case["B"]) if name == "constructed" else ()      # (built ON the thresholds: held to the known answers below)
    n_screened = db.judge(got, case, exp, defn, skip_rule3=skip)
    print(f"DET_SCREENED {name} {n_screened} of {case['B']}")
    if name == "constructed":
        _, index, known = db.constructed()
        db.check_known(got, case, index, known)


def one_image(case, b):
    """image b of a case as a case of its own"""
    p0, p1, b0, b1, g0, g1 = (int(case[k][b + i]) for k in ("pair_off", "box_off", "gt_off") for i in (0, 1))
    out = dict(case, B=1, pair_off=np.asarray([0, p1 - p0], np.int32), box_off=np.asarray([0, b1 - b0], np.int32), gt_off=np.asarray([0, g1 - g0], np.int32),
               prior=case["prior"][:, p0:p1], scores=case["scores"][p0:p1], pair_h=case["pair_h"][p0:p1], pair_o=case["pair_o"][p0:p1],
               objects=case["objects"][p0:p1], boxes=case["boxes"][b0:b1], gt_h=case["gt_h"][g0:g1], gt_o=case["gt_o"][g0:g1],
               gt_hoi=case["gt_hoi"][g0:g1], gt_sizes=case["gt_sizes"][b:b + 1])
    return out


def test_batch_equals_single_images():
    case, exp, _ = expected("b8_nc117_conv")
    for b in range(case["B"]):
        rc, got, intact, _ = call(one_image(case, b))
        assert rc == 0 and intact
        lo, hi = exp["det_off"][b], exp["det_off"][b + 1]
        assert list(got["det_off"]) == [0, hi - lo] and got["status"][0] == exp["status"][b]
        for k in OUT_KEYS.values():
            assert db.same_bits(got[k], exp[k][lo:hi]), (b, k)
        g0, g1 = case["gt_off"][b], case["gt_off"][b + 1]
        assert db.same_bits(got["gt_boxes"], exp["gt_boxes"][:, g0:g1])


def test_compaction_only_leaves_the_association_outputs_untouched():
    case, exp, _ = expected("b3_nc24_conv")
    rc, got, intact, o = call(case, assoc=False)
    assert rc == 0 and intact
    db.judge(got, dict(case, gt_off=None), {k: exp[k] for k in ("det_off", "status", "score") + db.ENTRY_INT})
    assert all(o[k].untouched() for k in ASSOC)
    # the association outputs without ground truth are refused
    rc, _, intact, o = call(case, assoc=False, det_label=o["det_label"].ptr)
    assert rc == -1 and intact and b"gt_off" in _lib.lib().hg_last_error(_lib.ctx(0))


def test_every_output_but_det_off_may_be_left_out():
    case, exp, _ = expected("b3_nc65")
    omit = ("det_pair", "det_h", "det_o", "det_score", "det_interaction", "det_gt", "det_max_iou", "gt_boxes_out", "det_object")
    rc, got, intact, o = call(case, omit=omit)
    assert rc == 0 and intact and all(o[k].untouched() for k in omit)
    assert np.array_equal(got["det_off"], exp["det_off"]) and db.same_bits(got["label"], exp["label"]) and np.array_equal(got["verb"], exp["verb"])
    rc, _, intact, _ = call(case, omit=("det_off",))
    assert rc == -1 and intact


def test_cap_one_short():
    """cap one short of image 2's need: bit 2 on that image and those after it, the true counts in det_off, nothing written at or beyond cap,
    the images before it unaffected"""
    case, exp, _ = expected("b8_nc63")
    cap = int(exp["det_off"][3]) - 1
    rc, got, intact, o = call(case, cap=cap)
    assert rc == 0 and intact      # (the pads sit right behind slot cap - 1)
    want = db.apply_cap(exp, cap)
    assert np.array_equal(got["det_off"], exp["det_off"]) and np.array_equal(got["status"], want["status"])
    assert list(got["status"] & 4) == [0, 0, 4, 4, 4, 4, 4, 4]
    lo = int(exp["det_off"][2])
    for k in OUT_KEYS.values():
        assert db.same_bits(got[k][:lo], exp[k][:lo]), k                   # the images before it: everything
    for k in db.ENTRY_INT + ("score", "gt", "max_iou"):
        assert db.same_bits(got[k], want[k]), k                              # the cut image: its entries below cap as they would be


def test_limits_are_refused():
    case, _, _ = expected("b3_nc24_conv")
    I32 = _lib.C.c_int32
    err = lambda: _lib.lib().hg_last_error(_lib.ctx(0))
    B = case["B"]
    big_gt = (I32 * (B + 1))(0, 257, 257, 257)
    bad_off = (I32 * (B + 1))(0, 5, 3, 66)
    wide = (I32 * (B + 1))(0, 1 << 22, 1 << 22, 1 << 22)      # 2^22 pairs x 1024 classes = 2^32 words
    far = (I32 * (B + 1))(0, (1 << 24) + 1, (1 << 24) + 1, (1 << 24) + 1)
    many = (I32 * 66)(*([0] * 66))
    for what, kw, word in (("B", dict(B=65, pair_off=many, box_off=many, gt_off=many), b"images"), ("NC", dict(num_classes=1025), b"num_classes"),
                           ("NC0", dict(num_classes=0), b"num_classes"), ("gt", dict(gt_off=big_gt), b"ground-truth"),
                           ("decreasing", dict(pair_off=bad_off), b"decrease"), ("count", dict(pair_off=wide, num_classes=1024), b"32-bit"),
                           ("pairs", dict(pair_off=far), b"2^24"), ("cap", dict(cap=-1), b"cap"), ("format", dict(gt_format=2), b"gt_format"),
                           ("prior", dict(prior=None), b"prior")):
        rc, _, intact, o = call(case, **kw)
        assert rc == -1 and intact and word in err(), (what, err())
        assert all(v.untouched() for v in o.values()), what
    assert _lib.lib().hg_hoi_detections(_lib.ctx(0), None, None) == -1


# ---- through the façade -------------------------------------------------------------------------------------------------------------------
NC_HEAD, N_OBJ, SIZE = 12, 4, (200, 224)


def head_batch(seed, counts=((5, 2), (1, 1), (7, 3))):
    """a real HOIHead call on `counts` = (boxes, humans) per image -> (head, branch, its outputs, per-image boxes, sizes, obj2target)"""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = len(counts), 64, 14, 14
    feat = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = torch.randn(NC_HEAD, C, generator=g)
    branch = CacheLogits((w / w.norm(dim=1, keepdim=True)).to(DEV))
    obj2target = (torch.rand(N_OBJ, NC_HEAD, generator=g) < 0.4).to(torch.uint8)
    obj2target[0, :3] = 1
    sizes = torch.tensor([[float(SIZE[0]), float(SIZE[1])]] * B)
    props = []
    for n, n_h in counts:
        xy = torch.rand(n, 2, generator=g) * 120
        wh = 20 + torch.rand(n, 2, generator=g) * 60
        labels = torch.cat([torch.zeros(n_h, dtype=torch.int64), torch.randint(1, N_OBJ, (n - n_h,), generator=g)])
        props.append(dict(boxes=torch.cat([xy, xy + wh], 1).to(DEV), scores=(0.2 + 0.8 * torch.rand(n, generator=g)).to(DEV), labels=labels.to(DEV)))
    head = interaction.HOIHead([("union", branch, 1.0)], obj2target, 0, NC_HEAD)
    out = head(None, feat, sizes, props)
    return head, branch, out, [p["boxes"] for p in props], sizes, obj2target


def case_of(out, boxes, targets, conversion=None):
    """the head's outputs and the targets as a detections_bound case (host copies)"""
    logits, prior, bh, bo, objects = out
    cat = lambda ts, dt: torch.cat([t.reshape(-1) for t in ts]).cpu().numpy().astype(dt)      # noqa: E731
    off = lambda ns: np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)                       # noqa: E731
    return dict(B=len(logits), NC=NC_HEAD, pair_off=off([p.shape[1] for p in prior]), box_off=off([len(b) for b in boxes]),
                gt_off=off([len(t["hoi"]) for t in targets]), prior=torch.cat(list(prior), 1).cpu().numpy(),
                scores=torch.cat([lg.hg_dense_scores for lg in logits]).cpu().numpy(), pair_h=cat(bh, np.int32), pair_o=cat(bo, np.int32),
                objects=cat(objects, np.int32), boxes=torch.cat(boxes).cpu().numpy(), conversion=conversion,
                gt_h=torch.cat([t["boxes_h"] for t in targets]).numpy(), gt_o=torch.cat([t["boxes_o"] for t in targets]).numpy(),
                gt_hoi=torch.cat([t["hoi"] for t in targets]).numpy().astype(np.int32),
                gt_sizes=np.asarray([[int(v) for v in t["size"]] for t in targets], np.int32), gt_format=1, min_iou=0.5)


def targets_of(out, boxes, seed):
    """per image, ground truth = the boxes of some of its pairs plus jitter, with a verb the pair's object admits; normalised cx, cy, w, h"""
    r = np.random.RandomState(seed)
    _, prior, bh, bo, _ = out
    h, w = SIZE
    targets = []
    for pr, x, y, bx in zip(prior, bh, bo, boxes):
        rows, cols = np.nonzero((pr[0] * pr[1]).cpu().numpy())
        G = min(4, len(rows))
        pick = r.randint(0, max(len(rows), 1), G)
        bx = bx.cpu().numpy().astype(np.float64)
        to_c = lambda g: np.stack([(g[:, 0] + g[:, 2]) / 2 / w, (g[:, 1] + g[:, 3]) / 2 / h, (g[:, 2] - g[:, 0]) / w, (g[:, 3] - g[:, 1]) / h], 1)      # noqa: E731
        g_h = bx[x.cpu().numpy()[rows[pick]]].reshape(G, 4) + r.normal(0, 3, (G, 4))
        g_o = bx[y.cpu().numpy()[rows[pick]]].reshape(G, 4) + r.normal(0, 3, (G, 4))
        targets.append(dict(boxes_h=torch.from_numpy(to_c(g_h).astype(np.float32)), boxes_o=torch.from_numpy(to_c(g_o).astype(np.float32)),
                            hoi=torch.from_numpy(cols[pick].astype(np.int64)), size=torch.tensor([h, w])))
    return targets


@pytest.mark.parametrize("bounded", (True, False))
def test_facade_equals_postprocess(bounded):
    """HOIDetections on a real HOIHead call gives the dicts HOIHead.postprocess gives on that call, every tensor bit for bit"""
    head, branch, out, boxes, sizes, obj2target = head_batch(5)
    try:
        logits, prior, bh, bo, objects = out
        want = head.postprocess(boxes, bh, bo, logits, prior, objects, sizes)
        got = evaluation.HOIDetections(obj2target=obj2target if bounded else None)(out, boxes, image_sizes=sizes)
        assert len(got) == len(want) == 3 and sum(len(d["scores"]) for d in want) > 10 and len(want[1]["scores"]) == 0
        for a, b in zip(got, want):
            assert set(a) == set(b)
            for k in ("boxes", "pairing", "scores", "labels", "objects", "size"):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    finally:
        branch.close()


def test_evaluator_over_three_batches():
    """HOIDetections + HOIEvaluator over three batches == the host restatement of test_hico's association and the meter on the same
    detections"""
    meter, host = evaluation.HOIEvaluator(NC_HEAD, algorithm="11P"), evaluation.HOIEvaluator(NC_HEAD, algorithm="11P")
    n_tp = 0
    for seed in (11, 12, 13):
        head, branch, out, boxes, sizes, obj2target = head_batch(seed)
        try:
            targets = targets_of(out, boxes, seed)
            dets = evaluation.HOIDetections(obj2target=obj2target)(out, boxes, targets)
            exp = db.restate(case_of(out, boxes, targets))
            for b, d in enumerate(dets):
                lo, hi = exp["det_off"][b], exp["det_off"][b + 1]
                assert db.same_bits(d["tp"].cpu().numpy(), exp["label"][lo:hi]) and np.array_equal(d["interactions"].cpu().numpy(), exp["interaction"][lo:hi])
                assert np.array_equal(d["gt"].cpu().numpy(), exp["gt"][lo:hi]) and db.same_bits(d["max_iou"].cpu().numpy(), exp["max_iou"][lo:hi])
                assert torch.equal(d["size"], targets[b]["size"])
            meter.append(dets)
            host.append([dict(scores=torch.from_numpy(exp["score"][lo:hi]), interactions=torch.from_numpy(exp["interaction"][lo:hi]).long(),
                              tp=torch.from_numpy(exp["label"][lo:hi])) for lo, hi in zip(exp["det_off"][:-1], exp["det_off"][1:])])
            n_tp += int(exp["label"].sum())
        finally:
            branch.close()
    ap = meter.eval()
    assert n_tp >= 6 and (ap > 0).any() and np.array_equal(ap, host.eval())


def test_facade_raises_on_a_status_bit():
    head, branch, out, boxes, sizes, obj2target = head_batch(5)
    try:
        conv = torch.full((N_OBJ, NC_HEAD), -1, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="image 0.*no interaction"):
            evaluation.HOIDetections(conversion=conv, obj2target=obj2target)(out, boxes)
        targets = targets_of(out, boxes, 1)
        targets[2]["boxes_h"][0, 0] = float("inf")
        with pytest.raises(RuntimeError, match="image 2.*non-finite"):
            evaluation.HOIDetections(obj2target=obj2target)(out, boxes, targets)
    finally:
        branch.close()
