"""hg_hoi_head through the C ABI (and once through hoigen_amd.interaction.HOIHead), held to tests/hoi_head_bound.py:

  integer outputs and union boxes       bit for bit against the restatement of the reference's pair enumeration
  pooled means                          bit for bit against the fp32 restatement (rule 1), within E of roi_bound.definition's float64
                                        mean for the boxes the screen keeps (rule 2), within E + roi_bound's bound of hg_roi_align's mean
  feats                                 == hg_l2_normalize of the returned means, bit for bit
  branch_logits                         == hg_cache_logits on the returned feats, bit for bit (this covers the lda = 2C view)
  logits                                == branch_0 scale_0 + branch_1 scale_1 + .. left to right in fp32 on the returned branches
  prior                                 exact at p = 1, within POWF_ULP of float64 pow at p = 2.8; scores within the propagated bound
  NaN of the zero-width box             in the rows of its own pairs and nowhere else
  canary rows in front of and behind every output; a B-image call == B one-image calls; a repeated call == the first; every refusal

Shapes: B = 1, 2, 3 with an image of one box and an image without humans between two normal ones and images of humans only; maps
14 x 14, 24 x 24, 5 x 9, and 26 x 26 and 32 x 32 (channel chunks of 32); C = 4, 40, 96 and 257 (pooling only), 64, 128, 768 (with six
branches: every source), 256 with 552 pairs cut into chunks of 256 rows and through the ring GEMM (test_chunk_seams_and_ring_gemm); RoIs per image 1, 8 and 9 (a
workgroup's eight waves and one more), 64 and 65 (a wave's lanes and one more) and 15 + 15 boxes (435 pairs) once.  Boxes: seeded
uniform draws with a zero-width box, one reaching 2.5 cells beyond the map, the whole image and one smaller than a bin among them;
the boxes on the cuts in a case of their own.  Lines HOI_RATIO carry the kernel's worst |err| / E.

File total on an MI355X: about 20 s, most of it the restatement and the float64 reference on the CPU."""
import functools

import numpy as np
import pytest
import torch

import hoi_head_bound as hb
import roi_bound as rb
from hoigen_amd import _lib, interaction, vae
from hoigen_amd.cache_model import CacheLogits
from hoigen_amd.roi import roi_align

pytestmark = pytest.mark.gpu
CANARY = 0x7FC0DEAD
P = 7
NC, S = 24, 40
SIX = (("human_object", 0.5), ("union", 1.0), ("text", 2.0), ("human", 0.7), ("object", 1.3), ("global", 0.3))
# name: (H, W, C, image size, scale, boxes per image, humans per image, with branches, score power)
CASES = {
    "b3_one_box_between": (14, 14, 64, 224, "1/16", (9, 1, 5), (7, 1, 2), True, 2.8),          # 65 and 13 RoIs
    "b3_no_human_between": (14, 14, 128, 224, "1/16", (8, 6, 3), (8, 0, 3), True, 1.0),        # 64, 6 and 9 RoIs; humans only twice
    "b2_24x24_c768": (24, 24, 768, 336, "1/14", (4, 3), (2, 1), True, 2.8),                    # 12 channel chunks; 10 and 5 RoIs
    "b1_435_pairs": (14, 14, 64, 224, "1/16", (30,), (15,), True, 1.0),
    "b1_5x9_c4": (5, 9, 4, 100, "1/14", (12,), (3,), False, 1.0),
    "b2_c257": (14, 14, 257, 224, "1/16", (6, 2), (2, 1), False, 1.0),                         # 4 chunks of 64 and one channel
    "b3_24x24_c4": (24, 24, 4, 336, "1/14", (8, 1, 2), (0, 0, 2), False, 1.0),                 # 8, 1 and 4 RoIs
    "b1_cuts": (14, 14, 4, 224, "1/16", (5,), (2,), False, 1.0),
    # maps of more than 639 cells: channel chunks of 32, half the lanes idle (hoi_pool_chunk)
    "b1_26x26_c96": (26, 26, 96, 364, "1/14", (6,), (2,), False, 1.0),                         # 3 chunks of 32; 16 RoIs
    "b2_32x32_c40": (32, 32, 40, 448, "1/14", (3, 2), (1, 1), False, 1.0),                     # a chunk of 32 and one of 8; the largest map
}


@functools.lru_cache(maxsize=None)
def batch_of(name):
    H, W, C, size, sk, sizes, humans, _, _ = CASES[name]
    b = hb.make_batch(sizes, humans, H, W, C, size, seed=sum(map(ord, name)), num_classes=NC)
    if name == "b1_cuts":
        b["boxes"] = np.ascontiguousarray(rb.on_the_cuts(14, P, rb.SCALES[sk]))
    b["scale"] = rb.SCALES[sk]
    b["feat_global"] = np.random.RandomState(5).randn(b["B"], C).astype(np.float32)
    b["pairs"] = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    return b


@functools.lru_cache(maxsize=None)
def expected_pool(name):
    """(single [N, C], union [Pt, C]) of the restatement, and the float64 references per image.  Cached: leave unchanged."""
    b = batch_of(name)
    pr, off = b["pairs"], b["box_off"]
    single, union, refs = [], [], []
    for i in range(b["B"]):
        rois = np.concatenate([b["boxes"][off[i]:off[i + 1]], pr["union_boxes"][pr["pair_off"][i]:pr["pair_off"][i + 1]]])
        m = hb.pool(b["feat"][i], rois, P, b["scale"])
        n = off[i + 1] - off[i]
        single.append(m[:n]), union.append(m[n:])
        refs.append(hb.reference(b["feat"][i], rois, P, b["scale"]))
    return np.concatenate(single), np.concatenate(union), refs


def make_branches(C, dev, which=SIX, S=S):
    """one CacheLogits per entry of `which` (the text branch a linear map), seeded"""
    g = torch.Generator().manual_seed(C)
    out = []
    for src, scale in which:
        K = 2 * C if src == "human_object" else C
        w = torch.randn(S if src != "text" else NC, K, generator=g)
        w = (w / w.norm(dim=1, keepdim=True)).to(dev)
        if src == "text":
            out.append(("union", CacheLogits(w), scale))
            continue
        lab = (torch.rand(S, NC, generator=g) < 0.2).float()
        lens = lab.sum(0).clamp_min(1.0)
        out.append((src, CacheLogits(w, -torch.ones(S, device=dev), lab.to(dev), lens.to(dev), 2.0 if src == "human_object" else 1.0), scale))
    return out


def canaried(rows, cols, dev, dtype=torch.float32):
    return torch.full((rows + 2, max(cols, 1)), CANARY, dtype=torch.int32, device=dev)


def call(b, branches, power, images=None, outputs=True, ctx=None, **override):
    """one hg_hoi_head call on the images `images` of the batch (all by default) -> (rc, dict of outputs, canaries intact)"""
    dev = torch.device("cuda:0")
    images = list(range(b["B"])) if images is None else images
    off, C, H, W = b["box_off"], b["C"], b["H"], b["W"]
    sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in images] + [np.zeros(0, np.int64)]).astype(np.int64)
    sizes = [int(off[i + 1] - off[i]) for i in images]
    nh = [int(b["n_human"][i]) for i in images]
    N, Pt = len(sel), sum(h * (n - 1) if n > 1 else 0 for n, h in zip(sizes, nh))
    t = {k: torch.from_numpy(np.ascontiguousarray(b[k][sel])).to(dev) for k in ("boxes", "scores", "labels")}
    feat = torch.from_numpy(np.ascontiguousarray(b["feat"][images])).to(dev)
    fg = torch.from_numpy(np.ascontiguousarray(b["feat_global"][images])).to(dev)
    o2t = torch.from_numpy(b["obj2target"]).to(dev)
    nb = len(branches)
    shapes = {"pair_h": (Pt, 1), "pair_o": (Pt, 1), "objects": (Pt, 1), "union_boxes": (Pt, 4), "pooled_single": (N, C), "pooled_union": (Pt, C),
              "feats": (Pt, 3 * C), "branch_logits": (nb * Pt, NC), "logits": (Pt, NC), "prior": (2 * Pt, NC), "scores_out": (Pt, NC)}
    if not nb:
        for k in ("feats", "branch_logits", "logits", "prior", "scores_out"):
            shapes.pop(k)
    out = {k: canaried(r, c, dev) for k, (r, c) in shapes.items()} if outputs else {"logits": canaried(Pt, NC, dev)}
    a = _lib.hg_hoi_head_args()
    a.feat_local, a.feat_global, a.boxes, a.scores, a.labels = feat.data_ptr(), fg.data_ptr(), t["boxes"].data_ptr(), t["scores"].data_ptr(), t["labels"].data_ptr()
    box_off = (_lib.C.c_int32 * (len(images) + 1))(*np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist())
    n_human = (_lib.C.c_int32 * max(len(images), 1))(*nh)
    a.box_off, a.n_human = box_off, n_human
    a.B, a.C, a.H, a.W, a.P, a.spatial_scale = len(images), C, H, W, P, float(b["scale"])
    a.n_branch = nb
    for i, (src, cache, scale) in enumerate(branches):
        a.branch[i].source, a.branch[i].slot, a.branch[i].scale = _lib.HG_HOI_SRC[src], cache.slot, scale
    a.obj2target, a.n_obj_classes, a.num_classes, a.score_pow = o2t.data_ptr(), o2t.shape[0], NC, power
    for k, v in out.items():
        setattr(a, k, v[1:].data_ptr())
    for k, v in override.items():
        if k.startswith("branch_"):
            setattr(a.branch[0], k[7:], v)
        else:
            setattr(a, k, v)
    rc = _lib.lib().hg_hoi_head(ctx or _lib.ctx(0), _lib.C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = all(bool((v[0] == CANARY).all()) and bool((v[-1] == CANARY).all()) for v in out.values())
    res = {}
    for k, v in out.items():
        r, c = shapes[k] if k in shapes else (Pt, NC)
        body = v[1:r + 1, :c]
        res[k] = body.reshape(-1).clone() if k in ("pair_h", "pair_o", "objects") else body.contiguous().view(torch.float32)
    return rc, res, intact


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def same_values(a, b):
    """bit-equal where finite, NaN where NaN (a NaN's payload is not held)"""
    a, b = a.cpu().numpy(), (b.cpu().numpy() if isinstance(b, torch.Tensor) else b)
    na, nb_ = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb_) and np.array_equal(a[~na], b[~nb_])


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    H, W, C, size, sk, sizes, humans, with_branches, power = CASES[name]
    dev = torch.device("cuda:0")
    b = batch_of(name)
    pr = b["pairs"]
    Pt = len(pr["pair_h"])
    branches = make_branches(C, dev) if with_branches else []
    fails = []
    try:
        rc, got, intact = call(b, branches, power)
        assert rc == 0, _lib.lib().hg_last_error(_lib.ctx(0))
        if not intact:
            fails.append("a row in front of or behind an output was written")
        # ---- integer outputs, union boxes
        for k in ("pair_h", "pair_o", "objects"):
            if not np.array_equal(got[k].cpu().numpy(), pr[k]):
                fails.append(f"{k} differs")
        if not same_bits(got["union_boxes"], pr["union_boxes"]):
            fails.append("union boxes differ")
        # ---- pooled means: rule 1, rule 2, hg_roi_align
        want_s, want_u, refs = expected_pool(name)
        for k, want in (("pooled_single", want_s), ("pooled_union", want_u)):
            if not same_bits(got[k], want):
                g = got[k].cpu().numpy()
                bad = g.view(np.int32) != want.view(np.int32)
                fails.append(f"{k}: {int(bad.sum())} of {bad.size} means are not the restatement's bits, first at {tuple(np.argwhere(bad)[0])}")
        worst = worst_roi = 0.0
        for i in range(b["B"]):
            lo, hi, plo, phi = b["box_off"][i], b["box_off"][i + 1], pr["pair_off"][i], pr["pair_off"][i + 1]
            mine = torch.cat([got["pooled_single"][lo:hi], got["pooled_union"][plo:phi]])
            worst = max(worst, hb.worst(mine.cpu().numpy(), refs[i]))
            rois = torch.from_numpy(np.concatenate([b["boxes"][lo:hi], pr["union_boxes"][plo:phi]])).to(dev)
            theirs = roi_align(torch.from_numpy(b["feat"][i]).to(dev), rois, P, float(b["scale"]), reduce_mean=True)
            k = refs[i]["kept"]
            d = np.abs(mine.cpu().numpy().astype(np.float64) - theirs.cpu().numpy())[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(d == 0, 0.0, d / (refs[i]["E"] + refs[i]["roi_E"])[k])
            worst_roi = max(worst_roi, float(r.max()) if r.size else 0.0)
        print(f"\nHOI_RATIO {name} kernel: mean {worst:.3f}; against hg_roi_align over both bounds {worst_roi:.3f}")
        if not (worst <= 1.0 and worst_roi <= 1.0):
            fails.append(f"float64 rule: {worst:.3f}; against hg_roi_align {worst_roi:.3f}")
        if with_branches:
            fails += check_head(b, got, branches, power, dev, want_s, want_u)
            # ---- a repeated call, and the images one at a time
            _, again, _ = call(b, branches, power)
            for k in got:
                if not same_bits(got[k], again[k]):
                    fails.append(f"{k}: a repeated call differs")
            parts = [call(b, branches, power, images=[i])[1] for i in range(b["B"])] if b["B"] > 1 else []
            for k in (got if parts else ()):
                if k == "prior":
                    joined = torch.cat([torch.cat([p[k][:len(p[k]) // 2] for p in parts]), torch.cat([p[k][len(p[k]) // 2:] for p in parts])])
                elif k == "branch_logits":
                    joined = torch.cat([torch.cat([p[k].view(len(branches), -1, NC)[j] for p in parts]) for j in range(len(branches))])
                else:
                    joined = torch.cat([p[k] for p in parts])
                if not same_bits(got[k], joined):
                    fails.append(f"{k}: the {b['B']}-image call differs from {b['B']} one-image calls")
    finally:
        for _, c, _ in branches:
            c.close()
    assert not fails, fails


def check_head(b, got, branches, power, dev, want_s, want_u):
    fails = []
    pr, C = b["pairs"], b["C"]
    Pt = len(pr["pair_h"])
    gx = torch.from_numpy(b["box_off"][pr["image"]] + pr["pair_h"]).to(dev).long()
    gy = torch.from_numpy(b["box_off"][pr["image"]] + pr["pair_o"]).to(dev).long()
    # ---- feats == hg_l2_normalize of the returned means
    rows = torch.cat([got["pooled_single"][gx], got["pooled_single"][gy], got["pooled_union"]], 1).reshape(3 * Pt, C)
    if not same_values(got["feats"], vae.l2_normalize(rows).reshape(Pt, 3 * C)):
        fails.append("feats are not hg_l2_normalize of the returned means")
    # ---- NaN of a box that pools to zero (the zero-width box 1 of an image of six or more; a box wholly outside the map) in its own
    # pairs only
    empty = (want_s == 0).all(1)
    dirty = empty[gx.cpu().numpy()] | empty[gy.cpu().numpy()] | (want_u == 0).all(1)
    for i, n in enumerate(np.diff(b["box_off"])):
        if n >= 6:
            assert empty[b["box_off"][i] + 1] and (b["n_human"][i] == 0 or dirty[pr["image"] == i].any())
    assert not dirty.all()
    for k in ("feats", "logits", "scores_out"):
        nan_rows = torch.isnan(got[k]).any(1).cpu().numpy()
        if not np.array_equal(nan_rows, dirty if k != "scores_out" else nan_rows & dirty) or (k != "scores_out" and not nan_rows[dirty].all()):
            fails.append(f"{k}: NaN rows are not the rows of the zero-width box's pairs")
    # ---- branch logits == hg_cache_logits on the returned feats
    f = got["feats"]
    src_rows = {"human": f[:, :C], "object": f[:, C:2 * C], "union": f[:, 2 * C:], "human_object": f[:, :2 * C],
                "global": vae.l2_normalize(torch.from_numpy(b["feat_global"]).to(dev))[torch.from_numpy(pr["image"]).to(dev).long()]}
    br = got["branch_logits"].view(len(branches), Pt, NC)
    for i, (src, cache, _) in enumerate(branches):
        if not same_values(br[i], cache(src_rows[src].contiguous())):
            fails.append(f"branch {i} ({src}) is not hg_cache_logits on the returned feats")
    # ---- logits == the left-to-right fp32 expression (torch on the CPU: one rounding per operation)
    bc = br.cpu()
    want = bc[0] * branches[0][2]
    for i in range(1, len(branches)):
        want = want + bc[i] * branches[i][2]
    if not same_values(got["logits"], want):
        fails.append("logits are not the left-to-right sum of the returned branches")
    # ---- priors and scores
    sx, sy = b["scores"][gx.cpu().numpy()], b["scores"][gy.cpu().numpy()]
    on = b["obj2target"][b["labels"][gy.cpu().numpy()]] != 0
    p64 = np.stack([np.where(on, sx.astype(np.float64)[:, None] ** float(np.float32(power)), 0.0),
                    np.where(on, sy.astype(np.float64)[:, None] ** float(np.float32(power)), 0.0)])
    prior = got["prior"].view(2, Pt, NC).cpu().numpy()
    if power == 1.0:
        if not np.array_equal(prior, p64.astype(np.float32)):
            fails.append("prior at p = 1 is not the score itself")
    elif not (np.abs(prior - p64) <= hb.prior_bound(p64)).all():
        fails.append(f"prior: worst |err| / bound {float((np.abs(prior - p64) / np.maximum(hb.prior_bound(p64), 1e-300)).max()):.2f}")
    lg = got["logits"].cpu().numpy()
    clean = ~np.isnan(lg).any(1)
    w, e = hb.score_bound(lg[clean], p64[:, clean])
    sc = got["scores_out"].cpu().numpy()[clean]
    if not (np.abs(sc - w) <= e).all():
        fails.append(f"scores: worst |err| / bound {float((np.abs(sc - w) / e).max()):.2f}")
    return fails


def test_facade_once():
    """HOIHead on a batch whose boxes are NOT humans first: the reference's lists, against the C ABI call on the permuted batch"""
    dev = torch.device("cuda:0")
    b = batch_of("b3_one_box_between")
    branches = make_branches(b["C"], dev)
    try:
        human = 0
        rp, shuffles = [], []
        for i in range(b["B"]):
            lo, hi = b["box_off"][i], b["box_off"][i + 1]
            # a stable permutation brings this order back: objects moved in front of the humans, both in their order
            is_h = b["labels"][lo:hi] == human
            sh = np.concatenate([np.nonzero(~is_h)[0], np.nonzero(is_h)[0]])
            shuffles.append(sh)
            rp.append({k: torch.from_numpy(b[k][lo:hi][sh]).to(dev) for k in ("boxes", "scores")} | {"labels": torch.from_numpy(b["labels"][lo:hi][sh]).long().to(dev)})
        head = interaction.HOIHead(branches, torch.from_numpy(b["obj2target"]), human, NC, hyper_lambda=2.8, pool=P)
        sizes = torch.tensor([[224.0, 224.0]] * b["B"], device=dev)
        logits, prior, bh, bo, objects = head(torch.from_numpy(b["feat_global"]).to(dev), torch.from_numpy(b["feat"]).to(dev), sizes, rp)
        rc, want, _ = call(b, branches, 2.8)
        assert rc == 0
        assert same_bits(torch.cat(logits), want["logits"]) and same_bits(torch.cat(prior, 1).reshape(-1, NC), want["prior"])
        assert torch.equal(torch.cat(bh), want["pair_h"].long()) and torch.equal(torch.cat(bo), want["pair_o"].long())
        assert torch.equal(torch.cat(objects), want["objects"].long()) and objects[0].dtype == torch.int64
        assert [len(x) for x in bh] == [7 * 8, 0, 2 * 4] and prior[1].shape == (2, 0, NC) and bh[1].shape == (0,)
        det = head.postprocess([r["boxes"] for r in rp], bh, bo, logits, prior, objects, sizes)
        for i, d in enumerate(det):
            x, y = torch.nonzero(prior[i].prod(0)).unbind(1)
            lo = b["pairs"]["pair_off"][i]
            assert torch.equal(d["labels"], y) and torch.equal(d["pairing"], torch.stack([bh[i][x], bo[i][x]]))
            assert same_bits(d["scores"], want["scores_out"][lo:lo + len(bh[i])][x, y]) and torch.equal(d["objects"], objects[i][x])
        with pytest.raises(RuntimeError, match="HOIHead call returned"):
            head.postprocess([r["boxes"] for r in rp], bh, bo, [t.clone() for t in logits], prior, objects, sizes)
    finally:
        for _, c, _ in branches:
            c.close()


def test_refusals_and_pooling_only():
    dev = torch.device("cuda:0")
    b = batch_of("b3_one_box_between")
    branches = make_branches(b["C"], dev, (SIX[1], SIX[5]))      # union, global
    INVALID = -1
    try:
        spare = CacheLogits(torch.randn(NC, 2 * b["C"], device=dev))      # a loaded slot of another K
        narrow = CacheLogits(torch.randn(NC + 1, b["C"], device=dev))     # ... and one of another width
        fresh = _lib.lib().hg_create(0)                                    # a context of its own: none of its slots is loaded
        assert fresh
        rc, _, intact = call(b, branches, 1.0, outputs=False, ctx=fresh)
        msg = _lib.lib().hg_last_error(fresh)
        _lib.lib().hg_destroy(fresh)
        assert rc == INVALID and intact and b"not loaded" in msg
        cases = {"a slot out of range": dict(branch_slot=99), "a slot of another K": dict(branch_slot=spare.slot),
                 "a slot of another width": dict(branch_slot=narrow.slot), "an unknown source": dict(branch_source=7),
                 "a global source without feat_global": dict(feat_global=None), "a negative slot": dict(branch_slot=-1), "H over the limit": dict(H=33), "C over the limit": dict(C=1088),
                 "too many branches": dict(n_branch=7), "P over the limit": dict(P=33), "P = 0": dict(P=0), "too many images": dict(B=65), "no logits": dict(logits=None)}
        for what, kw in cases.items():
            rc, _, intact = call(b, branches, 1.0, outputs=False, **kw)
            assert rc == INVALID and intact, what
            assert _lib.lib().hg_last_error(_lib.ctx(0)), what
        spare.close(), narrow.close()
        # a negative step of box_off, more humans than boxes
        for off, nh in (((0, 9, 5, 15), (7, 1, 2)), ((0, 9, 10, 15), (7, 2, 2))):
            a = (_lib.C.c_int32 * 4)(*off)
            h = (_lib.C.c_int32 * 3)(*nh)
            rc, _, intact = call(b, branches, 1.0, outputs=False, box_off=a, n_human=h)
            assert rc == INVALID and intact
        # C % 64 != 0 with branches is refused; without branches it pools
        b257 = batch_of("b2_c257")
        rc, _, intact = call(b257, branches[:1], 1.0, outputs=False)
        assert rc == INVALID and intact
        o2 = torch.zeros(16, NC, device=dev)      # scores without a branch have no logits to come from
        rc, _, intact = call(b257, [], 1.0, outputs=False, logits=None, scores_out=o2.data_ptr())
        assert rc == INVALID and intact and bool((o2 == 0).all())
        rc, got, intact = call(b257, [], 1.0)
        assert rc == 0 and intact and set(got) == {"pair_h", "pair_o", "objects", "union_boxes", "pooled_single", "pooled_union"}
        # every output but logits may be missing: the logits are the same
        rc, only, intact = call(b, branches, 2.8, outputs=False)
        rc2, full, _ = call(b, branches, 2.8)
        assert rc == 0 and rc2 == 0 and intact and same_bits(only["logits"], full["logits"])
        # no images, no boxes
        rc, _, _ = call(b, branches, 1.0, images=[], outputs=False)
        assert rc == 0
    finally:
        for _, c, _ in branches:
            c.close()


def test_chunk_seams_and_ring_gemm():
    """552 pairs at C = 256 with slots of S = 200 (Sp = 256): one chunk runs the first GEMM of every labelled branch on the ring kernel
    (M >= 512, K >= 256, N % 256 == 0); option chunk_rows = 256 cuts the rows 256 + 256 + 40, = 300 (not a multiple of 256: the head
    cuts at 256) 256 + 296, = 512 one chunk of 552 with its absorbed tail.  Every cut: branches == hg_cache_logits on the returned
    feats under the DEFAULT chunking bit for bit - also the object half at column C of the lda = 2C buffer behind a seam - and every
    output of the call == the one-chunk call."""
    dev = torch.device("cuda:0")
    C = 256
    b = hb.make_batch((24, 24), (12, 12), 14, 14, C, 224, seed=77, num_classes=NC)
    b["scale"] = rb.SCALES["1/16"]
    b["feat_global"] = np.random.RandomState(6).randn(2, C).astype(np.float32)
    b["pairs"] = pr = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    Pt = len(pr["pair_h"])
    assert Pt == 552
    branches = make_branches(C, dev, S=200)
    handle, v = _lib.ctx(0), _lib.C.c_int32()
    assert _lib.lib().hg_get_option(handle, b"chunk_rows", _lib.C.byref(v)) == 0
    prev = int(v.value)
    assert prev >= 552 + 24

    def set_chunk(n):
        assert _lib.lib().hg_set_option(handle, b"chunk_rows", int(n)) == 0

    try:
        rc, one, intact = call(b, branches, 2.8)
        assert rc == 0 and intact
        want_s = np.concatenate([hb.pool(b["feat"][i], b["boxes"][b["box_off"][i]:b["box_off"][i + 1]], P, b["scale"]) for i in range(2)])
        assert same_bits(one["pooled_single"], want_s)
        f = one["feats"]
        src_rows = {"human": f[:, :C], "object": f[:, C:2 * C], "union": f[:, 2 * C:], "human_object": f[:, :2 * C],
                    "global": vae.l2_normalize(torch.from_numpy(b["feat_global"]).to(dev))[torch.from_numpy(pr["image"]).to(dev).long()]}
        want_br = [cache(src_rows[src].contiguous()) for src, cache, _ in branches]
        for chunk in (prev, 256, 300, 512):
            set_chunk(chunk)
            rc, got, intact = call(b, branches, 2.8)
            assert rc == 0 and intact, chunk
            br = got["branch_logits"].view(len(branches), Pt, NC)
            for i, (src, _, _) in enumerate(branches):
                assert same_values(br[i], want_br[i]), f"chunk_rows {chunk}: branch {i} ({src}) is not hg_cache_logits on the returned feats"
            for k in got:
                assert same_values(got[k], one[k]) if got[k].dtype == torch.float32 else torch.equal(got[k], one[k]), (chunk, k)
    finally:
        set_chunk(prev)
        for _, c, _ in branches:
            c.close()
