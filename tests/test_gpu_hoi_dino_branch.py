"""The per-image branch source of hg_hoi_head (HG_HOI_SRC_IMAGE: the reference's DINO branch,
upt_tip_cache_model_free_finetune_distill3.py:1111-1115, :1184-1207) through the C ABI (hg_hoi_head_image) and once through HOIHead, held to
tests/dino_bound.py:

  image_logits      == hg_cache_logits (CacheLogits) on the rows of feat_image, bit for bit; within heads_bound's float64 bound
  the branch slab   == image_logits broadcast by the pair's image
  logits            == the restatement on the returned branches, bit for bit, the image branch first, in the middle and last of six
  scale 0           logits, scores and priors bit-identical to the same call without the image branch
  a NaN row         poisons exactly its image's pairs; the call after it is clean (the operand's padding rows are rewritten)
  refusals          every one of them returns its message and leaves the outputs untouched

Batches: hoi_head_bound.make_batch with sizes [3, 1, 0, 5] and humans [2, 1, 0, 0] (pairs, one box only, no boxes, no humans: more
images than images with pairs), and [4, 3, 2] with humans [2, 1, 1] (three images with pairs, so a wrong row shows).  K_img 64 and
2048; caches of S = 5 (padded to 128) with labels and bias -1, S = 300 with labels, and a plain linear map."""
import functools

import numpy as np
import pytest
import torch

import dino_bound as db
import heads_bound as hdb
import hoi_head_bound as hb
import roi_bound as rb
import test_gpu_hoi_head as th
from hoigen_amd import _lib, interaction
from hoigen_amd.cache_model import CacheLogits

pytestmark = pytest.mark.gpu
NC = th.NC
HG_ERR_INVALID = -1
BATCHES = {"pairs_in_one_image": ((3, 1, 0, 5), (2, 1, 0, 0)), "pairs_in_three_images": ((4, 3, 2), (2, 1, 1))}
FIVE = (("human_object", 0.5), ("union", 1.0), ("text", 2.0), ("human", 0.7), ("global", 0.3))
IMAGE_SCALE = 0.6


@functools.lru_cache(maxsize=None)
def batch_of(name):
    sizes, humans = BATCHES[name]
    b = hb.make_batch(list(sizes), list(humans), 14, 14, 64, 224, seed=sum(map(ord, name)), num_classes=NC)
    b["scale"] = rb.SCALES["1/16"]
    b["feat_global"] = np.random.RandomState(5).randn(b["B"], 64).astype(np.float32)
    b["pairs"] = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    return b


@functools.lru_cache(maxsize=None)
def image_inputs(kind, K, B):
    """(f [B, K] unit rows, w, bias, labels, lens) as CPU tensors; kind: 's5' labels + bias -1, 's300' labels, 'linear'"""
    g = torch.Generator().manual_seed(K * 31 + B + len(kind))
    f = torch.randn(B, K, generator=g)
    f = f / f.norm(dim=1, keepdim=True)
    S = {"s5": 5, "s300": 300, "linear": NC}[kind]
    w = torch.randn(S, K, generator=g)
    w = w / w.norm(dim=1, keepdim=True)
    if kind == "linear":
        return f, w, None, None, None
    lab = (torch.rand(S, NC, generator=g) < 0.2).float()
    return f, w, (-torch.ones(S) if kind == "s5" else 0.1 * torch.randn(S, generator=g)), lab, lab.sum(0).clamp_min(1.0)


def image_cache(kind, K, B, dev):
    f, w, bias, lab, lens = image_inputs(kind, K, B)
    d = lambda t: None if t is None else t.to(dev)
    return f, CacheLogits(d(w), d(bias), d(lab), d(lens))


def call_image(b, branches, f, power=2.8, **override):
    """one hg_hoi_head_image call on the whole batch, laid out as test_gpu_hoi_head.call lays out hg_hoi_head's -> (rc, outputs incl.
    'image_logits' [n_img, B, NC], canaries intact).  override: feat_image, K_img, image_logits of hg_hoi_image_args; image=False
    passes no hg_hoi_image_args at all"""
    dev = torch.device("cuda:0")
    off, C, H, W, B = b["box_off"], b["C"], b["H"], b["W"], b["B"]
    sizes = [int(off[i + 1] - off[i]) for i in range(B)]
    nh = [int(v) for v in b["n_human"]]
    N, Pt = int(off[-1]), sum(h * (n - 1) if n > 1 else 0 for n, h in zip(sizes, nh))
    t = {k: torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("boxes", "scores", "labels", "feat", "feat_global", "obj2target")}
    nb = len(branches)
    n_img = sum(src == "image" for src, _, _ in branches)
    shapes = {"pair_h": (Pt, 1), "pair_o": (Pt, 1), "objects": (Pt, 1), "union_boxes": (Pt, 4), "pooled_single": (N, C), "pooled_union": (Pt, C),
              "feats": (Pt, 3 * C), "branch_logits": (nb * Pt, NC), "logits": (Pt, NC), "prior": (2 * Pt, NC), "scores_out": (Pt, NC)}
    out = {k: th.canaried(r, c, dev) for k, (r, c) in shapes.items()}
    il = th.canaried(max(n_img, 1) * B, NC, dev)
    a = _lib.hg_hoi_head_args()
    a.feat_local, a.feat_global, a.boxes, a.scores, a.labels = (t[k].data_ptr() for k in ("feat", "feat_global", "boxes", "scores", "labels"))
    box_off = (_lib.C.c_int32 * (B + 1))(*[int(v) for v in off])
    n_human = (_lib.C.c_int32 * max(B, 1))(*nh)
    a.box_off, a.n_human = box_off, n_human
    a.B, a.C, a.H, a.W, a.P, a.spatial_scale = B, C, H, W, th.P, float(b["scale"])
    a.n_branch = nb
    for i, (src, cache, scale) in enumerate(branches):
        a.branch[i].source, a.branch[i].slot, a.branch[i].scale = _lib.HG_HOI_SRC[src], cache.slot, scale
    a.obj2target, a.n_obj_classes, a.num_classes, a.score_pow = t["obj2target"].data_ptr(), t["obj2target"].shape[0], NC, power
    for k, v in out.items():
        setattr(a, k, v[1:].data_ptr())
    fd = f.to(dev).contiguous() if f is not None else None
    im = _lib.hg_hoi_image_args(fd.data_ptr() if fd is not None else None, int(f.shape[1]) if f is not None else 0, il[1:].data_ptr())
    with_im = override.pop("image", True)
    for k, v in override.items():
        setattr(im, k, v)
    rc = _lib.lib().hg_hoi_head_image(_lib.ctx(0), _lib.C.byref(a), _lib.C.byref(im) if with_im else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out["image_logits"], shapes["image_logits"] = il, (max(n_img, 1) * B, NC)
    intact = all(bool((v[0] == th.CANARY).all()) and bool((v[-1] == th.CANARY).all()) for v in out.values())
    res = {}
    for k, v in out.items():
        r, c = shapes[k]
        body = v[1:r + 1, :c]
        res[k] = body.reshape(-1).clone() if k in ("pair_h", "pair_o", "objects") else body.contiguous().view(torch.float32)
    return rc, res, intact


def with_image(five, image, at):
    out = list(five)
    out.insert(at, image)
    return out


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("K,kind", ((64, "s5"), (2048, "s300"), (2048, "s5"), (64, "linear")))
def test_image_branch(name, K, kind):
    dev = torch.device("cuda:0")
    b = batch_of(name)
    pr = b["pairs"]
    Pt, B = len(pr["pair_h"]), b["B"]
    five = th.make_branches(64, dev, which=FIVE)
    f, cache = image_cache(kind, K, B, dev)
    fails = []
    try:
        rc0, base, _ = th.call(b, five, 2.8)
        assert rc0 == 0
        gx, gy = b["box_off"][pr["image"]] + pr["pair_h"], b["box_off"][pr["image"]] + pr["pair_o"]
        for at in (0, 3, 5):
            branches = with_image(five, ("image", cache, IMAGE_SCALE), at)
            rc, got, intact = call_image(b, branches, f)
            assert rc == 0, _lib.lib().hg_last_error(_lib.ctx(0))
            if not intact:
                fails.append(f"at {at}: a canary row was written")
            il = got["image_logits"].view(1, B, NC)[0]
            if not th.same_bits(il, cache(f.to(dev))):
                fails.append(f"at {at}: image_logits is not hg_cache_logits on feat_image")
            br = got["branch_logits"].view(6, Pt, NC).cpu().numpy()
            if not th.same_bits(br[at], db.broadcast(il.cpu().numpy(), pr["image"])):
                fails.append(f"at {at}: the branch slab is not the broadcast rows")
            rows = [il.cpu().numpy() if i == at else br[i] for i in range(6)]
            want, _, _ = db.head(rows, [i == at for i in range(6)], [s for _, _, s in branches], pr["image"], b["scores"][gx], b["scores"][gy],
                                 b["labels"][gx], b["labels"][gy], b["obj2target"], 2.8)
            if not th.same_bits(got["logits"], want):
                fails.append(f"at {at}: logits are not the left-to-right sum of the returned branches")
            for i, j in enumerate(k for k in range(6) if k != at):      # the other branches are what they are without it
                if not th.same_bits(br[j], base["branch_logits"].view(5, Pt, NC)[i]):
                    fails.append(f"at {at}: branch {j} changed with the image branch in the list")
            # ---- scale 0: the non-image outputs are the call's without the branch
            rc, zero, _ = call_image(b, with_image(five, ("image", cache, 0.0), at), f)
            assert rc == 0
            for k in ("logits", "scores_out", "prior", "pair_h", "pair_o", "objects", "feats", "pooled_single", "pooled_union"):
                if not th.same_bits(zero[k], base[k]):
                    fails.append(f"at {at}: {k} at scale 0 differs from the call without the image branch")
        # ---- the float64 bound
        fi, w, bias, lab, lens = image_inputs(kind, K, B)
        want64, E = hdb.cache_reference(db.image_case(fi, w, bias, lab, lens))
        r = hdb.worst(il.cpu().double(), want64, E)
        print(f"DINO_RATIO image_logits {name} K {K} {kind}: worst |err| / bound {r:.3f}")
        if not r <= 1.0:
            fails.append(f"image_logits outside heads_bound's bound: {r:.3f}")
    finally:
        cache.close()
        for _, c, _ in five:
            c.close()
    assert not fails, "\n".join(fails)


def test_a_nan_row_poisons_its_image_only_and_the_next_call_is_clean():
    dev = torch.device("cuda:0")
    b = batch_of("pairs_in_three_images")
    pr = b["pairs"]
    five = th.make_branches(64, dev, which=FIVE)
    f, cache = image_cache("s300", 2048, b["B"], dev)
    try:
        branches = with_image(five, ("image", cache, IMAGE_SCALE), 5)
        _, clean, _ = call_image(b, branches, f)
        # (the batch's last box lies above the map and pools to zero: its pair is NaN in every call, as in the reference)
        clean_nan = torch.isnan(clean["logits"]).any(1).cpu().numpy()
        assert not clean_nan[:8].any()
        for img in range(b["B"]):
            bad = f.clone()
            bad[img, 77] = float("nan")
            rc, got, intact = call_image(b, branches, bad)
            assert rc == 0 and intact
            nan_rows = torch.isnan(got["logits"]).any(1).cpu().numpy()
            assert np.array_equal(nan_rows, (pr["image"] == img) | clean_nan), img
            assert torch.isnan(got["logits"][torch.from_numpy(pr["image"] == img).to(dev)]).all()
            assert th.same_bits(got["logits"][torch.from_numpy(~nan_rows).to(dev)], clean["logits"][torch.from_numpy(~nan_rows).to(dev)])
            il = got["image_logits"].view(b["B"], NC)
            assert torch.isnan(il[img]).all() and th.same_bits(il[[i for i in range(b["B"]) if i != img]],
                                                               clean["image_logits"].view(b["B"], NC)[[i for i in range(b["B"]) if i != img]])
        # a NaN operand of ALL 64 rows of a larger call, then the small call: its padding rows were rewritten
        big = hb.make_batch([2] * 64, [1] * 64, 14, 14, 64, 224, seed=3, num_classes=NC)
        big["scale"], big["feat_global"] = rb.SCALES["1/16"], np.random.RandomState(6).randn(64, 64).astype(np.float32)
        rc, _, _ = call_image(big, branches, torch.full((64, 2048), float("nan")))
        assert rc == 0
        rc, after, intact = call_image(b, branches, f)
        assert rc == 0 and intact
        for k in ("logits", "scores_out", "branch_logits", "image_logits"):
            assert th.same_bits(after[k], clean[k]), k
    finally:
        cache.close()
        for _, c, _ in five:
            c.close()


def test_refusals_leave_the_outputs_untouched():
    dev = torch.device("cuda:0")
    b = batch_of("pairs_in_one_image")
    five = th.make_branches(64, dev, which=FIVE)[:2]
    f, cache = image_cache("s5", 64, b["B"], dev)
    f2048, wide = image_cache("s300", 2048, b["B"], dev)
    narrow = CacheLogits(torch.randn(NC + 1, 64, device=dev))      # a linear map of the wrong width
    try:
        branches = five + [("image", cache, IMAGE_SCALE)]
        cases = [("without feat_image", branches, f, dict(feat_image=None)), ("without feat_image", branches, f, dict(image=False)),
                 ("K_img", branches, f, dict(K_img=0)), ("K_img", branches, f, dict(K_img=-64)), ("K_img", branches, f, dict(K_img=96)),
                 ("K_img", branches, f2048, dict(K_img=4096 + 64)),
                 ("the branch needs", five + [("image", wide, 1.0)], f, {}),          # slot K 2048, K_img 64
                 ("the branch needs", five + [("image", narrow, 1.0)], f, {})]        # width NC + 1
        for msg, brs, feat, kw in cases:
            rc, got, intact = call_image(b, brs, feat, **kw)
            err = _lib.lib().hg_last_error(_lib.ctx(0)).decode()
            assert rc == HG_ERR_INVALID and msg in err and "hg_hoi_head" in err, (msg, kw, rc, err)
            assert intact
            for k, v in got.items():
                assert bool((v.contiguous().view(torch.int32) == th.CANARY).all()), f"{msg} {kw}: {k} was written"
        rc, got, intact = call_image(b, branches, f)      # and the context still works
        assert rc == 0 and intact and th.same_bits(got["image_logits"].view(b["B"], NC), cache(f.to(dev)))
    finally:
        for c in [cache, wide, narrow] + [c for _, c, _ in five]:
            c.close()


def test_facade():
    """HOIHead with an ("image", ..) branch: against the C ABI call; without feat_image it raises; feat_image without such a branch is
    ignored"""
    dev = torch.device("cuda:0")
    b = batch_of("pairs_in_three_images")
    five = th.make_branches(64, dev, which=FIVE)
    f, cache = image_cache("s300", 2048, b["B"], dev)
    try:
        rp = []
        for i in range(b["B"]):
            lo, hi = b["box_off"][i], b["box_off"][i + 1]
            rp.append({k: torch.from_numpy(b[k][lo:hi]).to(dev) for k in ("boxes", "scores")} | {"labels": torch.from_numpy(b["labels"][lo:hi]).long().to(dev)})
        sizes = torch.tensor([[224.0, 224.0]] * b["B"], device=dev)
        args = (torch.from_numpy(b["feat_global"]).to(dev), torch.from_numpy(b["feat"]).to(dev), sizes, rp)
        branches = five + [("image", cache, IMAGE_SCALE)]
        head = interaction.HOIHead(branches, torch.from_numpy(b["obj2target"]), 0, NC, hyper_lambda=2.8, pool=th.P)
        logits = head(*args, feat_image=f.to(dev))[0]
        rc, want, _ = call_image(b, branches, f)
        assert rc == 0 and th.same_bits(torch.cat(logits), want["logits"])
        with pytest.raises(RuntimeError, match="feat_image"):
            head(*args)
        plain = interaction.HOIHead(five, torch.from_numpy(b["obj2target"]), 0, NC, hyper_lambda=2.8, pool=th.P)
        assert th.same_bits(torch.cat(plain(*args, feat_image=f.to(dev))[0]), torch.cat(plain(*args)[0]))
    finally:
        cache.close()
        for _, c, _ in five:
            c.close()


def test_end_to_end_on_the_fixture_case():
    """ResNetFeatures.normalized -> HOIHead(feat_image=...) on the case of tests/golden/g24_dino_branch.npz, against the reference's own
    dino_cache_logits (:1112-1115 executed).  The head holds the image branch alone, so its logits are scale * row b(p) with one rounding.
    No new tolerance - the chain of bounds, per element:
      the device's rows f against the fixture's f_ref     the project's contract, relative L2 1e-3 per row (asserted)
      got against float64 on fp16(f), fp16(w)             heads_bound.cache_reference's E at K = K_img, on the rows the device returned
      that against float64 on f_ref, w                    |d phi_s| <= 1e-3 |f_ref| |w_s| (Cauchy-Schwarz on the contract) + 2^-10 (1 + 1e-3) sum_k |f_ref,k| |w_sk|
                                                          (one fp16 rounding of each operand), carried through labels / sample_len
      that against the fixture's fp32 statements          (K + S + 3) 2^-24 of sum_s (sum_k |f_ref,k w_sk| + |b_s|) lab_sc / len_c: fp32 sums in any order
    times the scale, plus 2^-24 of the result for the product."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import dino_branch_cases as dc
    import hoi_head_cases as hc
    from hoigen_amd.resnet import ResNetFeatures
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_dino_branch.npz"))
    dev = torch.device("cuda:0")
    wrapped = dc.dino_net()
    net = wrapped.net
    net.avgpool, net.fc = wrapped.avgpool, wrapped.fc
    feats = ResNetFeatures.from_module(net).to(dev).normalized(torch.from_numpy(dc.views()).to(dev))
    f, f_ref = feats.cpu().double().numpy(), G["features"].astype(np.float64)
    rel = np.linalg.norm(f - f_ref, axis=1) / np.linalg.norm(f_ref, axis=1)
    assert rel.max() < 1e-3, rel
    c = dc.caches()
    w, bias, lab, lens = (torch.from_numpy(c[k]) for k in ("dino_cache", "dino_bias", "dino_values", "dino_len"))
    w = w.t().contiguous()
    scale = dc.SCALES["dino_cache_logit"]
    cache = CacheLogits(w.to(dev), bias.to(dev), lab.to(dev), lens.to(dev))
    try:
        o2t = np.zeros((hc.N_OBJ, hc.NC), np.uint8)
        for o, tar in enumerate(hc.weights()["obj2target"]):
            o2t[o, tar] = 1
        rp = [{k: torch.from_numpy(hc.image(i)[k]).to(dev) for k in ("boxes", "scores", "labels")} for i in range(dc.B)]
        local = torch.from_numpy(np.stack([hc.image(i)["feat"] for i in range(dc.B)])).to(dev)
        head = interaction.HOIHead([("image", cache, scale)], torch.from_numpy(o2t), 0, hc.NC, hyper_lambda=hc.HYPER_LAMBDA, pool=7)
        logits = head(None, local, torch.tensor([[float(hc.IMAGE)] * 2] * dc.B, device=dev), rp, feat_image=feats)[0]
    finally:
        cache.close()
    _, E = hdb.cache_reference(db.image_case(feats.cpu(), w, bias, lab, lens))
    W, L = w.double().numpy(), lab.double().numpy() / lens.double().numpy()[None]
    aw = np.abs(f_ref) @ np.abs(W).T
    d_phi = 1e-3 * np.linalg.norm(f_ref, axis=1)[:, None] * np.linalg.norm(W, axis=1)[None] + 2.0 ** -10 * (1 + 1e-3) * aw
    fixture = (W.shape[1] + W.shape[0] + 3) * 2.0 ** -24 * ((aw + np.abs(bias.double().numpy())[None]) @ L)
    want = np.float32(scale).astype(np.float64) * G["dino_cache_logits"].astype(np.float64)
    bound = float(np.float32(scale)) * (E.numpy() + d_phi @ L + fixture) + 2.0 ** -24 * np.abs(want)
    worst = 0.0
    for i, lg in enumerate(logits):
        assert tuple(lg.shape) == (hc.HUMANS[i] * (hc.SIZES[i] - 1), hc.NC)
        err = np.abs(lg.cpu().double().numpy() - want[i][None])
        worst = max(worst, float((err / bound[i][None]).max()))
    print(f"DINO_RATIO end to end on g24: rows {rel.max():.2e} relative L2 from the fixture's; logits worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
