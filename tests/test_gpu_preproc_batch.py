"""hg_preprocess_batch (hg_preproc_batch.hip) on the GPU, bit for bit: against oracle/preprocess_oracle.py on every case of
tests/preproc_cases.py and on the cases of tests/preproc_batch_model.py, grouped into calls of several images; against
hg_preprocess_crops; independent of crop order, image order, the images around and the split into calls; sentinel crop slots in front
of and behind every output untouched; refusals as specified with their neighbours unchanged; the whole-image view; the workspace's old
bytes; and records.emit_records against records.emit_record.

    uint8 crops   array_equal          fp32 planes   array_equal as int32 bit patterns (a refused crop: 0x7fc00000)

tests/test_preproc_batch_model.py proves on the CPU which wrong kernels these cases reject.  The oracle's results are
preproc_cases.expected / preproc_batch_model.expected, cached across the test files of one pytest process."""
import ctypes

import numpy as np
import pytest
import torch

import preproc_batch_model as pbm
import preproc_cases as pc
from hoigen_amd import _lib, preprocess, records

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN_BITS = 0x7fc00000


@pytest.fixture(scope="module")
def dev_images():
    return {n: torch.from_numpy(pc.image(n)).to(DEV) for n in ("noise", "step")}


def raw_call(images, boxes, crop_image, n_px, flags=0, background=(0, 0, 0), return_u8=True, B=None):
    """hg_preprocess_batch through ctypes with one sentinel crop slot in front of and behind out, out_u8 and status (asserted untouched)
    -> (u8 [n, n_px, n_px, 3] or None, planes as int32 [n, 3, n_px, n_px], status [n]) as numpy"""
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    n = boxes.shape[0]
    out = torch.full((n + 2, 3, n_px, n_px), 7.25, dtype=torch.float32, device=DEV)
    u8 = torch.full((n + 2, n_px, n_px, 3), 0x5C, dtype=torch.uint8, device=DEV)
    status = torch.full((n + 2,), -77, dtype=torch.int32, device=DEV)
    bx = torch.from_numpy(boxes).to(DEV)
    ci = torch.from_numpy(np.asarray(crop_image, np.int32)).to(DEV)
    images = [im.contiguous() for im in images]
    nb = len(images)
    a = _lib.hg_preprocess_batch_args(
        (ctypes.c_void_p * nb)(*[im.data_ptr() for im in images]), (ctypes.c_int32 * nb)(*[im.shape[0] for im in images]),
        (ctypes.c_int32 * nb)(*[im.shape[1] for im in images]), nb if B is None else B, bx.data_ptr(), ci.data_ptr(), n, n_px, flags,
        (background[0] & 255) | ((background[1] & 255) << 8) | ((background[2] & 255) << 16), out[1:].data_ptr(),
        u8[1:].data_ptr() if return_u8 else None, status[1:].data_ptr())
    rc = _lib.lib().hg_preprocess_batch(_lib.ctx(0), ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    _lib.check(0, rc, "hg_preprocess_batch")
    torch.cuda.synchronize()
    o, u, s = out.cpu().numpy(), u8.cpu().numpy(), status.cpu().numpy()
    assert (o[0] == 7.25).all() and (o[-1] == 7.25).all(), "a sentinel slot of out was written"
    assert (u[0] == 0x5C).all() and (u[-1] == 0x5C).all(), "a sentinel slot of out_u8 was written"
    assert s[0] == -77 and s[-1] == -77, "a sentinel slot of status was written"
    if not return_u8:
        assert (u == 0x5C).all()
    return (u[1:-1] if return_u8 else None), o[1:-1].view(np.int32), s[1:-1]


class Guarded(preprocess.CropPreprocessor):
    """CropPreprocessor whose batch() writes into views of buffers with one sentinel crop slot in front and behind (CropPreprocessor.batch's
    `out`), asserted untouched after the call: the slices batch() hands its calls of 64 images, not only their values.  `calls` counts."""
    calls = 0

    def batch(self, images, boxes=None, return_u8=False, check=True, out=None):
        assert out is None
        images = list(images)
        n, p = (len(images) if boxes is None else sum(int(np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b).size) // 4 for b in boxes)), self.n_px
        f = torch.full((n + 2, 3, p, p), 7.25, dtype=torch.float32, device=DEV)
        u = torch.full((n + 2, p, p, 3), 0x5C, dtype=torch.uint8, device=DEV)
        s = torch.full((n + 2,), -77, dtype=torch.int32, device=DEV)
        done = False
        try:
            res = super().batch(images, boxes, return_u8, check, out=(f[1:n + 1], u[1:n + 1] if return_u8 else None, s[1:n + 1]))
            done = True
            return res
        finally:      # (also behind a refusal that raises: the calls have run)
            torch.cuda.synchronize()
            Guarded.calls += 1
            assert (f[0] == 7.25).all() and (f[-1] == 7.25).all(), "a sentinel slot of out was written"
            assert (u[0] == 0x5C).all() and (u[-1] == 0x5C).all() and (return_u8 or (u == 0x5C).all()), "a sentinel slot of out_u8 was written"
            assert s[0] == -77 and s[-1] == -77, "a sentinel slot of status was written"
            assert not done or (s[1:-1] != -77).all(), "a crop's status was not written"

def call_of(name):
    return next(names for names in pbm.CALLS if name in names)


def run_named(names, dev_images, return_u8=True, order=None, image_order=None, extra_images=()):
    """the call of `names`; order: a permutation of its crops; image_order: a permutation of its image table (crop_image follows);
    extra_images: (position, tensor) inserted into the table (crop_image follows)"""
    c = pbm.case(names[0])
    imgs, boxes, owner, slices = pbm.call_inputs(names)
    table = [dev_images[i] for i in imgs]
    if image_order is not None:
        table = [table[i] for i in image_order]
        owner = np.asarray([list(image_order).index(o) for o in owner], np.int32)
    for pos, t in extra_images:
        table.insert(pos, t)
        owner = np.where(owner >= pos, owner + 1, owner).astype(np.int32)
    if order is not None:
        boxes, owner = boxes[order], owner[order]
    u8, f, st = raw_call(table, boxes, owner, c["n_px"], pbm.flags_of(c), c["background"], return_u8)
    if order is not None:
        inv = np.argsort(order)
        u8, f, st = (None if u8 is None else u8[inv]), f[inv], st[inv]
    return u8, f, st, slices


@pytest.fixture(scope="module")
def base31(dev_images):
    return run_named(call_of("geo31"), dev_images)


@pytest.mark.parametrize("names", pbm.CALLS, ids=["+".join(n) for n in pbm.CALLS])
def test_bit_for_bit_against_the_oracle(names, dev_images):
    u8, f, st, slices = run_named(names, dev_images)
    for name, sl in slices.items():
        want_u8, want_f, want_st = pbm.expected(name)
        assert np.array_equal(st[sl], want_st), (name, st[sl])
        bad = int((u8[sl] != want_u8).sum())
        assert bad == 0, f"{name}: {bad} uint8 values differ from the oracle"
        bad = f[sl] != want_f.view(np.int32)
        assert not bad.any(), f"{name}: {int(bad.sum())} fp32 values are not the oracle's bits; first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("names", [call_of("geo31"), call_of("pad257_stretch"), call_of("mixed97_stretch"), call_of("plain518")],
                         ids=lambda n: "+".join(n))
def test_bit_for_bit_against_the_per_image_call(names, dev_images):
    """the same crops through hg_preprocess_crops, image by image (it refuses what the batch call marks: those crops are left out), and
    the batch call without out_u8"""
    u8, f, st, slices = run_named(names, dev_images)
    _, f_no_u8, st2, _ = run_named(names, dev_images, return_u8=False)
    assert np.array_equal(f, f_no_u8) and np.array_equal(st, st2)
    c = pbm.case(names[0])
    pre = preprocess.CropPreprocessor(c["n_px"], c["pad_square"], c["background"], c["stretch"], c["imagenet_norm"])
    for name, sl in slices.items():
        cc = pbm.case(name)
        keep = np.nonzero(st[sl] == 0)[0]
        out, u = pre(dev_images[cc["image"]], cc["boxes"][keep], return_u8=True)
        assert np.array_equal(u.cpu().numpy(), u8[sl][keep]), name
        assert np.array_equal(out.cpu().numpy().view(np.int32), f[sl][keep]), name
        assert np.array_equal(pre(dev_images[cc["image"]], cc["boxes"][keep]).cpu().numpy().view(np.int32), f[sl][keep]), name


def test_a_crop_does_not_depend_on_its_place_in_the_call(dev_images, base31):
    names = call_of("geo31")
    u8, f, st, _ = base31
    n = u8.shape[0]

    def same(got, what):
        assert np.array_equal(got[0], u8) and np.array_equal(got[1], f) and np.array_equal(got[2], st), what

    same(run_named(names, dev_images, order=np.arange(n)[::-1].copy()), "crop order reversed")
    same(run_named(names, dev_images, order=np.random.RandomState(5).permutation(n)), "crop order shuffled")
    same(run_named(names, dev_images, image_order=[1, 0]), "image order permuted")
    spare = torch.from_numpy(np.random.RandomState(9).randint(0, 256, size=(50, 70, 3)).astype(np.uint8)).to(DEV)
    same(run_named(names, dev_images, extra_images=[(1, spare)]), "an image without boxes in the middle")
    one = torch.full((1, 1, 3), 200, dtype=torch.uint8, device=DEV)
    same(run_named(names, dev_images, extra_images=[(0, one), (2, one)]), "1 x 1 images in the table")
    # calls of n = 1
    imgs, boxes, owner, _ = pbm.call_inputs(names)
    for i in (0, 1, n // 2, n - 1):
        g8, gf, gs = raw_call([dev_images[imgs[owner[i]]]], boxes[i:i + 1], [0], 31)
        assert np.array_equal(g8[0], u8[i]) and np.array_equal(gf[0], f[i]) and gs[0] == st[i], ("n = 1", i)
    # a 1 x 1 image of its own: every output pixel is that pixel (the weights of a row sum to 1 << 22)
    g8, _, gs = raw_call([one, dev_images["noise"]], [(0, 0, 1, 1), (5, 5, 40, 40)], [0, 1], 31)
    assert gs.tolist() == [0, 0] and (g8[0] == 200).all()


def test_batch_api_orders_splits_and_checks(dev_images, base31):
    names = call_of("geo31")
    u8, f, st, slices = base31
    imgs, boxes, owner, _ = pbm.call_inputs(names)
    pre = Guarded(31)
    per_image = [boxes[owner == b] for b in range(len(imgs))]
    by_image = np.concatenate([np.nonzero(owner == b)[0] for b in range(len(imgs))])
    table = [dev_images[i] for i in imgs]
    out, got_u8, status = pre.batch(table, per_image, return_u8=True, check=False)
    assert np.array_equal(got_u8.cpu().numpy(), u8[by_image]) and np.array_equal(out.cpu().numpy().view(np.int32), f[by_image])
    assert np.array_equal(status.cpu().numpy(), st[by_image]) and status.dtype == torch.int32
    # device boxes, host tensors and lists mixed; an image without boxes
    mixed = [torch.from_numpy(per_image[0]).to(DEV), torch.from_numpy(per_image[1])]
    spare = torch.zeros(9, 9, 3, dtype=torch.uint8, device=DEV)
    out2, status2 = pre.batch([table[0], spare, table[1]], [mixed[0], [], mixed[1]], check=False)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(status2, status)
    # check=True names the crop, its image and the reason (the call holds a box above the tap limit)
    bad = int(np.nonzero(st[by_image])[0][0])
    with pytest.raises(ValueError, match=rf"taps.*crop {bad} \(box {bad} of image 0\)"):
        pre.batch(table, per_image)
    with pytest.raises(ValueError, match=r"empty crop box: crop 2 \(box 0 of image 1\)"):
        pre.batch(table, [[(0, 0, 9, 9), (1, 1, 5, 5)], [(4, 4, 4, 8)]])
    # sum n_b = 0
    empty = pre.batch(table, [[], np.zeros((0, 4), np.int32)], return_u8=True)
    assert empty[0].shape == (0, 3, 31, 31) and empty[1].shape == (0, 31, 31, 3)
    with pytest.raises(RuntimeError):
        pre.batch([table[0].cpu()], None)
    with pytest.raises(TypeError):
        pre.batch(table[:1], [np.array([[0.5, 0, 9, 9]])])


def test_65_images_run_as_two_calls(dev_images):
    """views of `noise` of 65 sizes, two crops each: the one batch() equals the per-image calls crop for crop"""
    pre = Guarded(31, pad_square=True, background=pc.BG)
    imgs = [dev_images["noise"][i:i + 40 + i, 2 * i:2 * i + 90 - i].contiguous() for i in range(65)]
    boxes = [np.array([(3, 2, 30 + i % 7, 38), (-4, 10, 60, 30 + i % 5)], np.int32) for i in range(65)]
    out, u8 = pre.batch(imgs, boxes, return_u8=True)
    assert out.shape == (130, 3, 31, 31)
    for i in (0, 1, 31, 63, 64):
        o, u = pre(imgs[i], boxes[i], return_u8=True)
        assert torch.equal(u, u8[2 * i:2 * i + 2]) and torch.equal(o.view(torch.int32), out[2 * i:2 * i + 2].view(torch.int32)), i
    again = torch.cat([pre.batch(imgs[:64], boxes[:64]), pre.batch(imgs[64:], boxes[64:])])
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))


def test_refusals(dev_images):
    """an empty box, a box one tap above the limit and an image index of B between good crops: rejected inputs - status bits, NaN planes,
    zero bytes - with the neighbours bit-equal to the call without them"""
    table = [dev_images["noise"], dev_images["step"]]
    good = [((7, 9, 100, 120), 0), ((0, 0, 160, 120), 1), ((-20, -40, 352, 340), 0), ((30, 20, 61, 110), 1)]
    at_good, at_bad = [0, 2, 5, 8], [1, 3, 4, 6, 7]
    for n_px in (31, 97):
        above = (-20, -20, 16 * n_px - 19, 16 * n_px - 19)      # 16 n_px + 1 pixels a side: 67 taps (at 31: preproc_batch_model.ABOVE_BOX)
        assert pc._taps(16 * n_px + 1, n_px) == 67 and pc._taps(16 * n_px, n_px) == 65
        bad = [((50, 50, 50, 90), 0, pbm.EMPTY), (above, 0, pbm.TAPS), ((7, 9, 100, 120), 2, pbm.IMAGE), ((9, 9, 2, 2), 5, pbm.EMPTY | pbm.IMAGE),
               ((0, 0, (1 << 20) + 1, 9), 1, pbm.TAPS)]
        mixed = [good[0], bad[0][:2], good[1], bad[1][:2], bad[2][:2], good[2], bad[3][:2], bad[4][:2], good[3]]
        want = raw_call(table, [b for b, _ in good], [i for _, i in good], n_px)
        got = raw_call(table, [b for b, _ in mixed], [i for _, i in mixed], n_px)
        assert got[2].tolist() == [0, pbm.EMPTY, 0, pbm.TAPS, pbm.IMAGE, 0, pbm.EMPTY | pbm.IMAGE, pbm.TAPS, 0] and not want[2].any()
        assert np.array_equal(got[0][at_good], want[0]) and np.array_equal(got[1][at_good], want[1])
        assert not got[0][at_bad].any() and (got[1][at_bad] == NAN_BITS).all()
        no_u8 = raw_call(table, [b for b, _ in mixed], [i for _, i in mixed], n_px, return_u8=False)
        assert np.array_equal(no_u8[1], got[1]) and np.array_equal(no_u8[2], got[2])
    # the host's own limits
    for kw, what in ((dict(n_px=519), "n_px"), (dict(n_px=31, B=65), "B"), (dict(n_px=31, B=0), "B")):
        with pytest.raises(RuntimeError, match=what):
            raw_call(table, [good[0][0]], [0], **kw)


def test_whole_image_view(dev_images):
    """batch(images, None) with stretch and the ImageNet constants: the detector's CLIP view of every image of a batch"""
    pre = Guarded(224, stretch=True, imagenet_norm=True)
    imgs = [dev_images["noise"], dev_images["step"], dev_images["noise"][:200, :333].contiguous()]
    out = pre.batch(imgs, None)
    assert out.shape == (3, 3, 224, 224)
    for i, im in enumerate(imgs):
        want = pre(im, [(0, 0, im.shape[1], im.shape[0])])
        assert torch.equal(want.view(torch.int32)[0], out.view(torch.int32)[i]), i
    want_u8, _ = pc.po.preprocess_boxes(pc.image("step"), np.array([(0, 0, 160, 120)], np.int32), 224, False, (0, 0, 0), True, True)
    assert np.array_equal(pre.batch(imgs[1:2], None, return_u8=True)[1].cpu().numpy(), want_u8)


def test_calls_do_not_depend_on_the_workspace_left_behind(dev_images):
    """a small call behind a large one (headers and tables keep the large call's words) and the large one again"""
    for name in ("pad257_stretch", "one_box_31", "mixed31_stretch", "pad257_stretch"):
        c = pc.BY_NAME[name]
        u8, _, st = raw_call([dev_images[c["image"]]], c["boxes"], [0] * len(c["boxes"]), c["n_px"], pbm.flags_of(c), c["background"])
        assert np.array_equal(u8, pc.expected(name)[0]) and not st.any(), name


def test_records_of_a_batch():
    """five images of different sizes with 0 .. 3 pairs on the synthetic ViT-B/16: emit_records against emit_record per image (keys,
    shapes, integer fields), its crops bit-equal to the per-image crops, its features bit-equal to encode_image of those crops
    concatenated in the same groups (a 6-crop and a 30-crop call take different paths of the tower: the per-image FEATURES are not the
    yardstick), and within the 1e-3 contract of test_record_emission_vs_oracle_chain against the oracle chain on two of the pairs"""
    from hoigen_amd import synth
    from hoigen_amd.model import build_model
    from oracle import clip_oracle as co
    rng = np.random.RandomState(21)
    sizes = [(120, 160), (97, 131), (240, 320), (64, 64), (150, 90)]
    imgs_np = [rng.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in sizes]
    imgs = [torch.from_numpy(i).to(DEV) for i in imgs_np]
    ann = []
    for (H, W), n in zip(sizes, (2, 0, 3, 1, 2)):
        def boxes():
            x0, y0 = rng.uniform(-5, W * 0.6, n), rng.uniform(-5, H * 0.6, n)
            return np.stack([x0, y0, x0 + rng.uniform(8, W * 0.5, n), y0 + rng.uniform(8, H * 0.5, n)], 1).astype(np.float32)
        ann.append(dict(boxes_h=boxes(), boxes_o=boxes(), verbs=rng.randint(0, 117, n).tolist(), objects=rng.randint(0, 80, n).tolist()))
    sd_np = synth.clip_state_dict(synth.VIT_B16, 0)
    m = build_model(synth.to_torch(sd_np)).float().to(DEV)
    for max_crops in (256, 12):
        before = Guarded.calls
        recs = records.emit_records(m, imgs, ann, max_crops=max_crops, preprocessor=Guarded(224))
        groups = records.plan_record_batches([len(a["verbs"]) for a in ann], max_crops)
        assert groups == ([(0, 5)] if max_crops == 256 else [(0, 2), (2, 4), (4, 5)]) and Guarded.calls - before == len(groups)
        pre = Guarded(224)
        crops = []
        for im, a, rec in zip(imgs, ann, recs):
            one = records.emit_record(m, im, **a)
            assert sorted(rec) == sorted(one)
            for k in one:
                assert rec[k].shape == one[k].shape and rec[k].dtype == one[k].dtype, k
            for k in ("boxes_h", "boxes_o", "verbs", "objects"):
                assert np.array_equal(rec[k], one[k]), k
            b = np.concatenate([records.pil_box(records.union_boxes(a["boxes_h"], a["boxes_o"])), records.pil_box(a["boxes_o"]),
                                records.pil_box(a["boxes_h"])]).reshape(-1, 4)
            crops.append(pre(im, b))
        for first, last in groups:
            x = torch.cat(crops[first:last])
            got_x = pre.batch(imgs[first:last], [np.concatenate([records.pil_box(records.union_boxes(a["boxes_h"], a["boxes_o"])),
                                                                 records.pil_box(a["boxes_o"]), records.pil_box(a["boxes_h"])]).reshape(-1, 4)
                                                 for a in ann[first:last]])
            assert torch.equal(got_x.view(torch.int32), x.view(torch.int32))
            if not x.shape[0]:
                continue
            feats = m.encode_image(x).float().cpu().numpy()
            at = 0
            for rec in recs[first:last]:
                n = rec["verbs"].shape[0]
                want = feats[at:at + 3 * n]
                at += 3 * n
                for k, part in (("union_features", want[:n]), ("object_features", want[n:2 * n]), ("huamn_features", want[2 * n:])):
                    assert np.array_equal(rec[k].view(np.int32), part.view(np.int32)), (k, max_crops)
    # the oracle chain on two of the pairs (image 0)
    sd = co.reference_weight_rounding(sd_np)
    ub = records.union_boxes(ann[0]["boxes_h"], ann[0]["boxes_o"])
    for key, boxes in (("union_features", ub), ("object_features", ann[0]["boxes_o"]), ("huamn_features", ann[0]["boxes_h"])):
        _, x = pc.po.preprocess_boxes(imgs_np[0], records.pil_box(boxes))
        want = co.encode_image(sd, torch.from_numpy(x)).numpy()
        err = np.linalg.norm(recs[0][key] - want, axis=1) / np.linalg.norm(want, axis=1)
        assert err.max() <= 1e-3, (key, err)
