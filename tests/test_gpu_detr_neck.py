"""hg_load_detr_neck / hg_detr_neck (hoigen_amd/csrc/hg_detr_neck.hip) through the C ABI, and the modules on top of it, on the device:
every feature and mask family inside the per-element bound of tests/detr_neck_bound.py with the exact families bit for bit and the mask
equal to F.interpolate's; NaN canaries around every output; alignment, strides and null outputs give the same bits; a NaN token and a
neighbouring image change nothing else; history independence; the fixture g21; Transformer.forward_tokens and Detector bit for bit
against the modules called by hand."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import detr_neck_bound as nb
import detr_neck_cases as nc
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HG_ERR_INVALID, HG_ERR_NOT_LOADED = -1, -3
PAD = 64      # canary elements in front of and behind every output
SEED = 21
CINS, DS = (64, 512, 2048), (128, 256)
SMALL = ((1, 1, 1), (1, 3, 5), (2, 7, 9), (3, 5, 13), (2, 4, 8))
BIG = (2, 25, 34)


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def load(ctx, c, expect=0, conv_shape=False, **override):
    lib = _lib.lib()
    w, b = torch.from_numpy(c["w"]).cuda(), torch.from_numpy(c["bias"]).cuda()
    if conv_shape:
        w = w.reshape(c["D"], c["Cin"], 1, 1)
    f = dict(cin=c["Cin"], d_model=c["D"], num_pos_feats=c["D"] // 2, temperature=c["temperature"], normalize=int(c["normalize"]),
             scale=c["scale"])
    f.update(override)
    wt = _lib.hg_detr_neck_weights(_lib.tensor(w), _lib.tensor(b), f["cin"], f["d_model"], f["num_pos_feats"], f["temperature"],
                                   f["normalize"], f["scale"])
    rc = lib.hg_load_detr_neck(ctx, C.byref(wt))
    assert rc == expect, (rc, lib.hg_last_error(ctx))
    return rc


def set_split(ctx, n):
    assert _lib.lib().hg_set_option(ctx, b"detr_neck_split", n) == 0


def run(ctx, c, want=(True, True), x_dev=None, sbc=False, expect=0, **override):
    """one hg_detr_neck call on case c -> dict of numpy outputs src, pos, mask (None for a null output); the canaries around every output
    are checked.  x_dev: a device tensor or view [B, Cin, H, W] to read instead of c['x']; sbc: src and pos through [S, B, C] strides"""
    lib = _lib.lib()
    B, H, W, D = c["B"], c["H"], c["W"], c["D"]
    S = H * W
    x = torch.from_numpy(c["x"]).cuda() if x_dev is None else x_dev
    im = torch.from_numpy(c["image_mask"]).cuda()
    n = dict(src=B * S * D, pos=B * S * D, mask=B * S)
    buf = {k: (torch.full((n[k] + 2 * PAD,), 0xAB, dtype=torch.uint8, device="cuda") if k == "mask" else
               torch.full((n[k] + 2 * PAD,), float("nan"), device="cuda")) for k in n}
    a = _lib.hg_detr_neck_args()
    a.x, a.B, a.H, a.W = x.data_ptr(), B, H, W
    a.x_stride[:] = [x.stride(0), x.stride(1), 1]
    a.image_mask, a.Hi, a.Wi = im.data_ptr(), c["Hi"], c["Wi"]
    strides = [D, B * D] if sbc else [S * D, D]
    a.src, a.src_stride[0], a.src_stride[1] = buf["src"][PAD:].data_ptr(), *strides
    if want[0]:
        a.pos, a.pos_stride[0], a.pos_stride[1] = buf["pos"][PAD:].data_ptr(), *strides
    if want[1]:
        a.mask = buf["mask"][PAD:].data_ptr()
    for k, v in override.items():
        if k.endswith("_stride2"):
            getattr(a, k[:-1])[2] = v
        else:
            setattr(a, k, v)
    rc = lib.hg_detr_neck(ctx, C.byref(a), None)
    assert rc == expect, (rc, lib.hg_last_error(ctx))
    torch.cuda.synchronize()
    out = {}
    for k in n:
        h = buf[k].cpu()
        untouched = (lambda t: bool((t == 0xAB).all())) if k == "mask" else (lambda t: bool(torch.isnan(t).all()))
        assert untouched(h[:PAD]) and untouched(h[PAD + n[k]:]), f"elements around {k} were written"
        written = k == "src" or (k == "pos" and want[0]) or (k == "mask" and want[1])
        if expect != 0 or not written:
            assert untouched(h), f"{k} was written"
            out[k] = None
        elif k == "mask":
            out[k] = h[PAD:PAD + n[k]].reshape(B, S).numpy()
        else:
            t = h[PAD:PAD + n[k]]
            out[k] = (t.reshape(S, B, D).permute(1, 0, 2) if sbc else t.reshape(B, S, D)).contiguous().numpy()
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def interpolate_mask(c):
    """backbone.py:78 on the device"""
    m = torch.from_numpy(c["image_mask"]).cuda() != 0
    return torch.stack([F.interpolate(mi[None, None].float(), size=(c["H"], c["W"])).to(torch.bool)[0, 0] for mi in m]).flatten(1).cpu().numpy()


def splits(Cin):
    """no split, the default rule, the largest the shape admits"""
    return (1, 0, Cin // 64)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("Cin", CINS)
def test_every_family_at_the_small_shapes_inside_the_bound(ctx, Cin, D):
    fails, top = [], {}
    pairs = [(f, m) for f in nc.FEATURES for m in nc.MASKS]
    for si, (B, H, W) in enumerate(SMALL):
        # every feature x mask family over the shapes and channel counts: each shape takes a sixth of the pairs per (Cin, D), all of
        # them at Cin 64, and normalize alternates
        for pi, (feat, mask) in enumerate(pairs):
            if Cin != 64 and (pi + si + (D == 256)) % 6:
                continue
            c = nc.make_case(feat, mask, B, Cin, H, W, D, SEED, normalize=(pi + si) % 3 != 0)
            load(ctx, c, conv_shape=bool(pi & 1))
            ref, want_mask = nb.reference(c), interpolate_mask(c)
            assert np.array_equal(ref["mask"], want_mask), "the reference's mask is not F.interpolate's"
            for sp in splits(Cin):
                set_split(ctx, sp)
                got = run(ctx, c)
                n_eff = Cin // 64 if sp else 8      # the default rule never exceeds 8 slices
                f, ratios = nb.check(c, got, sp or n_eff, ref)
                fails += [f"{feat} {mask} {(B, H, W)} split {sp}: {m}" for m in f]
                if not np.array_equal(got["mask"].astype(bool), want_mask):
                    fails.append(f"{feat} {mask} {(B, H, W)}: mask differs from F.interpolate")
                top = {k: max(top.get(k, 0.0), v) for k, v in ratios.items()}
    set_split(ctx, 0)
    print(f"DETR_NECK_RATIO Cin {Cin} D {D}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("feat,mask", list(zip(nc.FEATURES, nc.MASKS)))
def test_a_real_grid_of_850_tokens(ctx, feat, mask):
    B, H, W = BIG
    c = nc.make_case(feat, mask, B, 2048, H, W, 256, SEED)
    load(ctx, c)
    ref, bnd = nb.reference(c), {sp: None for sp in (1, 8, 32)}
    fails = []
    for sp in splits(2048):
        set_split(ctx, sp)
        got = run(ctx, c)
        n = sp or 8
        bnd[n] = bnd[n] or nb.bounds(c, n)
        f, ratios = nb.check(c, got, n, ref, bnd[n])
        fails += [f"split {sp}: {m}" for m in f]
        print(f"DETR_NECK_RATIO 850 tokens {feat} {mask} split {sp}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    set_split(ctx, 0)
    assert np.array_equal(ref["mask"], interpolate_mask(c))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [(2, 7, 9), (2, 4, 8)])
def test_alignment_strides_and_null_outputs_give_the_same_bits(ctx, shape):
    B, H, W = shape
    c = nc.make_case("relu", "rect", B, 512, H, W, 256, SEED)
    load(ctx, c)
    for sp in (1, 4):
        set_split(ctx, sp)
        full = run(ctx, c)
        assert not nb.check(c, full, sp)[0]
        x = torch.from_numpy(c["x"]).cuda()
        for off in (1, 2, 3):      # x 4, 8 and 12 bytes off a 16-byte boundary
            raw = torch.zeros(x.numel() + 8, device="cuda")
            xo = raw[off:off + x.numel()].view_as(x)
            xo.copy_(x)
            assert xo.data_ptr() % 16 == 4 * off
            got = run(ctx, c, x_dev=xo)
            assert all(same_bits(got[k], full[k]) for k in ("src", "pos")) and np.array_equal(got["mask"], full["mask"]), off
        big = torch.full((B + 1, c["Cin"] + 3, H + 2, W), float("nan"), device="cuda")      # x as a strided view of a larger buffer
        view = big[1:, 2:2 + c["Cin"], 1:1 + H]
        view.copy_(x)
        got = run(ctx, c, x_dev=view)
        assert all(same_bits(got[k], full[k]) for k in ("src", "pos"))
        got = run(ctx, c, sbc=True)      # outputs through [S, B, C] strides
        assert all(same_bits(got[k], full[k]) for k in ("src", "pos"))
        for want in ((True, False), (False, True), (False, False)):
            got = run(ctx, c, want)
            assert same_bits(got["src"], full["src"])
            assert got["pos"] is None or same_bits(got["pos"], full["pos"])
            assert got["mask"] is None or np.array_equal(got["mask"], full["mask"])
    set_split(ctx, 0)


def test_a_nan_token_and_a_neighbouring_image_change_nothing_else(ctx):
    c = nc.make_case("nan_token", "random", 2, 512, 7, 9, 256, SEED)
    load(ctx, c)
    b, s = c["nan_at"]
    clean = dict(c, x=c["x"].copy())
    clean["x"].reshape(2, 512, 63)[b, :, s] = 1.0
    for sp in (1, 8):
        set_split(ctx, sp)
        got, ok = run(ctx, c), run(ctx, clean)
        assert np.isnan(got["src"][b, s]).all()
        keep = np.ones((2, 63), bool)
        keep[b, s] = False
        assert same_bits(got["src"][keep], ok["src"][keep]) and same_bits(got["pos"], ok["pos"])
        for i in range(2):      # a row of the batch call equals the same image run alone
            one = dict(clean, x=clean["x"][i:i + 1].copy(), image_mask=clean["image_mask"][i:i + 1].copy(), B=1)
            alone = run(ctx, one)
            assert same_bits(alone["src"][0], ok["src"][i]) and same_bits(alone["pos"][0], ok["pos"][i])
            assert np.array_equal(alone["mask"][0], ok["mask"][i])
    set_split(ctx, 0)


def test_the_fixture(ctx):
    g = np.load(os.path.join(GOLDEN, "g21_detr_neck.npz"))
    c = nc.g21_case()
    load(ctx, c, conv_shape=True)
    ref = nb.reference(c)
    for sp in splits(c["Cin"]):
        set_split(ctx, sp)
        got = run(ctx, c)
        n = sp or 8
        bnd = nb.bounds(c, n)
        for k in ("src", "pos"):
            want = g[k].astype(np.float64)
            rel = np.linalg.norm(got[k] - want) / np.linalg.norm(want)
            slack = 4 * float(g[f"{k}_fp32_vs_fp64_max_abs"])
            worst = float((np.abs(got[k] - want) / (bnd[k] + slack)).max())
            print(f"DETR_NECK g21 {k} split {sp}: rel L2 {rel:.2e}, worst |err| / (bound + 4 x {slack / 4:.1e}) {worst:.3f}")
            assert rel < 1e-3 and worst <= 1.0
        assert np.array_equal(got["mask"].astype(bool), g["mask"])
        assert not nb.check(c, got, n, ref, bnd)[0]
    set_split(ctx, 0)


def test_refusals(ctx):
    lib = _lib.lib()
    fresh = lib.hg_create(0)
    c = nc.make_case("relu", "rect", 1, 128, 3, 5, 128, SEED)
    try:
        run(fresh, c, expect=HG_ERR_NOT_LOADED)
        for bad in (dict(d_model=192, num_pos_feats=96), dict(cin=96), dict(cin=4160), dict(num_pos_feats=32), dict(temperature=0.0)):
            load(fresh, c, expect=HG_ERR_INVALID, **bad)
        run(fresh, c, expect=HG_ERR_NOT_LOADED)
        load(fresh, c)
        for bad in (dict(B=0), dict(B=65), dict(H=0), dict(H=1793, W=1), dict(H=43, W=42), dict(Hi=0), dict(Wi=8193), dict(x=None), dict(src=None),
                    dict(image_mask=None), dict(x_stride2=2)):
            run(fresh, c, expect=HG_ERR_INVALID, **bad)
        assert lib.hg_set_option(fresh, b"detr_neck_split", 65) == HG_ERR_INVALID
        assert lib.hg_set_option(fresh, b"detr_neck_split", 3) == 0      # 128 channels are not three slices of a multiple of 64
        run(fresh, c, expect=HG_ERR_INVALID)
        assert lib.hg_set_option(fresh, b"detr_neck_split", 2) == 0
        assert not nb.check(c, run(fresh, c), 2)[0]
    finally:
        lib.hg_destroy(fresh)


# ---- the modules -------------------------------------------------------------------------------------------------------------------

def _seeded(module, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in module.parameters():
        p.data = torch.randn(p.shape, generator=gen) * (0.1 if p.dim() == 1 else float(np.prod(p.shape[1:])) ** -0.5)
    return module


class _Sine(nn.Module):
    def __init__(self, npf):
        super().__init__()
        self.num_pos_feats, self.temperature, self.normalize, self.scale = npf, 10000, True, 2 * np.pi


def _stand_in_detr(D=128, queries=7, logits=17):
    from hoigen_amd import detr as hd
    body = nn.Sequential(nn.Conv2d(3, 64, 32, stride=32), nn.ReLU())
    m = nn.Module()
    m.backbone = nn.ModuleList([nn.Module(), _Sine(D // 2)])
    m.backbone[0].body = body
    m.input_proj = nn.Conv2d(64, D, 1)
    m.transformer = hd.Transformer(D, 4, 2, 2, 256, True)
    m.class_embed, m.bbox_embed = nn.Linear(D, logits), hd.BoxMLP(D)
    m.query_embed = nn.Embedding(queries, D)
    return _seeded(m, 5).cuda().eval()


def test_forward_tokens_equals_forward_on_the_permuted_views():
    from hoigen_amd import detr as hd
    detr = _stand_in_detr()
    neck = hd.DetectorNeck.from_modules(detr.input_proj, detr.backbone[1])
    gen = torch.Generator().manual_seed(9)
    feats = torch.randn(2, 64, 5, 7, generator=gen).relu().cuda()
    im = torch.zeros(2, 160, 224, dtype=torch.bool, device="cuda")
    im[1, 120:], im[1, :, 200:] = True, True
    src, pos, mask, hw = neck(feats, im)
    assert src.shape == (2, 35, 128) and pos.shape == src.shape and mask.dtype == torch.bool and hw == (5, 7)
    tr = detr.transformer
    hs_t, mem_t = tr.forward_tokens(src, mask, detr.query_embed.weight, pos, hw)
    as_map = lambda t: t.permute(0, 2, 1).reshape(2, 128, 5, 7)      # the [B, C, H, W] views of the same two buffers
    hs_f, mem_f = tr(as_map(src), mask.view(2, 5, 7), detr.query_embed.weight, as_map(pos))
    assert torch.equal(hs_t, hs_f) and torch.equal(mem_t, mem_f) and not torch.isnan(hs_t).any()
    # and the neck against torch's own statements on the device
    want_src = detr.input_proj(feats).flatten(2).transpose(1, 2)
    assert float((src - want_src).norm() / want_src.norm()) < 1e-3
    want_mask = F.interpolate(im[None].float(), size=(5, 7)).to(torch.bool)[0].flatten(1)
    assert torch.equal(mask, want_mask)


def test_detector_equals_the_four_modules_called_by_hand():
    from hoigen_amd import detr as hd
    detr = _stand_in_detr()
    det = hd.Detector.from_module(detr)
    gen = torch.Generator().manual_seed(11)
    imgs = torch.randn(2, 3, 160, 224, generator=gen).cuda()
    im = torch.zeros(2, 160, 224, dtype=torch.bool, device="cuda")
    im[1, 100:], im[1, :, 190:] = True, True
    sizes = [(160.0, 224.0), (100.0, 190.0)]
    with torch.no_grad():
        results, hs, memory = det(imgs, im, sizes)
        feats = detr.backbone[0].body(imgs)
    neck = hd.DetectorNeck.from_modules(detr.input_proj, detr.backbone[1])
    tr = hd.Transformer.from_module(detr.transformer)
    heads = hd.DetectionHeads.from_modules(detr.class_embed, detr.bbox_embed)
    src, pos, mask, hw = neck(feats, im)
    hs2, mem2 = tr.forward_tokens(src, mask, detr.query_embed.weight, pos, hw)
    res2 = heads.detect(hs2, sizes)
    assert torch.equal(hs, hs2) and torch.equal(memory, mem2) and hs.shape == (2, 2, 7, 128)
    for a, b in zip(results, res2):
        assert all(torch.equal(a[k], b[k]) for k in ("scores", "labels", "boxes"))
    # the dict IntermediateLayerGetter returns is taken too
    det.body = type("Getter", (nn.Module,), {"forward": lambda self, t: {"0": detr.backbone[0].body(t)}})()
    with torch.no_grad():
        assert torch.equal(det(imgs, im, sizes)[1], hs)
