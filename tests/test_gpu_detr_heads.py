"""hg_load_detr_heads / hg_detr_heads (hoigen_amd/csrc/hg_detr_heads.hip) and hoigen_amd.detr.DetectionHeads on the device, against the
float64 reference and the per-element bound of tests/detr_heads_bound.py: every family and shape inside the bound with the exact
families bit for bit, the label rule, `boxes` bit for bit the fp32 restatement on the returned `pred_boxes`; NaN canaries around every
output; every combination of null outputs, strides, class_rows, a row's independence of its tile, the refusals; and the module against
torch's own fp32 modules, the DetectorFrontEnd behind it and the fixture g20 behind the native Transformer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import detr_decoder_cases as dd
import detr_encoder_cases as ec
import detr_heads_bound as hb
import detr_heads_cases as hc
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HG_ERR_INVALID, HG_ERR_NOT_LOADED = -1, -3
PAD = 16      # canary elements in front of and behind every output (64 bytes: the alignment of `boxes` stays)
OUTPUTS = ("logits", "pred_boxes", "scores", "labels", "boxes")


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def test_the_error_codes_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hoigen_amd.h")).read()
    import re
    assert int(re.search(r"HG_ERR_INVALID\s*=?\s*(-?\d+)", hdr).group(1)) == HG_ERR_INVALID
    assert int(re.search(r"HG_ERR_NOT_LOADED\s*=?\s*(-?\d+)", hdr).group(1)) == HG_ERR_NOT_LOADED


def load(ctx, c, expect=0):
    lib = _lib.lib()
    keep = [torch.from_numpy(c[k]).cuda() for k in ("wc", "bc", "w0", "b0", "w1", "b1", "w2", "b2")]
    rows = c["class_rows"]
    arr = (C.c_int32 * len(rows))(*rows) if rows is not None else None
    w = _lib.hg_detr_heads_weights(*[_lib.tensor(t) for t in keep], c["D"], c["wc"].shape[0], arr, len(rows) if rows is not None else 0)
    rc = lib.hg_load_detr_heads(ctx, C.byref(w))
    assert rc == expect, (rc, lib.hg_last_error(ctx))
    return rc


def run(ctx, c, want=(True, True), hs_dev=None, expect=0, **override):
    """one hg_detr_heads call on case c -> dict of numpy outputs (None for a null output); the canaries around every output are checked.
    hs_dev: a device tensor (or view) [L, B, Q, D] to read instead of c['hs']"""
    lib = _lib.lib()
    L, B, Q, C1 = c["L"], c["B"], c["Q"], c["C1"]
    x = torch.from_numpy(c["hs"]).cuda() if hs_dev is None else hs_dev
    n = dict(logits=L * B * Q * C1, pred_boxes=L * B * Q * 4, scores=B * Q, labels=B * Q, boxes=B * Q * 4)
    buf = {k: (torch.full((n[k] + 2 * PAD,), -77, dtype=torch.int32, device="cuda") if k == "labels" else
               torch.full((n[k] + 2 * PAD,), float("nan"), device="cuda")) for k in OUTPUTS}
    ptr = {k: buf[k][PAD:].data_ptr() for k in OUTPUTS}
    a = _lib.hg_detr_heads_args()
    a.hs, a.L, a.B, a.Q = x.data_ptr(), L, B, Q
    a.hs_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
    sizes = (C.c_float * (2 * B))(*[float(v) for v in c["sizes"].reshape(-1)])
    a.target_sizes = sizes
    a.pred_logits, a.pred_boxes = (ptr["logits"] if want[0] else None), (ptr["pred_boxes"] if want[1] else None)
    a.scores, a.labels, a.boxes = ptr["scores"], ptr["labels"], ptr["boxes"]
    for k, v in override.items():
        setattr(a, k, v)
    rc = lib.hg_detr_heads(ctx, C.byref(a), None)
    assert rc == expect, (rc, lib.hg_last_error(ctx))
    torch.cuda.synchronize()
    out = {}
    shapes = dict(logits=(L, B, Q, C1), pred_boxes=(L, B, Q, 4), scores=(B, Q), labels=(B, Q), boxes=(B, Q, 4))
    for k in OUTPUTS:
        h = buf[k].cpu()
        untouched = (lambda t: bool((t == -77).all())) if k == "labels" else (lambda t: bool(torch.isnan(t).all()))
        assert untouched(h[:PAD]) and untouched(h[PAD + n[k]:]), f"elements around {k} were written"
        written = (k == "logits" and want[0]) or (k == "pred_boxes" and want[1]) or k in ("scores", "labels", "boxes")
        if expect != 0 or not written:
            assert untouched(h), f"{k} was written"
            out[k] = None
        else:
            out[k] = h[PAD:PAD + n[k]].reshape(shapes[k]).numpy()
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("D", (128, 256))
@pytest.mark.parametrize("C1", hb.C1S)
def test_every_family_and_shape_inside_the_bound(ctx, D, C1):
    fails, top = [], {}
    for L, B, Q in hb.SHAPES:
        for family in hb.FAMILIES:
            c = hb.make_case(family, L, B, Q, D, C1, seed=hb.SEED)
            load(ctx, c)
            got = run(ctx, c)
            f, stats = hb.verdict(c, got)
            fails += [f"{family} {(L, B, Q)}: {m}" for m in f]
            top = {k: max(top.get(k, 0.0), v) for k, v in stats.items()}
    print(f"DETR_HEADS_RATIO D {D} C1 {C1}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("D,C1", [(128, 17), (256, 92)])
def test_every_combination_of_null_outputs_gives_the_same_bits(ctx, D, C1):
    c = hb.make_case("randn", 2, 2, 33, D, C1, seed=31)
    load(ctx, c)
    full = run(ctx, c)
    assert not hb.verdict(c, full)[0]
    for want in ((True, False), (False, True), (False, False)):
        got = run(ctx, c, want)
        for k in OUTPUTS:
            if got[k] is not None:
                assert same_bits(got[k], full[k]), (want, k)


def test_hs_through_strides_and_off_a_16_byte_boundary(ctx):
    c = hb.make_case("randn", 2, 3, 33, 256, 17, seed=32)
    load(ctx, c)
    full = run(ctx, c)
    lqbc = torch.from_numpy(np.ascontiguousarray(c["hs"].transpose(0, 2, 1, 3))).cuda()      # [L, Q, B, C], as the decoder's own layout
    view = lqbc.permute(0, 2, 1, 3)
    assert not view.is_contiguous()
    flat = torch.zeros(c["hs"].size + 1, device="cuda")
    flat[1:] = torch.from_numpy(c["hs"]).cuda().flatten()
    shifted = flat[1:].view(*c["hs"].shape)
    assert shifted.data_ptr() % 16 == 4
    for x in (view, shifted):
        got = run(ctx, c, hs_dev=x)
        assert all(same_bits(got[k], full[k]) for k in OUTPUTS)


def test_class_rows_are_the_gathered_weights(ctx):
    rows = [i for i in range(92) if i % 9 != 4][:80] + [91]      # 81 rows of a 92-row head, the no-object row last
    c = hb.make_case("randn", 1, 2, 33, 256, 81, seed=33, class_rows=rows)
    c["wc"], c["bc"] = np.ascontiguousarray(c["wc"][:92]), np.ascontiguousarray(c["bc"][:92])
    load(ctx, c)
    got = run(ctx, c)
    assert not hb.verdict(c, got)[0]
    wc, bc = hb.class_head(c)
    direct = dict(c, wc=np.ascontiguousarray(wc), bc=np.ascontiguousarray(bc), class_rows=None)
    load(ctx, direct)
    again = run(ctx, direct)
    assert all(same_bits(got[k], again[k]) for k in OUTPUTS)
    load(ctx, dict(c, class_rows=rows[:-1] + [92]), expect=HG_ERR_INVALID)      # an index outside the head: refused, the slot keeps its load
    load(ctx, dict(c, class_rows=rows[:-1] + [-1]), expect=HG_ERR_INVALID)
    assert all(same_bits(run(ctx, direct)[k], again[k]) for k in OUTPUTS)


@pytest.mark.parametrize("D", (128, 256))
def test_a_row_depends_on_that_row_alone(ctx, D):
    c = hb.make_case("randn", 1, 1, 33, D, 92, seed=34)
    load(ctx, c)
    full = run(ctx, c)
    for r in (0, 13, 31, 32):
        one = run(ctx, dict(c, hs=np.ascontiguousarray(c["hs"][:, :, r:r + 1]), Q=1))
        for k in OUTPUTS:
            assert same_bits(one[k][..., 0:1, :] if one[k].ndim > 2 else one[k], full[k][..., r:r + 1, :] if full[k].ndim > 2 else full[k][..., r:r + 1]), (r, k)
    poisoned = c["hs"].copy()
    poisoned[0, 0, 5] = np.nan
    got = run(ctx, dict(c, hs=poisoned))
    others = [r for r in range(33) if r != 5]
    for k in OUTPUTS:
        assert same_bits(np.ascontiguousarray(got[k][..., others, :] if got[k].ndim > 2 else got[k][..., others]),
                         np.ascontiguousarray(full[k][..., others, :] if full[k].ndim > 2 else full[k][..., others])), k
    assert np.isnan(got["logits"][0, 0, 5]).all()


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    h = lib.hg_create(0)
    try:
        c = hb.make_case("randn", 1, 1, 4, 128, 17, seed=35)
        run(h, c, expect=HG_ERR_NOT_LOADED)
        for D, C1 in ((64, 17), (384, 17), (128, 1), (128, 257)):      # d_model in {128, 256}; 2 <= C1 <= 256
            bad = dict(c, D=D, wc=np.zeros((C1, D), np.float32), bc=np.zeros(C1, np.float32), w0=np.zeros((D, D), np.float32),
                       b0=np.zeros(D, np.float32), w1=np.zeros((D, D), np.float32), b1=np.zeros(D, np.float32), w2=np.zeros((4, D), np.float32))
            load(h, bad, expect=HG_ERR_INVALID)
            assert lib.hg_last_error(h)
            run(h, c, expect=HG_ERR_NOT_LOADED)
        load(h, c)
        assert not hb.verdict(c, run(h, c))[0]
        for field, value in (("L", 0), ("L", 13), ("B", 0), ("B", 65), ("Q", 0), ("Q", 1793), ("hs", None), ("scores", None), ("labels", None),
                             ("boxes", None)):
            run(h, c, expect=HG_ERR_INVALID, **{field: value})
            assert lib.hg_last_error(h), field
        a_null = C.POINTER(C.c_float)()
        run(h, c, expect=HG_ERR_INVALID, target_sizes=a_null)
        assert not hb.verdict(c, run(h, c))[0], "a refused call disturbed the slot"
    finally:
        lib.hg_destroy(h)


# ---- the module ------------------------------------------------------------------------------------------------------------------------
class _MLP(nn.Module):      # a stand-in with the state-dict keys of the reference's MLP (detr/models/detr.py:293-305)
    def __init__(self, i, h, o, n):
        super().__init__()
        self.num_layers = n
        dims = [h] * (n - 1)
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip([i] + dims, dims + [o]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = torch.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


def _post_process(logits, pred_boxes, sizes):
    """PostProcess.forward (detr/models/detr.py:274-282) restated with torch's own ops"""
    prob = torch.softmax(logits, -1)
    scores, labels = prob[..., :-1].max(-1)
    cx, cy, w, h = pred_boxes.unbind(-1)
    boxes = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    ih, iw = sizes.unbind(1)
    return scores, labels, boxes * torch.stack([iw, ih, iw, ih], 1)[:, None, :]


def _heads(seed=20, D=256, C1=92):
    sd = {k: torch.from_numpy(v) for k, v in hc.weights(D, C1, seed).items()}
    ce, be = nn.Linear(D, C1), _MLP(D, D, 4, 3)
    ce.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("class_embed.")})
    be.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("bbox_embed.")})
    return ce.cuda().eval(), be.cuda().eval()


def test_the_module_against_torch_fp32_and_into_the_front_end():
    from hoigen_amd.detr import DetectionHeads
    from hoigen_amd.proposals import DetectorFrontEnd, RegionProposals
    ce, be = _heads()
    heads = DetectionHeads.from_modules(ce, be)
    hs = torch.randn(6, 2, 100, 256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(36))
    sizes = [(480.0, 640.0), (333.0, 500.0)]
    with torch.no_grad():
        want_l, want_b = ce(hs), be(hs).sigmoid()
        ws, wl, wb = _post_process(want_l[-1], want_b[-1], torch.tensor(sizes, device="cuda"))
    oc, ob = heads(hs)
    assert tuple(oc.shape) == (6, 2, 100, 92) and tuple(ob.shape) == (6, 2, 100, 4) and oc.dtype == ob.dtype == torch.float32
    el, eb = dd.rel_l2(oc.reshape(-1, 92).cpu(), want_l.reshape(-1, 92).cpu())[0], dd.rel_l2(ob.reshape(-1, 4).cpu(), want_b.reshape(-1, 4).cpu())[0]
    print(f"DETR_HEADS module vs torch fp32 on the device: rel L2 logits {el:.2e}, pred_boxes {eb:.2e}")
    assert el <= 1e-3 and eb <= 1e-3
    res, outs = heads.detect(hs, sizes, with_outputs=True)
    assert torch.equal(outs["pred_logits"], oc[-1]) and torch.equal(outs["pred_boxes"], ob[-1])
    res2 = heads.detect(hs, torch.tensor(sizes, device="cuda"))      # a device tensor of sizes; only the last level computed
    assert len(res) == len(res2) == 2
    for b, (r, r2) in enumerate(zip(res, res2)):
        assert sorted(r) == ["boxes", "labels", "scores"]
        assert r["scores"].dtype == torch.float32 and r["labels"].dtype == torch.int64 and r["boxes"].dtype == torch.float32
        assert tuple(r["scores"].shape) == (100,) and tuple(r["labels"].shape) == (100,) and tuple(r["boxes"].shape) == (100, 4)
        assert all(torch.equal(r[k], r2[k]) for k in r)
        assert same_bits(r["boxes"].cpu().numpy(), hb.boxes_fp32(ob[-1, b:b + 1].cpu().numpy(), np.asarray(sizes[b:b + 1]))[0])
        gap = want_l[-1, b, :, :-1].topk(2, -1).values
        clear = (gap[:, 0] - gap[:, 1]) > 2 * float((oc[-1] - want_l[-1]).abs().max())
        assert float(clear.float().mean()) >= 0.85 and torch.equal(r["labels"][clear], wl[b][clear])
        assert float((r["scores"] - ws[b]).abs().max()) <= 1e-3 and float((r["boxes"] - wb[b]).abs().max()) <= 1e-3 * 640
    # the list feeds the DetectorFrontEnd as PostProcess's does
    front = DetectorFrontEnd(RegionProposals(human_idx=0, box_score_thresh=0.0, min_instances=3, max_instances=15), None)
    props, priors = front(res, sizes)
    want_props, _ = front([{k: v.clone() for k, v in r.items()} for r in res], sizes)      # the same values in tensors of their own
    assert priors is None and len(props) == 2 and all(len(p["scores"]) >= 3 for p in props)
    for p, w in zip(props, want_props):
        assert p["labels"].dtype == torch.int64 and all(torch.equal(p[k], w[k]) for k in ("boxes", "scores", "labels"))


def test_transformer_then_heads_against_the_fixture():
    from hoigen_amd.detr import DetectionHeads, Transformer
    g, cfg, h = dd.G19, dd.FULL, hc.G20
    D = cfg["d_model"]
    t = Transformer(D, cfg["heads"], cfg["layers"], cfg["layers"], cfg["d_ff"], True)
    t.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in ec.weights(cfg, g["enc_wseed"]).items()})
    t.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in dd.weights(cfg, g["wseed"]).items()})
    t = t.cuda().eval()
    heads = DetectionHeads.from_modules(*_heads(h["wseed"], h["D"], h["C1"]))
    heads._ctx = t.encoder._ctx      # one native context for the whole path
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src, pos_map = (dev(a) for a in dd.src_map(g["B"], g["gh"], g["gw"], D, g["xseed"]))
    qe = dev(dd.inputs(g["B"], g["gh"], g["gw"], g["Q"], D, g["xseed"])[0])
    mask = dev(ec.rect_mask(g["gh"], g["gw"], g["visible"])).bool().view(g["B"], g["gh"], g["gw"])
    hs, _ = t(src, mask, qe, pos_map)
    res, outs = heads.detect(hs, h["sizes"], with_outputs=True)
    fix = np.load(os.path.join(GOLDEN, "g20_detr_heads.npz"))
    el = dd.rel_l2(outs["pred_logits"].reshape(-1, 92).cpu(), fix["logits"].reshape(-1, 92))[0]
    eb = dd.rel_l2(outs["pred_boxes"].reshape(-1, 4).cpu(), fix["pred_boxes"].reshape(-1, 4))[0]
    worst = float(np.abs(outs["pred_logits"].cpu().numpy() - fix["logits"]).max())
    top = np.sort(fix["logits"][..., :-1], -1)
    clear = (top[..., -1] - top[..., -2]) > 2 * worst
    labels = torch.stack([r["labels"] for r in res]).cpu().numpy()
    print(f"DETR_HEADS_CHAIN Transformer -> DetectionHeads against g20: rel L2 logits {el:.2e}, pred_boxes {eb:.2e}; largest logit error "
          f"{worst:.2e}; {1 - clear.mean():.1%} of the rows within twice that of a tie")
    assert el <= 1e-3 and eb <= 1e-3
    assert 1 - clear.mean() <= 0.15
    assert np.array_equal(labels[clear], fix["labels"][clear])
