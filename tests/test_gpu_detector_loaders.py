"""The failure paths and the two dtype branches of the detector's weight loaders (hg_load_detr_encoder, hg_load_detr_decoder,
hg_load_detr_neck, hg_load_mlp, hg_load_resnet_stages, hg_load_resnet_stem; hg_load_detr_heads' refusals are in test_gpu_detr_heads.py).

Per loader, through raw descriptors: the first and the last tensor field once missing and once with a dtype code that is neither fp32
nor fp16 - the return code and the whole hg_last_error text.  The ResNet descriptors hold plain fp32 pointers and no dtype code, so
there only a missing tensor can be asked for.  What a failed load leaves behind: an encoder or decoder slot is empty (the runner says
HG_ERR_NOT_LOADED) and a good load afterwards runs; the neck refuses a bad tensor before it touches its slot; a ResNet slot keeps the
weights it held, bit for bit.

Through the facades: encoder, decoder, heads and neck with parameters that are exact in fp16 give the same bits whether the parameters
arrive as fp32 or as fp16 - both branches of every conversion, and the decoder's conversions at an element offset (the K rows at D * D,
the V rows at 2 * D * D, layer 1's slice of the stacked matrices)."""
import ctypes as C

import pytest
import torch

from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

HG_ERR_INVALID, HG_ERR_NOT_LOADED = -1, -3
BAD_DTYPE = 7
D, HEADS, F = 128, 4, 128      # the transformer of this file
B, S, Q = 1, 3, 2


@pytest.fixture()
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def exact(shape, seed, scale=None, shift=0.0):
    """fp32 values on the device that fp16 holds exactly"""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    scale = (shape[-1] ** -0.5 if len(shape) > 1 else 0.1) if scale is None else scale
    return (t * scale + shift).half().float().cuda()


def broken(t, how):
    return _lib.hg_tensor(None, 0) if how == "missing" else _lib.hg_tensor(t.ptr, BAD_DTYPE)


def last_error(h):
    return _lib.lib().hg_last_error(h).decode()


def refused(h, rc, text):
    assert rc == HG_ERR_INVALID and last_error(h) == text, (rc, last_error(h))


# ---- encoder and decoder -----------------------------------------------------------------------------------------------------------------
LAYER_NAMES = {"in_proj_weight": "self_attn.in_proj_weight", "norm2_bias": "norm2.bias", "norm3_bias": "norm3.bias"}


def layer_tensors(fields, seed):
    """one layer's tensors in the order of `fields`, kept alive by the caller"""
    shapes = dict(in_proj_weight=(3 * D, D), in_proj_bias=(3 * D,), out_proj_weight=(D, D), out_proj_bias=(D,), linear1_weight=(F, D),
                  linear1_bias=(F,), linear2_weight=(D, F), linear2_bias=(D,), cross_in_proj_weight=(3 * D, D), cross_in_proj_bias=(3 * D,),
                  cross_out_proj_weight=(D, D), cross_out_proj_bias=(D,))
    return [exact(shapes.get(f, (D,)), seed + i, shift=1.0 if f.startswith("norm") and f.endswith("weight") else 0.0) for i, f in enumerate(fields)]


def encoder_weights(seed=1):
    keep = layer_tensors(_lib._DETR_LAYER_FIELDS, seed)
    arr = (_lib.hg_detr_layer_weights * 1)(_lib.hg_detr_layer_weights(*[_lib.tensor(t) for t in keep]))
    return _lib.hg_detr_encoder_weights(D, HEADS, F, 1, 0, 0, arr), [keep, arr]


def run_encoder(h, expect=0):
    x = exact((B, S, D), 50, 1.0)
    out = torch.full((B, S, D), float("nan"), device="cuda")
    a = _lib.hg_detr_encoder_args()
    a.src, a.out, a.B, a.S = x.data_ptr(), out.data_ptr(), B, S
    a.src_stride[:] = a.out_stride[:] = [S * D, D, 1]
    rc = _lib.lib().hg_detr_encoder(h, C.byref(a), None)
    assert rc == expect, (rc, last_error(h))
    torch.cuda.synchronize()
    return out


def decoder_weights(seed=100):
    keep = [layer_tensors(_lib._DETR_DEC_LAYER_FIELDS, seed + 40 * l) for l in range(2)] + [[exact((D,), seed - 1, shift=1.0), exact((D,), seed - 2)]]
    arr = (_lib.hg_detr_dec_layer_weights * 2)(*[_lib.hg_detr_dec_layer_weights(*[_lib.tensor(t) for t in keep[l]]) for l in range(2)])
    return _lib.hg_detr_decoder_weights(D, HEADS, F, 2, 0, 0, _lib.tensor(keep[2][0]), _lib.tensor(keep[2][1]), arr), [keep, arr]


def run_decoder(h, expect=0):
    mem, qpos = exact((B, S, D), 51, 1.0), exact((Q, D), 52, 1.0)
    out = torch.full((1, B, Q, D), float("nan"), device="cuda")
    a = _lib.hg_detr_decoder_args()
    a.memory, a.query_pos, a.out, a.B, a.S, a.Q = mem.data_ptr(), qpos.data_ptr(), out.data_ptr(), B, S, Q
    a.memory_stride[:] = [S * D, D, 1]
    a.query_pos_stride[:] = [0, D, 1]
    a.out_stride[:] = [B * Q * D, Q * D, D, 1]
    rc = _lib.lib().hg_detr_decoder(h, C.byref(a), None)
    assert rc == expect, (rc, last_error(h))
    torch.cuda.synchronize()
    return out


TRANSFORMER_LOADERS = {
    # loader, runner, descriptor, the layer whose first and last field are broken, that layer's last field
    "encoder": ("hg_load_detr_encoder", run_encoder, encoder_weights, 0, "norm2_bias"),
    "decoder": ("hg_load_detr_decoder", run_decoder, decoder_weights, 1, "norm3_bias"),
}


@pytest.mark.parametrize("which", sorted(TRANSFORMER_LOADERS))
def test_a_failed_transformer_load_names_the_tensor_and_empties_the_slot(ctx, which):
    name, run, weights, layer, last = TRANSFORMER_LOADERS[which]
    load = getattr(_lib.lib(), name)
    first_out = None
    for field in ("in_proj_weight", last):
        for how, text in (("missing", "missing tensor"), ("dtype", "bad dtype for")):
            w, keep = weights()
            setattr(w.layers[layer], field, broken(getattr(w.layers[layer], field), how))
            refused(ctx, load(ctx, C.byref(w)), f"{name}: {text} layers.{layer}.{LAYER_NAMES[field]}")
            run(ctx, expect=HG_ERR_NOT_LOADED)
            w, keep = weights()
            assert load(ctx, C.byref(w)) == 0, last_error(ctx)
            out = run(ctx)      # (the next round's failed load finds this slot loaded, and must empty it)
            assert bool(torch.isfinite(out).all())
            first_out = out if first_out is None else first_out
            assert torch.equal(out, first_out)


def test_the_decoders_final_norm(ctx):
    load = _lib.lib().hg_load_detr_decoder
    w, keep = decoder_weights()
    w.norm_weight = broken(w.norm_weight, "missing")
    refused(ctx, load(ctx, C.byref(w)), "hg_load_detr_decoder: the decoder's final norm (norm.weight, norm.bias) is required")
    w, keep = decoder_weights()
    w.norm_bias = broken(w.norm_bias, "dtype")
    refused(ctx, load(ctx, C.byref(w)), "hg_load_detr_decoder: bad dtype for layers.-1.norm.bias")
    run_decoder(ctx, expect=HG_ERR_NOT_LOADED)


# ---- neck --------------------------------------------------------------------------------------------------------------------------------
CIN = 64


def neck_weights(seed=200):
    keep = [exact((D, CIN), seed), exact((D,), seed + 1)]
    return _lib.hg_detr_neck_weights(_lib.tensor(keep[0]), _lib.tensor(keep[1]), CIN, D, D // 2, 10000.0, 1, 6.283185307179586), keep


def run_neck(h, expect=0):
    x = exact((1, CIN, 1, 3), 53, 1.0)
    im = torch.zeros(1, 4, 9, dtype=torch.uint8, device="cuda")
    im[:, :, 6:] = 1
    src, pos = (torch.full((1, 3, D), float("nan"), device="cuda") for _ in range(2))
    mask = torch.full((1, 3), 9, dtype=torch.uint8, device="cuda")
    a = _lib.hg_detr_neck_args()
    a.x, a.B, a.H, a.W = x.data_ptr(), 1, 1, 3
    a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(3)]
    a.image_mask, a.Hi, a.Wi = im.data_ptr(), 4, 9
    a.src, a.pos, a.mask = src.data_ptr(), pos.data_ptr(), mask.data_ptr()
    a.src_stride[:] = a.pos_stride[:] = [3 * D, D]
    rc = _lib.lib().hg_detr_neck(h, C.byref(a), None)
    assert rc == expect, (rc, last_error(h))
    torch.cuda.synchronize()
    return torch.cat([src.flatten(), pos.flatten(), mask.flatten().float()])


def test_a_failed_neck_load_names_the_tensor_and_keeps_the_slot(ctx):
    load = _lib.lib().hg_load_detr_neck
    cases = [(f, how, text) for f in ("weight", "bias") for how, text in (("missing", "missing tensor"), ("dtype", "bad dtype for"))]
    for field, how, text in cases:
        w, keep = neck_weights()
        setattr(w, field, broken(getattr(w, field), how))
        refused(ctx, load(ctx, C.byref(w)), f"hg_load_detr_neck: {text} {field}")
        run_neck(ctx, expect=HG_ERR_NOT_LOADED)
    w, keep = neck_weights()
    assert load(ctx, C.byref(w)) == 0, last_error(ctx)
    out = run_neck(ctx)
    assert bool(torch.isfinite(out).all())
    for field, how, text in cases:      # refused before the slot is touched: the neck goes on with what it held
        w, keep2 = neck_weights(seed=300)
        setattr(w, field, broken(getattr(w, field), how))
        refused(ctx, load(ctx, C.byref(w)), f"hg_load_detr_neck: {text} {field}")
        assert torch.equal(run_neck(ctx), out)


# ---- mlp_net -----------------------------------------------------------------------------------------------------------------------------
def mlp_weights(seed=400):
    keep = [exact(s, seed + i) for i, s in enumerate(((128, 64), (128,), (128, 128), (128,), (128, 128), (128,)))]
    return _lib.hg_mlp_weights(64, 128, 128, *[_lib.tensor(t) for t in keep]), keep


def run_mlp(h, expect=0):
    x = exact((5, 64), 54, 1.0)
    out = torch.full((5, 128), float("nan"), device="cuda")
    rc = _lib.lib().hg_mlp_net(h, 0, x.data_ptr(), 5, out.data_ptr(), None)
    assert rc == expect, (rc, last_error(h))
    torch.cuda.synchronize()
    return out


def test_a_failed_mlp_load_names_the_tensor(ctx):
    load = _lib.lib().hg_load_mlp
    for field, name in (("w0", "mlp.net.0.weight"), ("b4", "mlp.net.4.bias")):
        for how, text in (("missing", "missing tensor"), ("dtype", "bad dtype for")):
            w, keep = mlp_weights()
            setattr(w, field, broken(getattr(w, field), how))
            refused(ctx, load(ctx, 0, C.byref(w)), f"{text} {name}")
            run_mlp(ctx, expect=HG_ERR_NOT_LOADED)
            w, keep = mlp_weights()
            assert load(ctx, 0, C.byref(w)) == 0, last_error(ctx)
            assert bool(torch.isfinite(run_mlp(ctx)).all())


# ---- ResNet stages and stem --------------------------------------------------------------------------------------------------------------
def norm_of(n, seed, keep):
    ts = [exact((n,), seed, shift=1.0), exact((n,), seed + 1), exact((n,), seed + 2), exact((n,), seed + 3).abs() + 0.5]
    keep += ts
    return _lib.hg_resnet_norm(*[t.data_ptr() for t in ts], 1e-5)


def conv_of(cout, cin, k, stride, seed, keep):
    w = exact((cout, cin, k, k), seed, (2.0 / (cin * k * k)) ** 0.5)
    keep.append(w)
    return _lib.hg_resnet_conv(w.data_ptr(), cout, cin, k, k, stride, stride, (k - 1) // 2, (k - 1) // 2, 1, 1, 1, 0)


def stages_weights(seed=500):
    """one bottleneck 64 -> 64 -> 256 with a downsample"""
    keep = []
    arr = (_lib.hg_resnet_block * 1)()
    b = arr[0]
    b.conv1, b.conv2, b.conv3 = conv_of(64, 64, 1, 1, seed, keep), conv_of(64, 64, 3, 1, seed + 1, keep), conv_of(256, 64, 1, 1, seed + 2, keep)
    b.down_conv = conv_of(256, 64, 1, 1, seed + 3, keep)
    b.bn1, b.bn2, b.bn3, b.down_bn = (norm_of(n, seed + 10 * (i + 1), keep) for i, n in enumerate((64, 64, 256, 256)))
    b.has_downsample, b.ends_level = 1, 1
    return _lib.hg_resnet_weights(arr, 1), [keep, arr]


def run_stages(h):
    x = exact((1, 64, 2, 2), 55, 1.0).relu()
    out = torch.full((1, 256, 2, 2), float("nan"), device="cuda")
    a = _lib.hg_resnet_args()
    a.x, a.B, a.H, a.W, a.first_block, a.last_block, a.out = x.data_ptr(), 1, 2, 2, 0, 0, out.data_ptr()
    a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
    a.out_stride[:] = [out.stride(0), out.stride(1)]
    rc = _lib.lib().hg_resnet_stages(h, C.byref(a), None)
    assert rc == 0, (rc, last_error(h))
    torch.cuda.synchronize()
    return out


def test_a_failed_stages_load_names_the_pair_and_keeps_the_weights(ctx):
    load = _lib.lib().hg_load_resnet_stages
    w, keep = stages_weights()
    assert load(ctx, C.byref(w)) == 0, last_error(ctx)
    out = run_stages(ctx)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    for pair in ("conv1 / bn1", "downsample.0 / downsample.1"):
        w2, keep2 = stages_weights(seed=600)      # other weights: had the load gone through, the output would differ
        if pair.startswith("conv1"):
            w2.blocks[0].conv1.weight = None      # the descriptor's first tensor
        else:
            w2.blocks[0].down_bn.running_var = None      # ... and its last
        refused(ctx, load(ctx, C.byref(w2)), f"hg_load_resnet_stages: blocks[0]: missing tensor of {pair}")
        assert torch.equal(run_stages(ctx), out)
    w2, keep2 = stages_weights(seed=600)
    assert load(ctx, C.byref(w2)) == 0, last_error(ctx)
    assert not torch.equal(run_stages(ctx), out)


def stem_weights(seed=700):
    keep = []
    conv = conv_of(64, 3, 7, 2, seed, keep)
    return _lib.hg_resnet_stem_weights(conv, norm_of(64, seed + 1, keep), 3, 2, 1, 1, 0), keep


def run_stem(h):
    x = exact((1, 3, 8, 8), 56, 1.0)
    out = torch.full((1, 64, 2, 2), float("nan"), device="cuda")
    a = _lib.hg_resnet_stem_args()
    a.x, a.B, a.Hi, a.Wi, a.out = x.data_ptr(), 1, 8, 8, out.data_ptr()
    a.x_stride[:] = [x.stride(0), x.stride(1), x.stride(2)]
    a.out_stride[:] = [out.stride(0), out.stride(1)]
    rc = _lib.lib().hg_resnet_stem(h, C.byref(a), None)
    assert rc == 0, (rc, last_error(h))
    torch.cuda.synchronize()
    return out


def test_a_failed_stem_load_names_the_pair_and_keeps_the_weights(ctx):
    load = _lib.lib().hg_load_resnet_stem
    w, keep = stem_weights()
    assert load(ctx, C.byref(w)) == 0, last_error(ctx)
    out = run_stem(ctx)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    for first in (True, False):
        w2, keep2 = stem_weights(seed=800)
        if first:
            w2.conv1.weight = None
        else:
            w2.bn1.running_var = None
        refused(ctx, load(ctx, C.byref(w2)), "hg_load_resnet_stem: missing tensor of conv1 / bn1")
        assert torch.equal(run_stem(ctx), out)
    w2, keep2 = stem_weights(seed=800)
    assert load(ctx, C.byref(w2)) == 0, last_error(ctx)
    assert not torch.equal(run_stem(ctx), out)


# ---- fp32 and fp16 parameters give the same bits -----------------------------------------------------------------------------------------
def set_exact(module, seed):
    for i, p in enumerate(module.parameters()):
        norm_weight = p.dim() == 1 and any(p is m.weight for m in module.modules() if type(m).__name__ == "LayerNorm")
        p.data = exact(tuple(p.shape), seed + i, shift=1.0 if norm_weight else 0.0)
    return module.cuda().eval()


def both_dtypes(module, call):
    """call(module) with the parameters as fp32 and again after .half(): lists of tensors"""
    want = call(module)
    assert all(p.dtype == torch.float32 for p in module.parameters())
    got = call(module.half())
    assert all(p.dtype == torch.float16 for p in module.parameters())
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), i


def test_encoder_bits_do_not_depend_on_the_parameters_dtype():
    from hoigen_amd.detr import TransformerEncoder
    src, pos = exact((S, B, D), 60, 1.0), exact((S, B, D), 61, 1.0)
    both_dtypes(set_exact(TransformerEncoder(D, HEADS, 1, F), 900), lambda m: list(m.forward_trace(src, pos=pos)))


def test_decoder_bits_do_not_depend_on_the_parameters_dtype():
    from hoigen_amd.detr import TransformerDecoder
    mem, pos, qpos = exact((S, B, D), 62, 1.0), exact((S, B, D), 63, 1.0), exact((Q, D), 64, 1.0)
    dec = set_exact(TransformerDecoder(D, HEADS, 2, F, return_intermediate=True), 1000)
    both_dtypes(dec, lambda m: list(m.forward_trace(None, mem, pos=pos, query_pos=qpos)))


@pytest.mark.parametrize("rows", ([3, 0, 4], None))
def test_heads_bits_do_not_depend_on_the_parameters_dtype(rows):
    from hoigen_amd.detr import DetectionHeads
    hs = exact((1, 1, Q, D), 65, 1.0)

    def call(m):
        res, outs = m.detect(hs, [(30.0, 47.0)], with_outputs=True)
        return [outs["pred_logits"], outs["pred_boxes"], res[0]["scores"], res[0]["labels"], res[0]["boxes"]]

    heads = set_exact(DetectionHeads(D, 5, rows), 1100)
    assert heads.n_out == (3 if rows else 5)
    both_dtypes(heads, call)


def test_neck_bits_do_not_depend_on_the_parameters_dtype():
    from hoigen_amd.detr import DetectorNeck
    x = exact((1, CIN, 1, 3), 66, 1.0).relu()
    im = torch.zeros(1, 4, 9, dtype=torch.bool, device="cuda")
    im[:, :, 6:] = True
    both_dtypes(set_exact(DetectorNeck(CIN, D), 1200), lambda m: list(m(x, im)[:3]))
