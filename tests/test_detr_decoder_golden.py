"""tests/golden/g19_detr_decoder.npz and g19_detr_transformer.npz (the reference's own TransformerDecoder and Transformer in fp32, recorded
by tests/golden/make_golden_detr_decoder.py) against the float64 restatement of tests/detr_decoder_cases.py: 1e-5 relative, whole tensor
and worst row (the reference's fp32 run sits at most 5.5e-7 from its own fp64 run on these cases, worst row, as the generator prints:
more than ten times below the bound; tests/golden/README_detr_decoder.md).  CPU only."""
import os

import numpy as np
import torch

import detr_decoder_cases as dd
import detr_encoder_cases as ec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_restatement_reproduces_the_reference_decoder():
    g, cfg = dd.G19, dd.FULL
    sd = dd.weights(cfg, g["wseed"])
    qe, memory, pos = dd.inputs(g["B"], g["gh"], g["gw"], g["Q"], cfg["d_model"], g["xseed"])
    mask = ec.rect_mask(g["gh"], g["gw"], g["visible"])
    streams, hs = dd.decoder_fp64(sd, cfg, memory, pos, mask, qe)
    assert len(streams) == 6 and tuple(hs.shape) == (6, 100, 3, 256)
    fix = np.load(os.path.join(GOLDEN, "g19_detr_decoder.npz"))
    for name, layer in (("hs0", 0), ("hs_last", 5)):
        want = fix[name]
        assert want.shape == (100, 3, 256) and want.dtype == np.float32
        e, r = dd.rel_l2(hs[layer], want)
        print(f"hs[{layer}]: restatement vs fixture rel L2 {e:.2e}, worst row {r:.2e}")
        assert e < 1e-5 and r < 1e-5
    # the stream carries norm3's output, hs the final norm of it: the two differ
    assert dd.rel_l2(streams[5].view(3, 100, 256).transpose(0, 1), fix["hs_last"])[0] > 1e-2


def test_the_restatement_reproduces_the_reference_transformer():
    g, cfg = dd.G19, dd.FULL
    D = cfg["d_model"]
    src, pos_map = dd.src_map(g["B"], g["gh"], g["gw"], D, g["xseed"])
    qe = dd.inputs(g["B"], g["gh"], g["gw"], g["Q"], D, g["xseed"])[0]
    mask = ec.rect_mask(g["gh"], g["gw"], g["visible"])
    to_sbc = lambda a: np.ascontiguousarray(a.reshape(g["B"], D, -1).transpose(2, 0, 1))
    mem = ec.encoder_fp64(ec.weights(cfg, g["enc_wseed"]), cfg, to_sbc(src), to_sbc(pos_map), mask)[-1]
    mem = mem.view(g["B"], -1, D).transpose(0, 1)
    _, hs = dd.decoder_fp64(dd.weights(cfg, g["wseed"]), cfg, mem, to_sbc(pos_map), mask, qe)
    want = np.load(os.path.join(GOLDEN, "g19_detr_transformer.npz"))["hs_last"]
    assert want.shape == (3, 100, 256) and want.dtype == np.float32
    e, r = dd.rel_l2(hs[-1].transpose(0, 1), want)
    print(f"Transformer hs[-1]: restatement vs fixture rel L2 {e:.2e}, worst row {r:.2e}")
    assert e < 1e-5 and r < 1e-5


def test_weights_carry_the_decoder_key_names():
    sd = dd.weights(dd.SMALL, 19)
    assert len(sd) == 2 * 18 + 2 and sd["layers.1.multihead_attn.in_proj_weight"].shape == (384, 128) and sd["norm.weight"].shape == (128,)
    assert not np.array_equal(sd["layers.0.self_attn.in_proj_weight"], sd["layers.0.multihead_attn.in_proj_weight"])
    assert abs(sd["layers.0.norm3.weight"].mean() - 1) < 0.1
