"""Shapes that hg_load_vit accepts since patch 14 / 577 tokens and that the ViT-L/14@336px tests do not run: odd and other even
patch sizes (im2col_pad_kernel, both instances), a tower of width 768 with 257 tokens (the LayerNorm-folded blocks, the hi / lo stream
and the pair launch in front of attention_long_kernel), and hg_update_adapters' refusal of adapters on a tower of more than 224 tokens.
Reference: the CPU / fp64 oracle on the same synthetic weights; bound: the project's 1e-3 (whole matrix and worst row)."""
import numpy as np
import pytest
import torch

from hoigen_amd import _lib, synth
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
TOL = 1e-3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def check(a, b, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all(), what
    whole = float((a - b).norm() / b.norm())
    worst = float(((a - b).norm(dim=-1) / b.norm(dim=-1)).max())
    print(f"\n{what}: rel-L2 {whole:.3e}, worst row {worst:.3e}")
    assert whole <= TOL and worst <= TOL, f"{what}: rel-L2 {whole:.3e}, worst row {worst:.3e} > {TOL}"


# (patch, resolution): odd (K = 147 -> 192; 75 -> 128; 363 -> 384), even but not a multiple of 8 (300 -> 320; 588 -> 640 on a small
# grid; 432 -> 448), and a multiple of 8 on the new general rule's other side (24: 1728, no padding, the 8-pixel kernel)
@pytest.mark.parametrize("p,res", [(7, 35), (5, 40), (11, 33), (10, 40), (14, 42), (12, 36), (24, 48)])
def test_tiny_tower_at_other_patch_sizes_vs_oracle(p, res):
    from oracle import clip_oracle as co
    cfg = dict(synth.TINY, vision_patch_size=p, image_resolution=res)
    raw = synth.clip_state_dict(cfg, 20 + p)
    m = build_model(synth.to_torch(raw)).float().to(dev())
    sd = co.reference_weight_rounding(raw)
    img = torch.from_numpy(synth.crops(5, res, seed=p))
    want = co.encode_image(sd, img)
    got = m.encode_image(img.to(dev()))
    check(got, want, f"patch {p}, resolution {res}: encode_image")
    # pad columns after a non-finite call (the patch matrix shares the MLP's workspace): same bits as before it
    bad = img.clone()
    bad[0, 0, 0, 0] = float("inf")
    m.encode_image(bad.to(dev()))
    assert torch.equal(m.encode_image(img.to(dev())), got)
    # token <-> pixel block, exactly: one block of an all-zero image moves one row of the stream after ln_pre
    g = res // p
    zero = torch.zeros(1, 3, res, res, device=dev())
    _, t0 = m.visual.forward_stream_trace(zero)
    for gy, gx in ((0, 0), (g - 1, g - 2), (g // 2, g - 1)):
        one = zero.clone()
        one[0, :, p * gy:p * gy + p, p * gx:p * gx + p] = 1.0
        _, t1 = m.visual.forward_stream_trace(one)
        assert (t0[0] != t1[0]).any(dim=-1).nonzero().flatten().tolist() == [1 + g * gy + gx], (p, gy, gx)


def test_width_768_with_257_tokens_vs_oracle():
    """ViT-B/16's blocks at 256 x 256 pixels: 257 tokens take attention_long_kernel behind the LayerNorm-folded in_proj, on the hi / lo
    stream, with the MLP pair launch (8 crops = 2 056 rows); every crop against the oracle in fp64 on the device, the separate-
    LayerNorm path beside it."""
    from oracle import clip_oracle as co
    cfg = dict(synth.VIT_B16, image_resolution=256)
    raw = synth.clip_state_dict(cfg, 3)
    m = build_model(synth.to_torch(raw)).float().to(dev())
    sd = {k: v.to(dev(), torch.float64) for k, v in co.reference_weight_rounding(raw).items() if k.startswith("visual.")}
    img = torch.from_numpy(synth.crops(8, 256, seed=9)).to(dev())
    want = co.encode_image(sd, img.double(), torch.float64)
    check(m.encode_image(img), want, "width 768, 257 tokens, default path")
    for opts in ({"ln_fuse": 0}, {"last_block_row0": 0}, {"mlp_pair": 0, "stream_hilo": 0}):
        prev = {k: m.visual.get_option(k) for k in opts}
        for k, v in opts.items():
            m.visual.set_option(k, v)
        try:
            check(m.encode_image(img), want, f"width 768, 257 tokens, {opts}")
        finally:
            for k, v in prev.items():
                m.visual.set_option(k, v)


@pytest.mark.parametrize("res", [60, 65])
def test_width_256_with_adapters_on_either_side_of_the_fused_down_proj_switch(res):
    """plan_tower's own choice (tests/test_gpu_adapter.py bypasses the plan): patch 5 on 60 x 60 / 65 x 65 crops = 145 / 170 tokens, below
    and above the 161 from which down_proj runs inside the adapter's decoder; four crops (580 / 680 rows: LayerNorm folding on, the
    adapters folded into the blocks' GEMMs), with priors and without, against the oracle in fp64."""
    from oracle import clip_oracle as co
    cfg = dict(synth.TINY, vision_width=256, vision_patch_size=5, image_resolution=res)
    raw = synth.clip_state_dict(cfg, 31)
    raw.update(synth.adapter_state_dict(cfg, 32))
    m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").float().to(dev())
    assert m.visual.get_option("adapter_fold") == 1 and m.visual.get_option("ln_fuse") == 1
    sd = {k: v.double() for k, v in co.as_tensors(raw).items() if k.startswith("visual.")}
    img = torch.from_numpy(synth.crops(4, res, seed=res))
    pri, mask = synth.priors(4, n=14, dim=64, n_pad=4, seed=33)
    pri, mask = torch.from_numpy(pri), torch.from_numpy(mask)
    for prior in (None, (pri, mask)):
        want_g, want_l = co.visual_with_prior(sd, img.double(), None if prior is None else (pri.double(), mask), range(2), torch.float64)
        args = (img.to(dev()), None if prior is None else (pri.to(dev()), mask.to(dev())))
        m.visual(*args)      # (loads the weights: the context exists)
        (got_g, got_l), recs = _lib.profile(m.visual._ctx.handle, _lib.HG_PROF_ALL, 64, lambda: m.visual(*args))
        # what plan_tower chose, from the GEMM launches (kind, M, N, K): both blocks' in_proj over [x16 | e] (K = 256 + 64, folded
        # LayerNorm), no up_proj launch (K = 64), and down_proj as a GEMM of its own (kind 11, N = 128) below 161 tokens only
        gemms = [(k, M, N, K) for k, M, N, K, _ in recs]
        M = 4 * ((res // 5) ** 2 + 1)
        assert gemms.count((8, M, 768, 320)) == 2 and not [g for g in gemms if g[3] == 64], gemms
        assert gemms.count((11, M, 128, 256)) == (2 if M // 4 < 161 else 0), gemms
        tag = f"width 256, {(res // 5) ** 2 + 1} tokens, {'priors' if prior else 'no prior'}"
        check(got_g, want_g, tag + ": global")
        check(got_l.permute(0, 2, 3, 1), want_l.permute(0, 2, 3, 1), tag + ": local")


def test_more_than_32_prior_tokens_through_the_tower():
    """visual(x, (priors, mask)) with 40 prior tokens: the fp32 one-lane-per-token adapter kernels (adapter_kv_kernel,
    adapter_decoder_kernel) on the tiny tower against the oracle; with adapter_num_layers = 2 the call is refused."""
    from oracle import clip_oracle as co
    raw = synth.clip_state_dict(synth.TINY, 10)
    raw.update(synth.adapter_state_dict(synth.TINY, 13))
    m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").float().to(dev())
    img = torch.from_numpy(synth.crops(3, 32, seed=11))
    pri = torch.from_numpy(synth.hg_normal((3, 40, 64), 740))
    mask = torch.zeros(3, 40, dtype=torch.bool)
    mask[0, 33:] = True
    mask[1, ::3] = True
    mask[2, :39] = True
    want_g, want_l = co.visual_with_prior(co.as_tensors(raw), img, (pri, mask), adapter_layers=range(2))
    got_g, got_l = m.visual(img.to(dev()), (pri.to(dev()), mask.to(dev())))
    check(got_g, want_g, "tiny tower, 40 prior tokens: global")
    check(got_l.permute(0, 2, 3, 1), want_l.permute(0, 2, 3, 1), "tiny tower, 40 prior tokens: local")
    raw.update(synth.adapter_state_dict(synth.TINY, 13, num_layers=2))
    m2 = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all", adapter_num_layers=2).float().to(dev())
    with pytest.raises(RuntimeError, match="at most 32 prior tokens"):
        m2.visual(img.to(dev()), (pri.to(dev()), mask.to(dev())))


def test_update_adapters_refuses_a_tower_of_more_than_224_tokens():
    """A tower loaded without adapters (257 tokens: tiny width, patch 2 of 32 pixels) whose adapter weights arrive later through
    hg_update_adapters: HG_ERR_INVALID with the same explanation as at load."""
    cfg = dict(synth.TINY, vision_patch_size=2, image_resolution=32)
    raw = synth.to_torch(synth.clip_state_dict(cfg, 4))
    m = build_model(raw, use_adapter=True).float().to(dev())
    blocks = list(m.visual.transformer.resblocks)
    assert all(getattr(b, "adapter", False) for b in blocks)
    x = torch.from_numpy(synth.crops(2, 32, seed=1)).to(dev())
    for b in blocks:                      # first load: as a tower without adapters
        b.adapter = False
    gl, lo = m.visual(x, None)
    assert gl.shape == (2, 128) and lo.shape == (2, 128, 16, 16) and torch.isfinite(lo).all()
    for b in blocks:                      # now the adapter tensors "change": the façade sends them through hg_update_adapters
        b.adapter = True
    with torch.no_grad():
        next(p for n, p in m.visual.named_parameters() if "adaptermlp" in n).add_(1.0)
    with pytest.raises(RuntimeError, match="hg_update_adapters.*at most 224 tokens"):
        m.visual(x, None)
