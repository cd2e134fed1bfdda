"""Parity of the HIP path (through the C ABI) on a real MI355X.

Three kinds of evidence, per SURVEY.md §8c/§8d:
  * golden fixtures produced by the REFERENCE ITSELF (tests/golden/*.npz) on seeded synthetic weights;
  * the CPU oracle (oracle/*.py, itself pinned to those fixtures) on other seeded inputs / sizes;
  * size-independent properties at BASELINE.json's full sizes (batch invariance, determinism).

Tolerance (north_star): relative 1e-3 vs the fp32 reference.  We assert the relative L2 error of the
whole tensor AND of every row: ||y - ref||_2 / ||ref||_2 <= 1e-3.  Integer artefacts are exact.
"""
import json
import os

import numpy as np
import pytest
import torch

from hoigen_amd import clip, synth, vae
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rel_l2(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), "non-finite values in the HIP output"
    whole = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    rows = np.linalg.norm(a2 - b2, axis=1) / np.maximum(np.linalg.norm(b2, axis=1), 1e-30)
    return whole, rows.max()


def check(a, b, tol=TOL, what=""):
    whole, worst = rel_l2(a, b)
    assert whole <= tol and worst <= tol, f"{what}: rel-L2 {whole:.3e}, worst row {worst:.3e} > {tol}"
    return whole


def ids_from_g0(g0, name, n=None):
    rows = g0[name]["ids"][:n]
    ids = np.zeros((len(rows), 77), np.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    return torch.from_numpy(ids)


@pytest.fixture(scope="module")
def g0():
    return json.load(open(f"{G}/g0_tokens.json"))


# ------------------------------------------------------------------------------------------------
# tiny configuration (golden g1: reference intermediates)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1():
    return dict(np.load(f"{G}/g1_tiny.npz"))


@pytest.fixture(scope="module")
def tinyA():
    return build_model(synth.to_torch(synth.clip_state_dict(synth.TINY, 10))).float().to(dev())


def test_tiny_image_vs_reference(g1, tinyA):
    img = torch.from_numpy(synth.crops(3, 32, seed=11)).to(dev())
    out, trace = tinyA.visual.forward_trace(img)
    check(trace[0], g1["img_ln_pre"][:, 0, :], what="CLS after ln_pre")
    for i in range(2):
        check(trace[1 + i], g1["img_blocks"][i][:, 0, :], what=f"CLS after block {i}")
    check(out, g1["img_out"], what="encode_image tiny")
    check(tinyA.encode_image(img), g1["img_out"])


def test_tiny_text_vs_reference(g1, tinyA):
    toks = torch.from_numpy(g1["txt_tokens"])
    for trunc in (True, False):
        tinyA.truncate_text = trunc
        check(tinyA.encode_text(toks.to(dev())), g1["txt_out"], what=f"encode_text tiny trunc={trunc}")
        check(tinyA.encode_text(toks.int()), g1["txt_out"])                  # int32 ids, host tensor
    tinyA.truncate_text = True


def test_tiny_variant_c_vs_reference(g1):
    sd = synth.to_torch(synth.clip_state_dict(synth.TINY, 10))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.TINY, 13)))
    m = build_model(sd, use_adapter=True, adapter_pos="all").to(dev())
    img = torch.from_numpy(synth.crops(3, 32, seed=11)).to(dev())
    pri, mask = synth.priors(3, n=6, dim=64, n_pad=2, seed=14)
    prior = (torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev()))
    g, l = m.visual(img, prior)
    assert g.shape == (3, 128) and l.shape == (3, 128, 2, 2)
    check(g, g1["c_prior_global"], what="C global (prior)")
    check(l.permute(0, 2, 3, 1), np.transpose(g1["c_prior_local"], (0, 2, 3, 1)), what="C local (prior)")
    g, l = m.visual(img, None)
    check(g, g1["c_noprior_global"], what="C global (no prior)")
    check(l.permute(0, 2, 3, 1), np.transpose(g1["c_noprior_local"], (0, 2, 3, 1)), what="C local (no prior)")
    check(m.encode_text(torch.from_numpy(g1["txt_tokens"]).int()), g1["c_txt_out"], what="C encode_text")
    # untrained adapters (reference init) are a no-op: equals the adapter-free output
    sd0 = synth.to_torch(synth.clip_state_dict(synth.TINY, 10))
    sd0.update(synth.to_torch(synth.adapter_state_dict(synth.TINY, 13, trained=False)))
    m0 = build_model(sd0, use_adapter=True).to(dev())
    g0_, l0_ = m0.visual(img, prior)
    check(g0_, g1["c_untrained_global"]); check(l0_.permute(0, 2, 3, 1), np.transpose(g1["c_untrained_local"], (0, 2, 3, 1)))
    # updating only adapter parameters is picked up (hg_update_adapters)
    with torch.no_grad():
        for k, v in synth.to_torch(synth.adapter_state_dict(synth.TINY, 13)).items():
            m0.state_dict()[k].copy_(v)
    g2_, _ = m0.visual(img, prior)
    check(g2_, g1["c_prior_global"], what="after adapter update")


def test_tiny_variant_c_two_adapter_layers_vs_reference():
    """adapter_num_layers = 2: the prior path chains mhsa_layers.0 and .1 (CLIP_models_adapter_prior2.py:179,190-195);
    the no-prior path still uses the single `mhsa` layer.  Reference outputs: make_golden_adapter_layers.py."""
    g = dict(np.load(f"{G}/g10_adapter_layers.npz"))
    sd = synth.to_torch(synth.clip_state_dict(synth.TINY, 10))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.TINY, 13, num_layers=2)))
    m = build_model(sd, use_adapter=True, adapter_pos="all", adapter_num_layers=2).to(dev())
    assert len(m.visual.transformer.resblocks[0].adaptermlp.mhsa_layers) == 2
    img = torch.from_numpy(synth.crops(3, 32, seed=11)).to(dev())
    pri, mask = synth.priors(3, n=6, dim=64, n_pad=2, seed=14)
    gl, ll = m.visual(img, (torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev())))
    check(gl, g["prior_global"], what="C global, 2 adapter layers")
    check(ll.permute(0, 2, 3, 1), np.transpose(g["prior_local"], (0, 2, 3, 1)), what="C local, 2 adapter layers")
    gl, ll = m.visual(img, None)
    check(gl, g["noprior_global"], what="C global, 2 adapter layers, no prior")
    # one layer of the same weights gives a different answer (the second layer is really applied)
    sd1 = {k: v for k, v in sd.items() if "mhsa_layers.1." not in k}
    m1 = build_model(sd1, use_adapter=True, adapter_pos="all").to(dev())
    g1_, _ = m1.visual(img, (torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev())))
    assert rel_l2(g1_, g["prior_global"])[0] > 1e-3


@pytest.mark.parametrize("n_prior,n_pad", [(1, 0), (30, 0), (30, 29), (17, 5)])
def test_variant_c_prior_counts_and_masks_vs_oracle(n_prior, n_pad):
    """The MFMA adapter decoder over the range of prior-token counts the detector produces (6 <= N <= 30,
    upt...distill3.py:1378-1398; also the degenerate N = 1) and masks that leave a single valid key, against the oracle
    on the tiny configuration; and at ViT-B/16 width on 5 crops (LayerNorm folding kept on behind the adapters)."""
    from oracle import clip_oracle as co
    for cfg, res, B, seed in ((synth.TINY, 32, 3, 31), (synth.VIT_B16, 224, 5, 32)):
        if cfg is synth.VIT_B16 and (n_prior, n_pad) != (30, 29):
            continue                                    # one full-width case is enough (CPU oracle time)
        raw = synth.clip_state_dict(cfg, 10)
        raw.update(synth.adapter_state_dict(cfg, 13))
        m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").to(dev())
        img = torch.from_numpy(synth.crops(B, res, seed=seed))
        pri = torch.from_numpy(synth.hg_normal((B, n_prior, 64), 700 + n_prior))
        mask = torch.zeros(B, n_prior, dtype=torch.bool)
        if n_pad:
            mask[:, n_prior - n_pad:] = True
        sd = co.as_tensors(raw)
        want_g, want_l = co.visual_with_prior(sd, img, (pri, mask), adapter_layers=range(cfg["vision_layers"]))
        got_g, got_l = m.visual(img.to(dev()), (pri.to(dev()), mask.to(dev())))
        check(got_g, want_g.numpy(), what=f"global N={n_prior} pad={n_pad} width={cfg['vision_width']}")
        check(got_l.permute(0, 2, 3, 1), want_l.permute(0, 2, 3, 1).numpy(), what=f"local N={n_prior} pad={n_pad}")


def test_vitb16_variant_c_without_prior_folded_path_vs_oracle():
    """No prior: the adapter's decoder attends to the sequence's own 197 tokens (`mhsa`, CLIP_models_adapter_prior2.py:196-199).
    Three crops make M = 591 >= 512 rows, i.e. the production path (adapter folded into the block's GEMMs, self-attention decoder
    with down_proj inside) - the reference fixture's no-prior case has two crops and runs the small-batch path."""
    from oracle import clip_oracle as co
    raw = synth.clip_state_dict(synth.VIT_B16, 10)
    raw.update(synth.adapter_state_dict(synth.VIT_B16, 14))
    m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").to(dev())
    img = torch.from_numpy(synth.crops(3, 224, seed=33))
    want_g, want_l = co.visual_with_prior(co.as_tensors(raw), img, None, adapter_layers=range(12))
    got_g, got_l = m.visual(img.to(dev()), None)
    check(got_g, want_g.numpy(), what="global, no prior, ViT-B/16 x 3 crops")
    check(got_l.permute(0, 2, 3, 1), want_l.permute(0, 2, 3, 1).numpy(), what="local, no prior, ViT-B/16 x 3 crops")


def test_tiny_vae_chain_vs_reference(g1, tinyA):
    D = 128
    d = dev()
    feats = vae.l2_normalize(tinyA.encode_image(torch.from_numpy(synth.crops(5, 32, seed=16)).to(d)).float())
    check(feats, g1["vae_feats"], what="normalised crop features")
    E, Gn = vae.Encoder(D, 256).to(d), vae.Generator(D, 384).to(d)
    E.load_state_dict(synth.to_torch(synth.encoder_state_dict(17, dim=D, hidden=256, wstd=0.05)))
    Gn.load_state_dict(synth.to_torch(synth.generator_state_dict(18, dim=D, hidden=384, wstd=0.05)))
    eps = torch.from_numpy(synth.hg_normal((5, D), 19)).to(d)
    gf = torch.from_numpy(g1["vae_feats"]).to(d)
    mean, lv, z, bias = vae.VAE(E, Gn)(gf, eps)
    check(mean, g1["vae_mean"], what="mean"); check(lv, g1["vae_log_var"], what="log_var")
    check(z, g1["vae_z"], what="z"); check(bias, g1["vae_bias"], what="bias")
    m2, lv2 = E(gf)
    check(m2, g1["vae_mean"]); check(lv2, g1["vae_log_var"])
    check(Gn(torch.from_numpy(g1["vae_z"]).to(d)), g1["vae_bias"], what="Generator alone")
    # prompt assembly (exact data movement + one fp32 add) and TextEncoder on embedded prompts
    cls_tok = torch.from_numpy(g1["vae_cls_tokens"]).to(d)
    emb = tinyA.token_embedding(cls_tok)
    ref_emb = synth.to_torch(synth.clip_state_dict(synth.TINY, 10))["token_embedding.weight"][cls_tok.cpu()]
    assert torch.equal(emb.cpu(), ref_emb), "token embedding gather must be exact"
    import hoigen_amd._lib as L
    from hoigen_amd.vae import _util_ctx, _stream_ptr
    ctx_v = torch.from_numpy(synth.hg_normal((3, D), 21, 0.02)).to(d)
    target = torch.from_numpy(g1["vae_target"]).to(d).int()
    gb = torch.from_numpy(g1["vae_bias"]).to(d)
    prompts = torch.empty(5, 16, D, device=d)
    pre, suf = emb[:, :1].contiguous(), emb[:, 4:].contiguous()
    h = _util_ctx.get(d)
    rc = L.lib().hg_assemble_prompts(h, pre.data_ptr(), suf.data_ptr(), ctx_v.data_ptr(), gb.data_ptr(), target.data_ptr(),
                                     5, 4, 16, 3, D, prompts.data_ptr(), _stream_ptr(d))
    assert rc == 0
    assert np.array_equal(prompts.cpu().numpy(), g1["vae_prompts"]), "prompt assembly must be bit-exact"
    te = vae.TextEncoder(tinyA)
    tf = te(prompts, cls_tok[target.long()])
    check(tf, g1["vae_text_features"], what="TextEncoder(prompts)")
    loss = vae.vae_loss(vae.l2_normalize(torch.from_numpy(g1["vae_text_features"]).to(d)), gf,
                        torch.from_numpy(g1["vae_mean"]).to(d), torch.from_numpy(g1["vae_log_var"]).to(d))
    assert abs(float(loss) - float(g1["vae_loss"])) <= 1e-4 * abs(float(g1["vae_loss"]))


# ------------------------------------------------------------------------------------------------
# ViT-B/16 (golden g2/g3/g5)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fullA():
    return build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).to(dev())


def test_vitb16_encode_image_vs_reference(fullA):
    """BASELINE config 1: 4 seeded 224x224 crops vs the reference's CPU fp32 output."""
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    img = torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev())
    out = fullA.encode_image(img)
    assert out.shape == (4, 512) and out.dtype == torch.float16       # model.dtype on GPU (clipnet/model.py:430)
    out32, trace = fullA.visual.forward_trace(img)
    e = check(out32, g["encode_image"], what="encode_image ViT-B/16")
    print(f"\nViT-B/16 encode_image rel-L2 vs reference: {e:.3e}")
    for i in range(12):
        check(trace[1 + i], g["cls_after_block"][i], what=f"CLS after block {i}")


def test_vitb16_variant_c_vs_reference():
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    sd = synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.VIT_B16, 1)))
    m = build_model(sd, use_adapter=True).to(dev())
    img = torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev())
    pri, mask = synth.priors(4, n=14, dim=64, n_pad=4, seed=99)
    gl, lo = m.visual(img, (torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev())))
    assert gl.shape == (4, 512) and lo.shape == (4, 512, 14, 14) and gl.dtype == torch.float32
    check(gl, g["c_prior_global"], what="C global")
    check(lo.permute(0, 2, 3, 1), np.transpose(g["c_prior_local"], (0, 2, 3, 1)), what="C local [B,512,14,14]")
    gl, lo = m.visual(img[:2], None)
    check(gl, g["c_noprior_global"], what="C global no prior")
    check(lo.permute(0, 2, 3, 1), np.transpose(g["c_noprior_local"], (0, 2, 3, 1)), what="C local no prior")


def test_vitb16_encode_text_600_prompts_vs_reference(fullA, g0):
    """BASELINE config 3: the 600 HICO prompts (+81 object, +117 verb prompts)."""
    g3 = dict(np.load(f"{G}/g3_vitb16_text.npz"))
    for name in ("hoi600", "obj81", "verb117"):
        ids = clip.tokenize(g0[name]["text"])
        assert torch.equal(ids, ids_from_g0(g0, name))
        for trunc in (True, False):
            fullA.truncate_text = trunc
            e = check(fullA.encode_text(ids.to(dev())).float(), g3[name], what=f"encode_text {name} trunc={trunc}")
        print(f"\nencode_text {name} rel-L2 vs reference: {e:.3e}")
    fullA.truncate_text = True


def test_vitb16_prompt_learner_text_encoder_vs_reference(g0):
    g5 = dict(np.load(f"{G}/g5_prompt_text.npz"))
    d = dev()
    # fp32 parameters as in the reference's CPU path that produced the fixture (clipnet/clip.py:135-136);
    # with fp16 parameters token_prefix/suffix would be fp16 as they are in the reference on GPU
    m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).float().to(d)
    pl = vae.PromptLearner_hoi(g0["_classnames"]["hoi"], m).float().to(d)
    assert pl.n_ctx == 5 and list(pl.name_lens) == g5["name_lens"].tolist()
    with torch.no_grad():
        pl.ctx.copy_(torch.from_numpy(synth.hg_normal((5, 512), 40, 0.02)))
    target = torch.from_numpy(g5["target"]).to(d)
    assert np.array_equal(pl.tokenized_prompts[target].cpu().numpy(), g5["tokenized_target"])
    prompts = pl(torch.from_numpy(g5["bias"]).to(d), target)
    assert prompts.shape == (32, 77, 512)
    assert np.allclose(prompts[0].cpu().numpy(), g5["prompts_row0"], rtol=0, atol=1e-7)
    te = vae.TextEncoder(m)
    check(te(prompts, pl.tokenized_prompts[target]), g5["text_features"], what="TextEncoder(PromptLearner_hoi)")
    plo = vae.PromptLearner_o(g0["_classnames"]["obj"], m).float().to(d)
    with torch.no_grad():
        plo.ctx.copy_(torch.from_numpy(synth.hg_normal((4, 512), 42, 0.02)))
    tgt_o = torch.from_numpy(g5["o_target"]).to(d)
    check(te(plo(torch.from_numpy(g5["bias"][:16]).to(d), tgt_o), plo.tokenized_prompts[tgt_o]), g5["o_text_features"],
          what="TextEncoder(PromptLearner_o)")


def test_vae_g4_vs_reference():
    g = dict(np.load(f"{G}/g4_vae.npz"))
    d = dev()
    E, Gn, M = vae.Encoder().to(d), vae.Generator().to(d), vae.mlp_net(512, 512, 512).to(d)
    E.load_state_dict(synth.to_torch(synth.encoder_state_dict(2)))
    Gn.load_state_dict(synth.to_torch(synth.generator_state_dict(3)))
    M.load_state_dict(synth.to_torch(synth.mlp_net_state_dict(4)))
    assert list(E.state_dict()) == ["net.0.weight", "net.0.bias", "mean.weight", "mean.bias", "log_var.weight", "log_var.bias"]
    assert list(Gn.state_dict()) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias"]
    x = vae.l2_normalize(torch.from_numpy(synth.hg_normal((160, 512), 30)).to(d))
    eps = torch.from_numpy(synth.hg_normal((160, 512), 31)).to(d)
    mean, lv, z, bias = vae.VAE(E, Gn)(x, eps)
    check(mean, g["mean"], what="mean"); check(lv, g["log_var"], what="log_var")
    check(z, g["z"], what="z"); check(bias, g["bias"], what="bias")
    recon = vae.l2_normalize(torch.from_numpy(synth.hg_normal((160, 512), 32)).to(d))
    loss = vae.vae_loss(recon, x, torch.from_numpy(g["mean"]).to(d), torch.from_numpy(g["log_var"]).to(d))
    assert abs(float(loss) - float(g["vae_loss"])) <= 1e-4 * abs(float(g["vae_loss"]))
    check(Gn(torch.from_numpy(synth.hg_normal((64, 512), 33)).to(d)), g["gen_from_z"], what="Generator(z)")
    f = vae.l2_normalize(torch.from_numpy(synth.hg_normal((64, 512), 34)).to(d))
    check(M(f), g["mlp_net"], what="mlp_net")


# ------------------------------------------------------------------------------------------------
# HIP path vs CPU oracle on other seeded inputs / ragged sizes
# ------------------------------------------------------------------------------------------------
def test_vitb16_vs_oracle_ragged_batch(fullA):
    from oracle import clip_oracle as co
    sd = co.reference_weight_rounding(synth.clip_state_dict(synth.VIT_B16, 0))
    img = torch.from_numpy(synth.crops(3, 224, seed=77) * 1.7 + 0.3)
    ref = co.encode_image(sd, img)
    check(fullA.visual.forward_trace(img.to(dev()))[0], ref.numpy(), what="B=3 vs oracle")
    out0 = fullA.encode_image(torch.empty(0, 3, 224, 224, device=dev()))
    assert out0.shape == (0, 512)


def test_vitb16_offset_residual_stream_vs_oracle(monkeypatch):
    """Rows of the residual stream with a large common offset (|mean| >> spread; here through ln_pre.bias and the
    class/positional embeddings) are the hard case of the LayerNorm-folded GEMMs: the fp16 copy is stored centred on
    the row's previous mean so that its rounding stays relative to the spread.  Both paths vs the oracle."""
    from oracle import clip_oracle as co
    raw = synth.clip_state_dict(synth.VIT_B16, 0)
    raw["visual.ln_pre.bias"] = (raw["visual.ln_pre.bias"] + 6.0).astype(np.float32)
    sd = co.reference_weight_rounding(raw)
    img = torch.from_numpy(synth.crops(3, 224, seed=78))
    ref = co.encode_image(sd, img).numpy()
    m = build_model(synth.to_torch(raw)).to(dev())
    for mode in (1, 0):
        m.set_option("ln_fuse", mode)
        e = check(m.visual.forward_trace(img.to(dev()))[0], ref, what=f"offset stream, ln_fuse={mode}")
        print(f"\noffset residual stream rel-L2 vs oracle, ln_fuse={mode}: {e:.3e}")


def test_vitb16_stress_outliers_vs_reference(g0, monkeypatch):
    """SURVEY.md §7 hard part / VERDICT r1 item 8: residual channels 50-100x the rest (from the first block and from
    the middle of the network) and c_fc pre-activations near 100, the way trained CLIP checkpoints behave.  Reference
    outputs: tests/golden/make_golden_stress.py (fixture g8).  Both LayerNorm arrangements of the vision tower, text
    with and without truncation."""
    g = dict(np.load(f"{G}/g8_stress.npz"))
    m = build_model(synth.to_torch(synth.stress_clip_state_dict(synth.VIT_B16, 0))).to(dev())
    img = torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev())
    for mode in (1, 0):
        m.set_option("ln_fuse", mode)
        out = m.visual.forward_trace(img)[0]
        e = check(out, g["encode_image"], what=f"stress encode_image ln_fuse={mode}")
        print(f"\nstress encode_image rel-L2 vs reference, ln_fuse={mode}: {e:.3e}")
    m.set_option("ln_fuse", 1)
    ids = ids_from_g0(g0, "hoi600", 64).to(dev())
    for trunc in (True, False):
        m.truncate_text = trunc
        e = check(m.encode_text(ids), g["encode_text"], what=f"stress encode_text truncate={trunc}")
        print(f"\nstress encode_text rel-L2 vs reference, truncate={trunc}: {e:.3e}")


def test_vae_vs_oracle_ragged_rows():
    from oracle import clip_oracle as co, vae_oracle as vo
    d = dev()
    se, sg = synth.encoder_state_dict(2), synth.generator_state_dict(3)
    E, Gn = vae.Encoder().to(d), vae.Generator().to(d)
    E.load_state_dict(synth.to_torch(se)); Gn.load_state_dict(synth.to_torch(sg))
    for R in (1, 129, 1000):
        x = co.l2_normalize(torch.from_numpy(synth.hg_normal((R, 512), 50 + R)))
        eps = torch.from_numpy(synth.hg_normal((R, 512), 60 + R))
        ref = vo.vae_forward(co.as_tensors(se), co.as_tensors(sg), x, eps)
        got = vae.VAE(E, Gn)(x.to(d), eps.to(d))
        for a, b, n in zip(got, ref, ("mean", "log_var", "z", "bias")):
            check(a, b.numpy(), what=f"{n} R={R}")


# ------------------------------------------------------------------------------------------------
# full-size properties (BASELINE config 2: batch 256)
# ------------------------------------------------------------------------------------------------
def test_batch256_invariance_and_determinism(fullA):
    d = dev()
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    torch.manual_seed(0)
    big = torch.randn(256, 3, 224, 224, device=d)
    golden4 = torch.from_numpy(synth.crops(4, 224, seed=1234)).to(d)
    big[100:104] = golden4                      # rows with a known reference answer inside the big batch
    out = fullA.visual.forward_trace(big)[0]
    assert torch.isfinite(out).all()
    check(out[100:104], g["encode_image"], what="golden crops inside a 256 batch")
    again = fullA.visual.forward_trace(big)[0]
    assert torch.equal(out, again), "same input, same launch sequence -> bit-identical output"
    sub = fullA.visual.forward_trace(big[96:160])[0]
    assert torch.equal(sub, out[96:160]), "rows are independent: a crop's embedding does not depend on its batch"
    # chunking (B > 256 is processed in chunks of 256) keeps rows identical
    out300 = fullA.visual.forward_trace(torch.cat([big, big[:44]]))[0]
    assert torch.equal(out300[:256], out) and torch.equal(out300[256:], out[:44])


def test_batch256_every_row_vs_oracle(fullA):
    """BASELINE config 2 at full size, every row compared: all 256 crops of a batch through the CPU oracle (oracle/clip_oracle.py, pinned
    to the reference's fixtures; ~15-30 s on the host cores) against the production path - every row of the last block computed (the
    headline's work) and the class rows only (the library's default) -, the one-launch MLP on and off.  Tolerance: relative L2 <= 1e-3
    for the whole matrix and for EVERY row (north_star); the worst row is printed."""
    from oracle import clip_oracle as co
    d = dev()
    gen = torch.Generator().manual_seed(2560)
    crops = torch.randn(256, 3, 224, 224, generator=gen)
    sd = co.reference_weight_rounding(synth.clip_state_dict(synth.VIT_B16, 0))
    with torch.no_grad():
        want = torch.cat([co.encode_image(sd, crops[i:i + 32]) for i in range(0, 256, 32)]).numpy()
    x = crops.to(d)
    try:
        for row0 in (0, 1):
            fullA.visual.set_option("last_block_row0", row0)
            for pair in (1, 0):
                fullA.visual.set_option("mlp_pair", pair)
                got = fullA.visual.forward_trace(x)[0]
                whole, worst = rel_l2(got, want)
                print(f"\nbatch 256 vs oracle, last_block_row0={row0} mlp_pair={pair}: rel-L2 {whole:.3e}, worst of 256 rows {worst:.3e}")
                assert whole <= TOL and worst <= TOL, (row0, pair, whole, worst)
    finally:
        fullA.visual.set_option("last_block_row0", 1)
        fullA.visual.set_option("mlp_pair", 1)


def test_activation_range_overflow_is_reported():
    """The LayerNorm-folded towers hold x - (row centre) as fp16 (the GEMM operand copy; with option stream_hilo the stream itself): a
    row that reaches further than 65 504 from its centre overflows it.  finalize_stats sees every row's statistics, which bound that
    reach: when the bound leaves the range a sticky flag makes the NEXT tower call fail (HG_ERR_INVALID -> RuntimeError) with an
    explanation - the overflowing call itself cannot be failed without a synchronisation; its rows come out non-finite.  A crop that
    comes in non-finite is NOT reported (NaN statistics compare false: the reference returns NaN for it too)."""
    d = dev()
    sd = synth.clip_state_dict(synth.VIT_B16, 0)
    for blk in (3, 4):      # (the weights themselves are fp16: 6e4 per block, 1.2e5 off the row's centre in one channel from block 4 on)
        key = f"visual.transformer.resblocks.{blk}.mlp.c_proj.bias"
        sd[key] = sd[key].copy()
        sd[key][5] = 6.0e4
    m = build_model(synth.to_torch(sd)).to(d)
    x = torch.from_numpy(synth.crops(4, 224, seed=77)).to(d).repeat(8, 1, 1, 1)      # 32 crops: M = 6304 >= 512, the folded path
    out = m.visual.forward_trace(x)[0]
    torch.cuda.synchronize()
    assert not torch.isfinite(out).all(), "the stress weights did not leave the fp16 range"
    with pytest.raises(RuntimeError, match="left the fp16 range inside a tower"):
        m.encode_image(x)
    # the report is consumed by the call that raised: a model in range runs on the same device right after
    # a NaN crop is the caller's business, not a range overflow: no report
    m2 = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).to(d)
    x2 = x.clone()
    x2[3, 0, 0, 0] = float("nan")
    o2 = m2.visual.forward_trace(x2)[0]
    torch.cuda.synchronize()
    assert not torch.isfinite(o2[3]).any() and torch.isfinite(o2[:3]).all() and torch.isfinite(o2[4:]).all()
    m2.encode_image(x)


def test_layernorm_folding_matches_separate_layernorm(fullA, g0, monkeypatch):
    """The vision tower folds LayerNorm into its GEMMs for M >= 512; option ln_fuse = 0 selects the separate-LayerNorm
    path.  Both must sit within the parity tolerance of the reference and of each other.  The switch reaches the text tower as well
    (it folds by default since round 5: option text_ln_fold): with ln_fuse = 0 it runs the separate kernels, the same bits as
    text_ln_fold = 0."""
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    img = torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev())
    ids = clip.tokenize(g0["obj81"]["text"]).to(dev())
    outs = {}
    try:
        for mode in (1, 0):
            fullA.set_option("ln_fuse", mode)
            outs[mode] = (fullA.visual.forward_trace(img)[0], fullA.encode_text(ids).float())
            e = check(outs[mode][0], g["encode_image"], what=f"encode_image ln_fuse={mode}")
            print(f"\nencode_image rel-L2 vs reference, ln_fuse={mode}: {e:.3e}")
    finally:
        fullA.set_option("ln_fuse", 1)
    assert not torch.equal(outs[1][0], outs[0][0]), "the switch did not change the executed path"
    check(outs[1][0], outs[0][0].cpu().numpy(), what="folded vs separate LayerNorm (image)")
    g3 = dict(np.load(f"{G}/g3_vitb16_text.npz"))
    for mode in (1, 0):
        check(outs[mode][1], g3["obj81"], what=f"encode_text ln_fuse={mode}")
    assert not torch.equal(outs[1][1], outs[0][1]), "ln_fuse = 0 did not reach the text tower"
    try:
        fullA.set_option("text_ln_fold", 0)
        assert torch.equal(fullA.encode_text(ids).float(), outs[0][1]), "ln_fuse = 0 and text_ln_fold = 0 are the same path"
    finally:
        fullA.set_option("text_ln_fold", 1)


def _stream_lo_bits(model) -> int:
    """How the library holds the low half of a hi / lo residual stream (read-only option stream_lo_bits): 8 (bf8)."""
    import ctypes
    from hoigen_amd import _lib
    v = ctypes.c_int32(0)
    assert _lib.lib().hg_get_option(model.visual._ctx.handle, b"stream_lo_bits", ctypes.byref(v)) == 0
    return v.value


def test_last_block_on_class_rows_only_matches_full_last_block(fullA, g0, monkeypatch):
    """encode_image returns ln_post(x[:, 0]) @ proj, so after K and V the last block only needs the class-token row of
    every crop; option last_block_row0 = 0 runs it on all 197 rows like the reference does.  Same result
    within the parity tolerance, both within it of the reference, and the per-block trace agrees."""
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    torch.manual_seed(5)
    img = torch.cat([torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev()), torch.randn(36, 3, 224, 224, device=dev())])
    outs = {}
    ids = clip.tokenize(g0["obj81"]["text"]).to(dev())
    txt = {}
    try:
        for mode in (1, 0):
            fullA.set_option("last_block_row0", mode)
            outs[mode] = fullA.visual.forward_trace(img)
            for trunc in (True, False):
                fullA.truncate_text = trunc
                txt[mode, trunc] = fullA.encode_text(ids).float()
            fullA.truncate_text = True
            e = check(outs[mode][0][:4], g["encode_image"], what=f"encode_image last_block_row0={mode}")
            print(f"\nencode_image rel-L2 vs reference, last_block_row0={mode}: {e:.3e}")
    finally:
        fullA.set_option("last_block_row0", 1)
    assert not torch.equal(outs[1][0], outs[0][0]), "the switch did not change the executed path"
    check(outs[1][0], outs[0][0].cpu().numpy(), what="class rows only vs full last block (embedding)")
    assert torch.equal(outs[1][1][:-2], outs[0][1][:-2]), "blocks before the last two are untouched"
    # the stream leaves its hi + lo form one residual GEMM earlier when the last block runs on the class rows:
    # after the second-to-last block the two arrangements hold the same rows to the bits the halves carry (fp16 + bf8: 13-14)
    assert _stream_lo_bits(fullA) == 8
    check(outs[1][1][-2], outs[0][1][-2].cpu().numpy(), tol=1e-4, what="class rows after the second-to-last block")
    check(outs[1][1][-1], outs[0][1][-1].cpu().numpy(), what="class rows after the last block")
    # the text tower (EOT rows): with its LayerNorms folded (the default) the two arrangements differ like the image tower's do - the last
    # block's rows take the separate kernels on the dense EOT rows, the folded GEMMs on all rows - and agree within the tolerance; with the
    # separate kernels throughout (text_ln_fold = 0) the 128x128 GEMM kernel of the dense rows accumulates in the same order as the ring
    # kernels: bit-identical
    for trunc in (True, False):
        check(txt[1, trunc], txt[0, trunc].cpu().numpy(), what=f"text tower, EOT rows only vs every row (truncate={trunc})")
    try:
        fullA.set_option("text_ln_fold", 0)
        sep = {}
        for mode in (1, 0):
            fullA.set_option("last_block_row0", mode)
            for trunc in (True, False):
                fullA.truncate_text = trunc
                sep[mode, trunc] = fullA.encode_text(ids).float()
        for trunc in (True, False):
            assert torch.equal(sep[1, trunc], sep[0, trunc]), f"text tower, separate LayerNorm, EOT rows only (truncate={trunc})"
    finally:
        fullA.set_option("text_ln_fold", 1)
        fullA.set_option("last_block_row0", 1)
        fullA.truncate_text = True


def test_text_truncation_is_exact_selection(fullA, g0):
    ids = ids_from_g0(g0, "coop_hoi600", 64).to(dev())
    fullA.truncate_text = True
    a = fullA.encode_text(ids).float()
    fullA.truncate_text = False
    b = fullA.encode_text(ids).float()
    fullA.truncate_text = True
    whole, worst = rel_l2(a, b.cpu().numpy())
    assert worst <= 2e-4, "running the causal tower on max(EOT)+1 positions must not change the EOT outputs"


def test_stale_truncation_is_clamped_and_reported(fullA, g0):
    """a truncation length below max(EOT)+1 (a stale host memo: the tokens were rewritten through an alias that
    bumps no version counter) must neither read out of bounds nor stay silent: EOT rows are clamped on the device, the stale
    call's whole output is NaN, the NEXT text call raises AND drops the memo, the one after works again - with no help from the
    test (the memo is poisoned directly, not monkeypatched back)."""
    import weakref
    toks = ids_from_g0(g0, "hoi600", 16).to(dev())
    good = fullA.encode_text(toks).float().cpu()
    true_len = int(toks.argmax(-1).max()) + 1
    fullA._trunc_memo = (weakref.ref(toks), toks._version, toks.data_ptr(), true_len - 2)      # a stale memo for this very tensor
    bad = fullA.encode_text(toks).float().cpu()              # no crash, no out-of-bounds read; loud: every value is NaN
    assert torch.isnan(bad).all()
    with pytest.raises(RuntimeError, match="trunc"):
        fullA.encode_text(toks)
    assert fullA._trunc_memo[0] is None                      # the failure dropped the stale memo
    again = fullA.encode_text(toks).float().cpu()
    assert torch.equal(again, good)
    # the embeds entry point shares the memo and the flag
    fullA._trunc_memo = (weakref.ref(toks), toks._version, toks.data_ptr(), true_len - 2)
    emb = fullA.token_embedding(toks).float()
    assert torch.isnan(fullA.encode_text_embeds(emb, toks)).all()
    with pytest.raises(RuntimeError, match="trunc"):
        fullA.encode_text_embeds(emb, toks)
    assert torch.isfinite(fullA.encode_text_embeds(emb, toks)).all()


def test_generation_pipeline_vs_oracle(g0):
    """z -> Generator -> PromptLearner -> TextEncoder -> L2 -> mlp_net, two branches in one
    text-tower pass, against the CPU oracle chain on the same latents."""
    from oracle import clip_oracle as co, vae_oracle as vo
    from hoigen_amd.generation import Branch, FeatureSampler
    d = dev()
    sd_np = synth.clip_state_dict(synth.VIT_B16, 0)
    m = build_model(synth.to_torch(sd_np)).float().to(d)
    sd = co.reference_weight_rounding(sd_np)
    names = {"hoi": g0["_classnames"]["hoi"], "obj": g0["_classnames"]["obj"]}
    cls = {"hoi": vae.PromptLearner_hoi, "obj": vae.PromptLearner_o}
    tgt = {"hoi": torch.tensor([(41 * i + 3) % 600 for i in range(12)]), "obj": torch.tensor([(9 * i + 1) % 80 for i in range(8)])}
    branches, ref = {}, {}
    for i, k in enumerate(("hoi", "obj")):
        gw, mw = synth.generator_state_dict(70 + i), synth.mlp_net_state_dict(80 + i)
        G_, M_ = vae.Generator().to(d), vae.mlp_net(512, 512, 512).to(d)
        G_.load_state_dict(synth.to_torch(gw)); M_.load_state_dict(synth.to_torch(mw))
        pl = cls[k](names[k], m).float().to(d)
        ctx = synth.hg_normal((pl.n_ctx, 512), 90 + i, 0.02)
        with torch.no_grad():
            pl.ctx.copy_(torch.from_numpy(ctx))
        branches[k] = Branch(G_, pl, M_, tgt[k])
        ref[k] = (co.as_tensors(gw), co.as_tensors(mw), torch.from_numpy(ctx), pl.tokenized_prompts.cpu(), pl.n_ctx)
    sampler = FeatureSampler(m, branches)
    z = {k: torch.from_numpy(synth.hg_normal((len(tgt[k]), 512), 95 + i)) for i, k in enumerate(("hoi", "obj"))}
    got = sampler.step({k: v.to(d) for k, v in z.items()})
    for k in ("hoi", "obj"):
        gw, mw, ctx, tok, n_ctx = ref[k]
        bias = vo.generator(gw, z[k])
        emb = sd["token_embedding.weight"][tok]
        prompts = vo.assemble_prompts(emb[:, :1], emb[:, 1 + n_ctx:], ctx, bias, tgt[k])
        t = co.l2_normalize(co.text_encoder_embeds(sd, prompts, tok[tgt[k]]))
        check(got[k], vo.mlp_net(mw, t).numpy(), what=f"generation pipeline branch {k}")
    feat, target = sampler.sample(iterations=2)
    assert feat.shape == (2 * 20, 512) and target.shape == (40,) and torch.isfinite(feat).all()
    assert torch.equal(target.cpu(), torch.cat([tgt["hoi"].repeat(2), tgt["obj"].repeat(2)]))


def test_eval_modules_work_with_grad_mode_on(fullA, g0):
    """the suite runs under an autouse torch.no_grad(); users of ``build_model(...).eval()`` call with grad mode ON.
    eval() modules (frozen or not) must pass the inference-only guard and give the same bits: image (fp32 and fp16 input),
    text, variant C with adapters in eval(), and directly constructed VAE-family modules after .eval()."""
    img = torch.from_numpy(synth.crops(2, 224, seed=1234)).to(dev())
    ids = ids_from_g0(g0, "hoi600", 8).to(dev())
    want_i, want_t = fullA.encode_image(img), fullA.encode_text(ids)
    sd_c = synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))
    sd_c.update(synth.to_torch(synth.adapter_state_dict(synth.VIT_B16, 1)))
    mc = build_model(sd_c, use_adapter=True).to(dev()).eval()
    pri, mask = synth.priors(2, n=14, dim=64, n_pad=4, seed=99)
    pri, mask = torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev())
    want_c = mc.visual(img, (pri, mask))
    E, Gn = vae.Encoder().to(dev()), vae.Generator().to(dev())
    x = vae.l2_normalize(torch.randn(16, 512, device=dev()))
    with torch.enable_grad():
        assert torch.is_grad_enabled()
        fullA.eval()
        assert torch.equal(fullA.encode_image(img), want_i)
        assert torch.equal(fullA.encode_image(img.half()), fullA.encode_image(img.half()))
        assert torch.equal(fullA.encode_text(ids), want_t)
        got_c = mc.visual(img, (pri, mask))
        assert all(torch.equal(a, b) for a, b in zip(got_c, want_c))
        with pytest.raises(RuntimeError, match="train\\(\\) mode"):
            E(x)                                      # a freshly constructed module is in train() mode with trainable weights
        E.eval(); Gn.eval()
        mean, logvar = E(x)
        assert torch.isfinite(mean).all() and not mean.requires_grad
        assert torch.isfinite(Gn(mean)).all()


def test_residual_stream_as_centre_hi_lo_matches_fp32_stream(fullA):
    """Option stream_hilo (default on): between the LayerNorm-folded blocks of variant A the residual stream
    lives as centre + hi + lo (the fp16 copy + its remainder as bf8, 13-14 bits of x - centre)
    instead of fp32.  Both arrangements sit within the parity
    tolerance of the reference; against each other the embeddings and the per-block class-token trace differ by rounding noise
    only; with the class-rows-only last block and with every row."""  # noqa: D400
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    torch.manual_seed(11)
    img = torch.cat([torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev()), torch.randn(20, 3, 224, 224, device=dev())])
    fullA.visual.forward_trace(img[:1])      # (creates the native context)
    assert _stream_lo_bits(fullA) == 8
    try:
        for row0 in (1, 0):
            fullA.set_option("last_block_row0", row0)
            outs = {}
            for mode in (1, 0):
                fullA.set_option("stream_hilo", mode)
                outs[mode] = fullA.visual.forward_trace(img)
                e = check(outs[mode][0][:4], g["encode_image"], what=f"encode_image stream_hilo={mode} row0={row0}")
                print(f"\nencode_image rel-L2 vs reference, stream_hilo={mode}, last_block_row0={row0}: {e:.3e}")
            assert not torch.equal(outs[1][1], outs[0][1]), "the switch did not change the executed path"
            # (a 1e-7 difference in the stream flips fp16 roundings of the operand copies downstream: the two arrangements are two
            # realisations of the same fp16 rounding noise, each 3e-4 from the reference - against each other they sit at that level too)
            check(outs[1][0], outs[0][0].cpu().numpy(), what="hi/lo stream vs fp32 stream (embedding)")
            # early blocks: before the roundings decorrelate the stream itself agrees to the bits the halves carry
            check(outs[1][1][1], outs[0][1][1].cpu().numpy(), tol=1e-4, what="class rows after block 1, hi/lo vs fp32 stream")
            check(outs[1][1], outs[0][1].cpu().numpy(), what="class-token trace, hi/lo vs fp32 stream")
    finally:
        fullA.set_option("stream_hilo", 1)
        fullA.set_option("last_block_row0", 1)


def test_non_finite_crop_does_not_poison_its_neighbours(fullA):
    """Rows are independent in the reference (clipnet/model.py:219-236: nothing mixes crops), also for non-finite data.  The fused
    in_proj + attention kernel computes 208-row tiles of a 197-token sequence: the 11 pad rows of V are the NEXT crop's first rows
    (or workspace rows an earlier, larger call left behind); their keys are masked, but 0 * NaN in P V is NaN - they are stored as
    zeros (review of round 4).  (a) one NaN crop inside a batch leaves every other crop finite and unchanged; (b) a clean batch of 40
    after a batch of 256 whose crop 40 was NaN is clean."""
    d = dev()
    torch.manual_seed(5)
    big = torch.randn(256, 3, 224, 224, device=d)
    clean = fullA.visual.forward_trace(big)[0]
    bad = big.clone()
    bad[40] = float("nan")
    out = fullA.visual.forward_trace(bad)[0]
    finite = torch.isfinite(out).all(dim=1)
    assert not finite[40], "the NaN crop itself must not come out finite"
    keep = torch.ones(256, dtype=torch.bool, device=d)
    keep[40] = False
    assert finite[keep].all(), f"crops {(~finite & keep).nonzero().flatten().tolist()} were poisoned by crop 40"
    assert torch.equal(out[keep], clean[keep])
    small = fullA.visual.forward_trace(big[:40])[0]        # the workspace rows behind row 40 * 197 still hold the NaN crop's activations
    assert torch.isfinite(small).all()
    assert torch.equal(small, clean[:40])


def test_set_option_rejects_out_of_range_values(fullA):
    """include/hoigen_amd.h: unknown keys and out-of-range values return HG_ERR_INVALID (the façade raises and does not record them)."""
    fullA.visual.forward_trace(torch.zeros(1, 3, 224, 224, device=dev()))      # (creates the native context)
    before = dict(fullA.visual._ctx.options)
    for key, val in (("qkv_attn", 3), ("qkv_attn", -1), ("qkv_attn_min_seq", 0), ("qkv_attn_gsz", 7), ("mlp_pair", 2), ("mlp_fused", 1),
                     ("no_such_option", 1)):
        with pytest.raises(RuntimeError):
            fullA.visual.set_option(key, val)
    assert fullA.visual._ctx.options == before


def test_small_scale_residual_stream_vs_oracle():
    """The hi / lo residual stream holds x as centre + fp16 + bf8 with NO per-row scale: a stream whose rows spread by 0.02 (here:
    ln_pre.weight x 0.02 and small block outputs) puts the fp16 remainder at ~1e-5 - below e5m2's normal range unless the low half is
    stored scaled (HG_LO_SCALE, hg_kernels.h).  40 crops (the fused in_proj + attention kernel and the hi / lo stream both engage)
    against the oracle, both stream arrangements, every row of the last block."""
    from oracle import clip_oracle as co
    raw = synth.clip_state_dict(synth.VIT_B16, 0)
    raw["visual.ln_pre.weight"] = (raw["visual.ln_pre.weight"] * 0.02).astype(np.float32)
    raw["visual.ln_pre.bias"] = (raw["visual.ln_pre.bias"] * 0.02).astype(np.float32)
    for i in range(12):      # keep the block updates at the stream's scale: otherwise the first residual add restores a spread of ~1
        for k in ("attn.out_proj", "mlp.c_proj"):
            raw[f"visual.transformer.resblocks.{i}.{k}.weight"] = (raw[f"visual.transformer.resblocks.{i}.{k}.weight"] * 0.02).astype(np.float32)
            raw[f"visual.transformer.resblocks.{i}.{k}.bias"] = (raw[f"visual.transformer.resblocks.{i}.{k}.bias"] * 0.02).astype(np.float32)
    sd = co.reference_weight_rounding(raw)
    img = torch.from_numpy(synth.crops(40, 224, seed=79))
    ref = co.encode_image(sd, img[:6]).numpy()
    m = build_model(synth.to_torch(raw)).to(dev())
    m.visual.forward_trace(img[:1].to(dev()))
    m.set_option("last_block_row0", 0)
    for mode in (1, 0):
        m.set_option("stream_hilo", mode)
        out = m.visual.forward_trace(img.to(dev()))[0]
        e = check(out[:6], ref, what=f"small-scale stream, stream_hilo={mode}")
        print(f"\nsmall-scale residual stream rel-L2 vs oracle, stream_hilo={mode}: {e:.3e}")


def test_variant_c_on_the_hi_lo_stream_vs_reference():
    """Round 5: with every block's adapter folded into its GEMMs (the default) variant C holds the residual stream as centre + hi + lo
    between the residual GEMMs like variant A does (option stream_hilo; the hi half lives in the in_proj operand buffer [x16 | e],
    attention writes into a second operand buffer [att | e], the decoder writes e into both).  Against the reference's own variant C
    outputs (g2: with priors and without) on both settings, the settings against each other, 40 crops (the chunk is batch-independent)."""
    g = dict(np.load(f"{G}/g2_vitb16_image.npz"))
    sd = synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.VIT_B16, 1)))
    m = build_model(sd, use_adapter=True).to(dev())
    torch.manual_seed(3)
    img = torch.cat([torch.from_numpy(synth.crops(4, 224, seed=1234)).to(dev()), torch.randn(36, 3, 224, 224, device=dev())])
    pri, mask = synth.priors(4, n=14, dim=64, n_pad=4, seed=99)
    pri40 = torch.cat([torch.from_numpy(pri).to(dev()), torch.randn(36, 14, 64, device=dev())])
    mask40 = torch.cat([torch.from_numpy(mask).to(dev()), torch.zeros(36, 14, dtype=torch.bool, device=dev())])
    outs = {}
    try:
        for mode in (1, 0):
            m.visual.set_option("stream_hilo", mode)
            gl, lo = m.visual(img, (pri40, mask40))
            e1 = check(gl[:4], g["c_prior_global"], what=f"C global, stream_hilo={mode}")
            e2 = check(lo[:4].permute(0, 2, 3, 1), np.transpose(g["c_prior_local"], (0, 2, 3, 1)), what=f"C local, stream_hilo={mode}")
            gn, ln_ = m.visual(img[:2], None)
            check(gn, g["c_noprior_global"], what=f"C global no prior, stream_hilo={mode}")
            check(ln_.permute(0, 2, 3, 1), np.transpose(g["c_noprior_local"], (0, 2, 3, 1)), what=f"C local no prior, stream_hilo={mode}")
            print(f"\nvariant C rel-L2 vs reference, stream_hilo={mode}: global {e1:.3e} local {e2:.3e}")
            outs[mode] = (gl, lo)
    finally:
        m.visual.set_option("stream_hilo", 1)
    assert not torch.equal(outs[1][0], outs[0][0]), "the switch did not change the executed path"
    check(outs[1][0], outs[0][0].cpu().numpy(), what="variant C hi / lo stream vs fp32 stream (global)")


def test_variant_c_in_proj_and_attention_as_one_kernel_is_bit_identical():
    """Variant C's blocks sum in_proj over [x16 | e] (D + 64 = 832 columns): the fused in_proj + attention kernel's second instance
    (13 K-tiles) runs them by default (option qkv_attn_c); switching it off gives the K = 832 GEMM and the attention kernel - the same
    bits, with priors and without, and the launches of the step really change."""
    from hoigen_amd import _lib
    sd = synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.VIT_B16, 1)))
    m = build_model(sd, use_adapter=True).to(dev())
    torch.manual_seed(4)
    img = torch.randn(40, 3, 224, 224, device=dev())
    pri = torch.randn(40, 14, 64, device=dev())
    mask = torch.zeros(40, 14, dtype=torch.bool, device=dev())
    mask[::3, 9:] = True
    outs, fused_launches = {}, {}
    try:
        for mode in (1, 0):
            m.visual.set_option("qkv_attn_c", mode)
            m.visual(img, (pri, mask))      # (weights folded and packed outside the profiled call)
            (gl, lo), recs = _lib.profile(m.visual._ctx.handle, _lib.HG_PROF_ALL, 512, lambda: m.visual(img, (pri, mask)))
            gn, ln_ = m.visual(img, None)
            outs[mode] = (gl, lo, gn, ln_)
            fused_launches[mode] = sum(1 for r in recs if r[0] == _lib.HG_PROF_QKV_ATTN)
    finally:
        m.visual.set_option("qkv_attn_c", 1)
    assert fused_launches[1] == 12 and fused_launches[0] == 0, fused_launches
    for a, b in zip(outs[1], outs[0]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_variant_c_non_finite_crop_does_not_poison_its_neighbours():
    """The same row independence on the detector's call (variant C: adapters folded into the GEMMs, hi / lo stream, in_proj + attention
    as one kernel over D + 64 columns, CLIP_models_adapter_prior2.py:489-506 mixes no crops either): one NaN crop (image and priors) in
    a batch of 64 leaves the others finite and bit-equal to the clean run; a clean batch of 40 behind it is clean."""
    d = dev()
    sd = synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.VIT_B16, 1)))
    m = build_model(sd, use_adapter=True).to(d)
    torch.manual_seed(6)
    img = torch.randn(64, 3, 224, 224, device=d)
    pri = torch.randn(64, 14, 64, device=d)
    mask = torch.zeros(64, 14, dtype=torch.bool, device=d)
    mask[:, 11:] = True
    clean_g, clean_l = m.visual(img, (pri, mask))
    bad_i, bad_p = img.clone(), pri.clone()
    bad_i[40] = float("nan")
    bad_p[40] = float("nan")
    g, l = m.visual(bad_i, (bad_p, mask))
    keep = torch.ones(64, dtype=torch.bool, device=d)
    keep[40] = False
    assert not torch.isfinite(g[40]).all(), "the NaN crop itself must not come out finite"
    assert torch.isfinite(g[keep]).all() and torch.isfinite(l[keep]).all(), "a NaN crop leaked into its neighbours"
    assert torch.equal(g[keep], clean_g[keep]) and torch.equal(l[keep], clean_l[keep])
    g2, l2 = m.visual(img[:40], (pri[:40], mask[:40]))      # workspace rows behind crop 39 still hold the NaN crop's activations
    assert torch.isfinite(g2).all() and torch.isfinite(l2).all()
    assert torch.equal(g2, clean_g[:40]) and torch.equal(l2, clean_l[:40])


def test_text_tower_with_folded_layernorm_vs_reference(fullA, g0):
    """Option text_ln_fold: how the text tower's LayerNorms reach its GEMMs.  1 (default since round 5): folded, the LayerNorm weight
    multiplied into the ACTIVATION copy the residual GEMM hands on (GemmArgs::gamma), so that in_proj / c_fc run on the layer's own fp16
    weights as the reference does - 6.2e-4 against its outputs (worst prompt of the 600 + 81 + 117 sets 7.5e-4); 0: the separate
    kernels (6.5e-4, worst 7.9e-4); 2: the weight folded into fp16(W * gamma) like the vision tower's - the fastest and, through that
    second rounding of the weights, the least close (7.6e-4, worst 9.6e-4: tests/test_gpu_text_fold_study.py).  All three against the
    reference on every prompt; the settings really differ; truncation keeps each setting's bits; the default comes back."""
    g3 = dict(np.load(f"{G}/g3_vitb16_text.npz"))
    ids = {n: clip.tokenize(g0[n]["text"]).to(dev()) for n in ("hoi600", "obj81", "verb117")}
    outs, errs = {}, {}
    try:
        for mode in (1, 0, 2):
            fullA.set_option("text_ln_fold", mode)
            for name in ("hoi600", "obj81", "verb117"):
                fullA.truncate_text = False
                full = fullA.encode_text(ids[name]).float()
                errs[mode, name] = check(full, g3[name], what=f"encode_text {name}, text_ln_fold={mode}")
                fullA.truncate_text = True
                assert torch.equal(fullA.encode_text(ids[name]).float(), full), f"truncation changed the rows (text_ln_fold={mode})"
                if name == "hoi600":
                    outs[mode] = full
            print(f"\nencode_text rel-L2 vs reference, text_ln_fold={mode}: " + ", ".join(f"{n} {errs[mode, n]:.3e}" for n in ids))
    finally:
        fullA.set_option("text_ln_fold", 1)
        fullA.truncate_text = False
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[2])
    assert all(errs[1, n] < errs[2, n] for n in ids), "the activation-side fold must be closer to the reference than the weight-side one"
    assert torch.equal(fullA.encode_text(ids["hoi600"]).float(), outs[1])
    fullA.truncate_text = True


def test_feature_sampler_with_folded_text_layernorm(fullA, g0):
    """FeatureSampler(text_ln_fold=2) runs the HICO loop with that setting of the library option for the duration of sample() and puts
    the default back: same latents -> features within the tolerance of the default path's, default again afterwards."""
    from hoigen_amd.generation import hico_sampler
    s = hico_sampler(fullA, g0["_classnames"])
    gen = torch.Generator(device=dev()).manual_seed(11)
    base, tgt = s.sample(iterations=2, generator=gen, batch_iters=2)
    s.text_ln_fold = 2
    gen = torch.Generator(device=dev()).manual_seed(11)
    fold, tgt2 = s.sample(iterations=2, generator=gen, batch_iters=2)
    assert torch.equal(tgt, tgt2) and base.shape == (2 * 1800, 512)
    assert not torch.equal(base, fold), "the flag did not change the executed path"
    # (two realisations of the fp16 roundings of 12 blocks + mlp_net, each within 1e-3 of the reference's: 9.2e-4 apart, worst row 1.3e-3)
    check(fold, base.cpu().numpy(), tol=2e-3, what="generated features, folded text LayerNorm vs default")
    s.text_ln_fold = None
    gen = torch.Generator(device=dev()).manual_seed(11)
    again, _ = s.sample(iterations=2, generator=gen, batch_iters=2)
    assert torch.equal(again, base), "the default path did not come back"

