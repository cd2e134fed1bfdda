"""The detector's call visual(x, (priors, mask)) on towers of more than 224 tokens per image, with instance adapters in front of every
block (option adapter_long = 1; hoigen_amd/csrc/hg_adapter_long.hip):

* CLIP ViT-L/14@336px (577 tokens) against the reference's own outputs (tests/golden/g13_vitl14_336_adapter.npz), with priors and with
  the sequence as the adapters' memory: rel-L2 <= 1e-3 for every tensor and for every stored row - the project's parity contract;
* a tiny tower of 257 tokens (patch 2 on 32 x 32 pixels) against the fp32 oracle, and a call longer than one pass of the tower (223
  crops at this length) against its two part-calls, bit for bit: priors and mask are offset per pass.

Measured values are printed (`-s`)."""
import os

import numpy as np
import pytest
import torch

from hoigen_amd import synth
from hoigen_amd.model import build_model
from oracle import clip_oracle as co

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rel_l2(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().cpu().numpy().astype(np.float64) if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all(), "non-finite values in the HIP output"
    whole = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    rows = np.linalg.norm(a2 - b2, axis=1) / np.maximum(np.linalg.norm(b2, axis=1), 1e-30)
    return whole, rows.max()


def check(a, b, what):
    whole, worst = rel_l2(a, b)
    print(f"\n{what}: rel-L2 {whole:.3e}, worst row {worst:.3e}")
    assert whole <= TOL and worst <= TOL, f"{what}: rel-L2 {whole:.3e}, worst row {worst:.3e} > {TOL}"


@pytest.fixture(scope="module")
def vitl():
    raw = synth.clip_state_dict(synth.VIT_L14_336, 0)
    raw.update(synth.adapter_state_dict(synth.VIT_L14_336, 1))
    m = build_model(synth.to_torch(raw), use_adapter=True).to(dev())
    m.visual.set_option("adapter_long", 1)       # before the first call: options are applied when the context is created, before the load
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("memory", ["prior", "self"])
def test_vitl14_336_with_adapters_vs_reference(vitl, memory):
    g13 = np.load(f"{G}/g13_vitl14_336_adapter.npz")
    x = torch.from_numpy(synth.crops(2, 336, seed=1234)).to(dev())
    if memory == "prior":
        pri, mask = synth.priors(2, n=14, dim=64, n_pad=4, seed=99)
        gl, lo = vitl.visual(x, (torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev())))
    else:
        gl, lo = vitl.visual(x[:1], None)
    assert gl.shape[1:] == (768,) and lo.shape[1:] == (768, 24, 24)
    check(gl, g13[f"c_{memory}_global"], f"ViT-L/14@336px with adapters ({memory} memory): global vs reference")
    at = torch.stack([lo[:, :, y, x_] for y, x_ in g13["c_local_pos"].tolist()], dim=1)
    check(at, g13[f"c_{memory}_local_at"], f"ViT-L/14@336px with adapters ({memory} memory): local map, 768-channel rows at 64 positions")


@pytest.mark.parametrize("memory", ["prior", "self"])
def test_vitl14_336_with_adapters_local_map_sum_vs_reference(vitl, memory):
    """The third quantity g13 stores: the fp64 sums of the whole [768,24,24] local maps, as one tensor per call, rel-L2 <= 1e-3.

    The sum cancels 270-fold here (1 304.7 against a sum of magnitudes of about 357 000; 174-fold without adapters,
    tests/test_gpu_vitl336.py) and weighs whatever is common to a channel's 576 tokens 576 times - which is what the fp16 rounding of
    a weight column times the mean of the GEMM's operand is; the reference keeps variant C's weights in fp32.  With every weight in
    fp16 the HIP path measured 1.5e-3 with the sequence as memory (4.7e-4 with priors, the second crop alone 1.2e-3).  The CPU oracle
    in fp32 with one group of weights rounded to fp16 at a time says where it comes from (self memory / priors' second crop): c_proj
    1.1e-3 / 4.9e-4, up_proj 5.1e-4 / 6.2e-4, down_proj 3.5e-4 / 1e-5, in_proj 3.0e-4 / 1.1e-4, c_fc 2.6e-4 / 2.6e-4, out_proj
    2.0e-4 / 1.3e-4 - the two GEMMs that write the stream from an operand whose mean is far from zero (QuickGELU's output; the
    decoder's LayerNorm output with its bias).  Calls with adapters on such a tower therefore run c_proj and up_proj as hi + lo
    (hg_load_vit), as visual.proj already is there.  Measured on an MI355X with that: 1.2e-4 with priors (the two crops 8e-5 and
    2.8e-4 of their own sums), 1.0e-4 with the sequence as memory."""
    g13 = np.load(f"{G}/g13_vitl14_336_adapter.npz")
    x = torch.from_numpy(synth.crops(2, 336, seed=1234)).to(dev())
    if memory == "prior":
        pri, mask = synth.priors(2, n=14, dim=64, n_pad=4, seed=99)
        _, lo = vitl.visual(x, (torch.from_numpy(pri).to(dev()), torch.from_numpy(mask).to(dev())))
    else:
        _, lo = vitl.visual(x[:1], None)
    s, ref = lo.double().sum(dim=(1, 2, 3)).cpu().numpy(), g13[f"c_{memory}_local_sum"]
    print(f"\nlocal map sums {s} vs reference {ref}: relative {np.abs(s - ref) / np.abs(ref)}")
    check(s[None], ref[None], f"ViT-L/14@336px with adapters ({memory} memory): the local maps' sums")


def test_the_option_taken_back_refuses_the_loaded_tower(vitl):
    x = torch.zeros(1, 3, 336, 336, device=dev())
    vitl.visual(x, None)
    vitl.visual.set_option("adapter_long", 0)
    try:
        with pytest.raises(RuntimeError, match="at most 224 tokens.*adapter_long = 1"):
            vitl.visual(x, None)
    finally:
        vitl.visual.set_option("adapter_long", 1)
    assert torch.isfinite(vitl.visual(x, None)[0]).all()


CFG257 = dict(synth.TINY, vision_patch_size=2, image_resolution=32)      # 16 x 16 patches + the class token = 257 tokens
CHUNK257 = 256 * 224 // 257                                              # crops per pass at this length (hg_tower.hip: image_chunk) = 223


@pytest.fixture(scope="module")
def tiny257():
    raw = synth.clip_state_dict(CFG257, 4)
    raw.update(synth.adapter_state_dict(CFG257, 5))
    m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").float().to(dev())
    assert m.visual.get_option("adapter_long") == 0
    m.visual.set_option("adapter_long", 1)
    B = CHUNK257 + 7
    x = torch.from_numpy(synth.crops(B, 32, seed=21))
    pri, mask = synth.priors(B, n=14, dim=64, n_pad=4, seed=22)
    return m, co.as_tensors(raw), x, torch.from_numpy(pri), torch.from_numpy(mask)


def test_tiny_tower_of_257_tokens_vs_oracle(tiny257):
    m, sd, x, pri, mask = tiny257
    layers = range(CFG257["vision_layers"])
    for prior in (None, (pri[:4], mask[:4])):
        want_g, want_l = co.visual_with_prior(sd, x[:4], prior, adapter_layers=layers)
        got_g, got_l = m.visual(x[:4].to(dev()), None if prior is None else (prior[0].to(dev()), prior[1].to(dev())))
        tag = f"tiny tower, 257 tokens, {'priors' if prior else 'no prior'}"
        check(got_g, want_g, tag + ": global")
        check(got_l.permute(0, 2, 3, 1), want_l.permute(0, 2, 3, 1), tag + ": local")
        none_g, _ = co.visual_with_prior(sd, x[:4], prior, adapter_layers=())
        assert rel_l2(want_g, none_g)[0] > 10 * TOL, "the adapters do not matter here: the check above would not see them skipped"


def test_a_call_longer_than_one_pass_equals_its_parts(tiny257):
    m, _, x, pri, mask = tiny257
    x, pri, mask = x.to(dev()), pri.to(dev()), mask.to(dev())
    assert not torch.equal(pri[:7], pri[CHUNK257:]) and mask.any()
    c = CHUNK257
    whole = m.visual(x, (pri, mask))
    first = m.visual(x[:c], (pri[:c], mask[:c]))
    second = m.visual(x[c:], (pri[c:], mask[c:]))
    for k, name in enumerate(("global", "local")):
        assert torch.isfinite(whole[k]).all()
        assert torch.equal(whole[k][:c], first[k]), f"{name}: the first pass differs from the call of its crops"
        assert torch.equal(whole[k][c:], second[k]), f"{name}: the second pass differs from the call of its crops (priors / mask offset)"
    wrong = m.visual(x[c:], (pri[:7], mask[:7]))
    assert not torch.equal(wrong[0], second[0]), "the priors do not reach the output: the comparison above shows nothing"


def test_update_adapters_follows_the_option():
    """A 257-token tower loaded without adapters whose adapter weights arrive later (hg_update_adapters): refused with the option at 0,
    the words as ever plus the hint; accepted at 1, with the bits of a tower loaded with them."""
    raw = synth.clip_state_dict(CFG257, 4)
    raw.update(synth.adapter_state_dict(CFG257, 5))
    m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").float().to(dev())
    blocks = list(m.visual.transformer.resblocks)
    x = torch.from_numpy(synth.crops(2, 32, seed=1)).to(dev())
    for b in blocks:                      # first load: as a tower without adapters
        b.adapter = False
    plain = m.visual(x, None)[0].clone()
    for b in blocks:                      # now the adapter tensors "change": the façade sends them through hg_update_adapters
        b.adapter = True
    scale = next(p for n, p in m.visual.named_parameters() if n.endswith("adaptermlp.scale"))
    scale.mul_(1.0)
    scale.add_(0.0)
    with pytest.raises(RuntimeError, match="hg_update_adapters.*at most 224 tokens.*adapter_long = 1"):
        m.visual(x, None)
    m.visual.set_option("adapter_long", 1)
    got = m.visual(x, None)[0]
    assert not torch.equal(got, plain)
    fresh = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all").float().to(dev())
    fresh.visual.set_option("adapter_long", 1)
    assert torch.equal(got, fresh.visual(x, None)[0])
