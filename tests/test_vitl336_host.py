"""ViT-L/14@336px on the host: the CPU oracle against the reference's own outputs (tests/golden/g12_vitl14_336*.npz) - what shows,
without a GPU, that fixture and oracle agree - and the shape inference of the façade.  CPU only.

Tolerance: the oracle is an fp32 restatement of the fp32 reference; the two differ by reduction order only (measured 5e-7 for the
image tower, 1e-6 for the text tower, 24 blocks deep): rel-L2 <= 1e-5 for the whole matrix and for every row."""
import json
import os

import numpy as np
import pytest
import torch

from hoigen_amd import clip, synth
from hoigen_amd.model import _infer_config, build_model
from oracle import clip_oracle as co

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = synth.VIT_L14_336
TOL = 1e-5


def rel_l2(a, b):
    a = a.detach().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    whole = np.linalg.norm(a - b) / np.linalg.norm(b)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return whole, (np.linalg.norm(a2 - b2, axis=1) / np.linalg.norm(b2, axis=1)).max()


def close(a, b, what):
    whole, worst = rel_l2(a, b)
    print(f"\n{what}: rel-L2 {whole:.2e}, worst row {worst:.2e}")
    assert whole <= TOL and worst <= TOL, (what, whole, worst)


@pytest.fixture(scope="module")
def raw():
    return synth.clip_state_dict(CFG, 0)


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(f"{G}/g12_vitl14_336.npz"))


def test_oracle_image_tower_vs_reference(raw, g12):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    sd = co.reference_weight_rounding(raw)
    img = torch.from_numpy(synth.crops(4, 336, seed=1234))
    col = []
    out = co.encode_image(sd, img, collect=col)
    assert out.shape == (4, 768) and len(col) == 25 and col[0].shape == (4, 577, 1024)
    close(out, g12["encode_image"], "encode_image")
    close(torch.stack([c[:, 0, :] for c in col[1:]]), g12["cls_after_block"], "class row after every block")
    close(col[-1][0][torch.from_numpy(g12["tok_rows"])], g12["tok_after_block23_img0"], "64 token rows of image 0 after block 23")


def test_oracle_text_tower_vs_reference(raw):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    sd = co.reference_weight_rounding(raw)
    g0 = json.load(open(f"{G}/g0_tokens.json"))
    want = np.load(f"{G}/g12_vitl14_336_text.npz")["verb117_obj81"]
    rows = g0["verb117"]["ids"] + g0["obj81"]["ids"]
    ids = np.zeros((len(rows), 77), np.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    assert want.shape == (198, 768)
    out = torch.cat([co.encode_text(sd, torch.from_numpy(ids[i:i + 66])) for i in range(0, 198, 66)])
    close(out, want, "encode_text of the 117 verb + 81 object prompts")


def test_oracle_variant_c_without_adapters_vs_reference(raw, g12):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    sd = co.as_tensors(raw)                                  # variant C: no fp16 rounding of the weights
    img = torch.from_numpy(synth.crops(4, 336, seed=1234))[:2]
    gl, lo = co.visual_with_prior(sd, img, None, ())
    assert gl.shape == (2, 768) and lo.shape == (2, 768, 24, 24)
    close(gl, g12["c_noprior_global"], "variant C global")
    at = torch.stack([lo[:, :, y, x] for y, x in g12["c_local_pos"].tolist()], dim=1)                  # [2,64,768]: whole rows
    close(at, g12["c_noprior_local_at"], "variant C local map, 768-channel rows at 64 positions")
    s, ref = lo.double().sum(dim=(1, 2, 3)).numpy(), g12["c_noprior_local_sum"]
    print(f"local map sums {s} vs {ref}")
    assert (np.abs(s - ref) <= TOL * np.abs(ref)).all(), (s, ref)


def test_build_model_infers_the_large_shape(raw):
    cfg = _infer_config(synth.to_torch(raw))
    assert cfg == CFG
    m = build_model(synth.to_torch(raw))
    v = m.visual
    assert (v.patch_size, v.input_resolution, v.output_dim) == (14, 336, 768)
    assert (v.transformer.layers, v.transformer.width, v.transformer.heads) == (24, 1024, 16)
    assert v.positional_embedding.shape == (577, 1024) and v.conv1.weight.shape == (1024, 3, 14, 14)
    assert (m.transformer.layers, m.transformer.width, m.transformer.heads) == (12, 768, 12)
    assert m.text_projection.shape == (768, 768) and m.context_length == 77
    assert v.conv1.weight.dtype == torch.float16      # variant A: weights held as fp16, as the reference's build_model leaves them
    mc = build_model(synth.to_torch(raw), use_adapter=False)
    assert mc.visual.returns_local and not any(getattr(b, "adapter", False) for b in mc.visual.transformer.resblocks)


def test_synthetic_state_dict_has_the_references_key_set(raw):
    want = json.load(open(f"{G}/g12_vitl14_336_keys.json"))
    assert set(raw) == set(want), (sorted(set(raw) ^ set(want)))
    for k, shape in want.items():
        assert list(raw[k].shape) == shape, (k, raw[k].shape, shape)
    assert abs(sum(int(v.size) for v in raw.values()) - 427.9e6) < 0.1e6      # 427.9 M parameters


def test_transform_at_336():
    from PIL import Image
    t = clip._transform(336)
    img = Image.fromarray((np.random.default_rng(0).random((400, 520, 3)) * 255).astype(np.uint8))
    out = t(img)
    assert out.shape == (3, 336, 336) and out.dtype == torch.float32
