"""ViT-L/14@336px with instance adapters in front of every block (the detector's call visual(x, (priors, mask)), 577 tokens per image) on
the host: the CPU oracle against the reference's own outputs (tests/golden/g13_vitl14_336_adapter.npz, make_golden_vitl_adapter.py).
What shows, without a GPU, that fixture and oracle agree.  CPU only.

Tolerance: the project's oracle tolerance, rel-L2 <= 1e-4 for the whole matrix and for every row (measured 6e-7 global, 8e-7 local:
an fp32 restatement of the fp32 reference, reduction order apart)."""
import os

import numpy as np
import pytest
import torch

from hoigen_amd import synth
from oracle import clip_oracle as co

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = synth.VIT_L14_336
TOL = 1e-4


def rel_l2(a, b):
    a, b = a.detach().numpy().astype(np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    return np.linalg.norm(a - b) / np.linalg.norm(b), (np.linalg.norm(a2 - b2, axis=1) / np.linalg.norm(b2, axis=1)).max()


def close(a, b, what):
    whole, worst = rel_l2(a, b)
    print(f"\n{what}: rel-L2 {whole:.2e}, worst row {worst:.2e}")
    assert whole <= TOL and worst <= TOL, (what, whole, worst)


@pytest.fixture(scope="module")
def sd():
    raw = synth.clip_state_dict(CFG, 0)
    raw.update(synth.adapter_state_dict(CFG, 1))
    return co.as_tensors(raw)                                # variant C: no fp16 rounding of the weights


@pytest.fixture(scope="module")
def g13():
    return dict(np.load(f"{G}/g13_vitl14_336_adapter.npz"))


def parts(gl, lo, g13):
    at = torch.stack([lo[:, :, y, x] for y, x in g13["c_local_pos"].tolist()], dim=1)
    return gl, at, lo.double().sum(dim=(1, 2, 3)).numpy()


@pytest.mark.parametrize("memory", ["prior", "self"])
def test_oracle_with_adapters_vs_reference(sd, g13, memory):
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    img = torch.from_numpy(synth.crops(2, 336, seed=1234))
    if memory == "prior":
        pri, mask = synth.priors(2, n=14, dim=64, n_pad=4, seed=99)
        prior = (torch.from_numpy(pri), torch.from_numpy(mask))
    else:
        img, prior = img[:1], None
    gl, lo = co.visual_with_prior(sd, img, prior, adapter_layers=range(CFG["vision_layers"]))
    assert gl.shape == (len(img), 768) and lo.shape == (len(img), 768, 24, 24)
    gl, at, s = parts(gl, lo, g13)
    close(gl, g13[f"c_{memory}_global"], f"variant C with adapters ({memory} memory): global")
    close(at, g13[f"c_{memory}_local_at"], f"variant C with adapters ({memory} memory): local map, 768-channel rows at 64 positions")
    ref = g13[f"c_{memory}_local_sum"]
    print(f"local map sums {s} vs {ref}")
    assert (np.abs(s - ref) <= TOL * np.abs(ref)).all(), (s, ref)


def test_the_adapters_matter(g13):
    """with and without priors the global row of crop 0 differs by 0.46 relative: a path that skips the adapters (or takes the wrong
    memory) cannot pass the 1e-3 of tests/test_gpu_vitl336_adapter.py"""
    a, b = g13["c_prior_global"][0].astype(np.float64), g13["c_self_global"][0].astype(np.float64)
    d = np.linalg.norm(a - b) / np.linalg.norm(a)
    print(f"\nglobal row of crop 0, priors against self memory: {d:.3f}")
    assert d > 0.1
    g12 = np.load(f"{G}/g12_vitl14_336.npz")["c_noprior_global"][0].astype(np.float64)
    assert np.linalg.norm(b - g12) / np.linalg.norm(g12) > 0.1, "self-memory adapters give what no adapters give"
