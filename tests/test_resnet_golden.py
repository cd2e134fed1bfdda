"""The fixture tests/golden/g22_resnet_stages.npz (made by tests/golden/make_golden_resnet.py from F.conv2d and the reference's own
FrozenBatchNorm2d.forward in fp32: one two-block stage with stride 2 and a downsample, 64 -> 256 channels, 2 x 64 x 9 x 7) against the
float64 statement and the fp16 / fp32 restatement of tests/resnet_bound.py on the CPU - this pins both to the reference's norm - and
against the native path on the device: relative L2 of every block inside the 1e-3 contract; every element of the first block inside the
bound plus four times the fixture's own fp32-against-fp64 distance; every element of the second block inside the bound of the float64
statement from the block input the run itself returned (a worst-case bound carried through two blocks is a hundred times the values
and would hold nothing)."""
import os

import numpy as np
import pytest
import torch

import resnet_bound as rb
import resnet_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    g = np.load(os.path.join(GOLDEN, "g22_resnet_stages.npz"))
    stage, _ = rc.g22_stage()
    keys = set(stage.state_dict())
    missing, unexpected = stage.load_state_dict({k: torch.from_numpy(g[k]) for k in g.files if k in keys}, strict=True)
    assert not missing and not unexpected
    return g, stage, torch.from_numpy(g["x"])


def statements(stage, x):
    """the float64 statement of every block from the fixture's input"""
    refs, v = [], x
    for blk in stage.layer1:
        refs.append(rb.block_reference(blk, v, None if v is x else torch.zeros_like(v)))
        v = refs[-1]["want"]
    return refs


def judge(tag, stage, g, refs, outs, x):
    """outs: every block's fp32 output of a run from x"""
    for i, blk in enumerate(stage.layer1):
        got, want = outs[i].double(), torch.from_numpy(g[f"out{i}"]).double()
        slack = 4 * float(g[f"out{i}_fp32_vs_fp64_max_abs"])
        rel = float((got - want).norm() / want.norm())
        if i == 0:
            worst = float(((got - want).abs() / (refs[0]["b32"] + slack)).max())
        else:
            own = rb.block_reference(blk, outs[i - 1])
            worst = float(((got - own["want"]).abs() / own["b32"]).max())
        print(f"RESNET g22 block {i} {tag}: rel L2 {rel:.2e}, worst |err| / bound {worst:.3f}" + (f" (bound + 4 x {slack / 4:.1e})" if i == 0 else
              " (from the block input the run returned)"))
        assert rel < 1e-3 and worst <= 1.0


def test_the_fixture_is_the_seeded_recipe_and_small():
    g, stage, x = fixture()
    fresh, x2 = rc.g22_stage()
    assert torch.equal(x, x2) and all(torch.equal(v, fresh.state_dict()[k]) for k, v in stage.state_dict().items())
    size = os.path.getsize(os.path.join(GOLDEN, "g22_resnet_stages.npz"))
    assert size <= max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "g22_resnet_stages.npz") and size < 1 << 20
    assert tuple(g["out0"].shape) == tuple(g["out1"].shape) == (2, 256, 5, 4)


def test_the_restatements_against_the_references_fp32_run():
    g, stage, x = fixture()
    refs = statements(stage, x)
    outs, t = [], x
    for i, blk in enumerate(stage.layer1):
        d64 = float((refs[i]["want"] - torch.from_numpy(g[f"out{i}"]).double()).abs().max())
        own = float(g[f"out{i}_fp32_vs_fp64_max_abs"])
        print(f"RESNET g22 block {i}: float64 statement against the reference's fp32 run max abs {d64:.2e} (its own fp32-against-fp64 distance {own:.1e})")
        assert d64 <= 1.5 * own + 1e-9, "the float64 statement is not the reference's arithmetic"
        out32, out16 = rb.block_model(blk, t)
        assert torch.equal(out16, out32.half().float())
        outs.append(out32)
        t = out32
    judge("restatement", stage, g, refs, outs, x)


@pytest.mark.gpu
def test_the_native_path_against_the_fixture():
    from hoigen_amd.resnet import ResNetStages
    g, stage, x = fixture()
    refs = statements(stage, x)
    m = ResNetStages.from_module(stage, levels=(1, 1)).cuda()
    out, trace = m.forward_trace(x.cuda())
    assert torch.equal(out, trace[-1])
    judge("native", stage, g, refs, [t.cpu() for t in trace], x)
