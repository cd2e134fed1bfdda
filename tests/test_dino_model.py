"""CPU proof of what tests/test_gpu_resnet_features.py and tests/test_gpu_hoi_dino_branch.py ask (tests/dino_bound.py): the fp32
restatement of the pool stays within the derived bound of the float64 mean on every committed case and the exact family comes out bit
for bit; the normalised rows stay within elem_bound's bound; every mutant is rejected by a rule on the committed cases; the façade
refuses what it does not implement without a device; and build_dino_cache_model makes build_clip_cache_model's draws."""
import numpy as np
import pytest
import torch
from torch import nn

import dino_bound as db
import heads_bound as hdb
import hoi_head_bound as hb
import resnet_cases as rc
from hoigen_amd import cache_model
from hoigen_amd.resnet import ResNetFeatures

NC = 24


@pytest.mark.parametrize("shape", db.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_within_the_bounds(shape):
    B, HW, C = shape
    top = [0.0, 0.0]
    for fam in db.FAMILIES:
        x = db.make_map(fam, B, HW, C)
        p = db.pool_model(x)
        sp = db.special_image(fam, B)
        rows = [b for b in range(B) if not (fam == "nan_image" and b == sp)]
        norm_rows = [b for b in range(B) if b != sp or fam not in ("zero_image", "nan_image")]
        if rows:
            top[0] = max(top[0], db.worst_pool(p[rows], x[rows]))
        if norm_rows:
            top[1] = max(top[1], db.worst_norm(db.normalize_model(p), p, norm_rows))
        if db.is_exact(fam, HW):
            assert np.array_equal(p.astype(np.float64), x.astype(np.float64).mean(1))
        if fam == "zero_image":
            assert np.isnan(db.normalize_model(p)[sp]).all()
    print(f"\nDINO_RATIO restatement {shape}: pooled {top[0]:.3f}, features {top[1]:.3f}")
    assert top[0] <= 1.0 and top[1] <= 1.0
    assert any(db.is_exact("ints", s[1]) for s in db.SHAPES)


@pytest.mark.parametrize("mutant", db.POOL_MUTANTS)
def test_pool_mutants_rejected(mutant):
    rejected = []
    for shape in db.SHAPES:
        x = db.make_map("relu", *shape)
        if db.worst_pool(db.pool_model(x, mutant), x) > 1.0:
            rejected.append(shape)
    assert rejected, f"{mutant} passes the float64 rule on every case"
    if mutant == "channel_seam_skipped":
        assert rejected == [s for s in db.SHAPES if s[2] > db.CH_STRIDE], "only the cases wider than the workgroup have a seam"
    if mutant in ("last_position_dropped", "mean_over_hw_plus_1"):
        assert rejected == list(db.SHAPES)


@pytest.mark.parametrize("mutant", db.NORM_MUTANTS)
def test_norm_mutants_rejected(mutant):
    for shape in db.SHAPES:
        p = db.pool_model(db.make_map("relu", *shape))
        assert db.worst_norm(db.normalize_model(p, mutant), p) > 1.0, shape


def _head_case(sizes, humans, at, seed=9):
    b = hb.make_batch(list(sizes), list(humans), 14, 14, 64, 224, seed=seed, num_classes=NC)
    pr = hb.batch_pairs(b["boxes"], b["labels"], b["box_off"], b["n_human"])
    g = np.random.default_rng(seed)
    Pt = len(pr["pair_h"])
    rows = [g.standard_normal((b["B"] if i == at else Pt, NC)).astype(np.float32) for i in range(6)]
    gx, gy = b["box_off"][pr["image"]] + pr["pair_h"], b["box_off"][pr["image"]] + pr["pair_o"]
    args = (rows, [i == at for i in range(6)], [0.5, 1.0, 2.0, 0.7, 0.3, 0.6], pr["image"], b["scores"][gx], b["scores"][gy], b["labels"][gx],
            b["labels"][gy], b["obj2target"], 2.8)
    return args


@pytest.mark.parametrize("mutant", [m for m in db.HEAD_MUTANTS if m != "image_bias_dropped"])
def test_head_mutants_rejected(mutant):
    """the rule: logits bit for bit"""
    for sizes, humans in (((3, 1, 0, 5), (2, 1, 0, 0)), ((4, 3, 2), (2, 1, 1))):
        args = _head_case(sizes, humans, at=5)
        want = db.head(*args)[0]
        got = db.head(*args, mutant=mutant)[0]
        assert want.shape == got.shape and not np.array_equal(want, got), (mutant, sizes)
    # the image branch's place in the list does not matter to the mutant that moves it first - when it IS first
    args = _head_case((4, 3, 2), (2, 1, 1), at=0)
    assert np.array_equal(db.head(*args)[0], db.head(*args, mutant="image_branch_summed_first")[0])


def test_image_bias_dropped_rejected():
    """the rule: image_logits within heads_bound's float64 bound (bias -1 on five samples)"""
    g = torch.Generator().manual_seed(3)
    f, w = torch.randn(4, 64, generator=g), torch.randn(5, 64, generator=g)
    f, w = f / f.norm(dim=1, keepdim=True), w / w.norm(dim=1, keepdim=True)
    lab = (torch.rand(5, NC, generator=g) < 0.4).float()
    c = db.image_case(f, w, -torch.ones(5), lab, lab.sum(0).clamp_min(1.0))
    want, E = hdb.cache_reference(c)
    assert hdb.worst(torch.from_numpy(db.image_logits_model(c)).double(), want, E) <= 1.0
    assert hdb.worst(torch.from_numpy(db.image_logits_model(c, "image_bias_dropped")).double(), want, E) > 1.0


# ---- the facade, without a device -----------------------------------------------------------------------------------------------------
def _net():
    net = rc.small_resnet()
    net.avgpool, net.fc = nn.AdaptiveAvgPool2d((1, 1)), nn.Identity()
    return net


def test_facade_reads_the_network_and_refuses_without_a_device():
    m = ResNetFeatures.from_module(_net())
    assert m.num_channels == 512 and not m.training and m.stem._ctx is m.stages._ctx
    bare = rc.small_resnet()      # no avgpool, no fc
    assert ResNetFeatures.from_module(bare).num_channels == 512
    net = _net()
    net.fc = nn.Linear(512, 10)
    with pytest.raises(RuntimeError, match="fc is a Linear 512 -> 10"):
        ResNetFeatures.from_module(net)
    net = _net()
    net.avgpool = nn.AvgPool2d(7)
    with pytest.raises(RuntimeError, match="avgpool is AvgPool2d"):
        ResNetFeatures.from_module(net)
    net = _net()
    net.avgpool = nn.AdaptiveAvgPool2d((2, 2))
    with pytest.raises(RuntimeError, match="only nn.AdaptiveAvgPool2d to 1 x 1"):
        ResNetFeatures.from_module(net)
    net = rc.make_resnet((2, 2, 1, 2), (64, 128, 64, 128), (1, 2, 2, 2), norm=nn.BatchNorm2d)
    net.avgpool, net.fc = nn.AdaptiveAvgPool2d((1, 1)), nn.Identity()
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):
        ResNetFeatures.from_module(net)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            m(torch.zeros(1, 3, 32, 32))
    with torch.enable_grad(), pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 32, 32, requires_grad=True))


def test_pool_workgroup_width_is_one_number():
    """the channel stride of the seam mutant is the kernel's workgroup width: hg_kernels.h, its mirror in _lib.py and dino_bound agree"""
    import os
    import re

    from hoigen_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hoigen_amd", "csrc", "hg_kernels.h")).read()
    assert int(re.search(r"RESNET_POOL_THREADS = (\d+);", src).group(1)) == _lib.HG_RESNET_POOL_THREADS == db.CH_STRIDE


def test_build_dino_cache_model_on_raw_rows():
    """raw (unnormalised) rows in, the selected keys normalised at the end, every selected key one of the rows.  (Equality with the
    reference's keys and values under one seed is tests/test_dino_branch_golden.py's; the two builders share one body, so comparing
    them here only pins that they stay one.)"""
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(20, 64, generator=g) * 7.0 + 1.0
    verbs = [[int(v) for v in torch.randperm(6, generator=g)[: 1 + i % 3]] for i in range(20)]      # class 6 and 7 stay empty
    torch.manual_seed(11)
    keys, values = cache_model.build_dino_cache_model(feats, verbs, 8, 2)
    torch.manual_seed(11)
    k2, v2 = cache_model.build_clip_cache_model(feats, verbs, 8, 2)
    assert torch.equal(keys, k2) and torch.equal(values, v2)
    assert keys.shape == (64, 16) and values.shape == (16, 8)
    assert torch.allclose(keys.norm(dim=0), torch.ones(16), atol=1e-6)
    sel = keys.t()[:12] @ (feats / feats.norm(dim=1, keepdim=True)).t()      # every selected key is one of the rows, normalised
    assert torch.allclose(sel.max(1).values, torch.ones(12), atol=1e-5)
