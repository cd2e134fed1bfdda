"""Host side of hoigen_amd.interaction (no GPU): the façade's permutation, pair counts and per-image output lists against the torch
expressions of the reference (upt_tip_cache_model_free_finetune_distill3.py:988-1023, :1000-1003, :1245-1249), its refusals, and the
C ABI of hg_hoi_head (symbol, struct layout against the header)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hoi_head_bound as hb
from hoigen_amd import _lib, interaction

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUMAN = 1


def reference_image(boxes, scores, labels, num_classes):
    """the reference's statements for one image -> (boxes, scores, labels permuted, x_keep, y_keep, union boxes) or None when skipped"""
    is_human = labels == HUMAN
    n_h = torch.sum(is_human); n = len(boxes)
    if not torch.all(labels[:n_h] == HUMAN):
        h_idx = torch.nonzero(is_human).squeeze(1)
        o_idx = torch.nonzero(is_human == 0).squeeze(1)
        perm = torch.cat([h_idx, o_idx])
        boxes = boxes[perm]; scores = scores[perm]
        labels = labels[perm]
    if n_h == 0 or n <= 1:
        return None
    x, y = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    x_keep, y_keep = torch.nonzero(torch.logical_and(x != y, x < n_h)).unbind(1)
    lt = torch.min(boxes[x_keep][..., :2], boxes[y_keep][..., :2])
    rb_ = torch.max(boxes[x_keep][..., 2:], boxes[y_keep][..., 2:])
    return boxes, scores, labels, x_keep, y_keep, torch.cat([lt, rb_], dim=-1)


def props():
    g = torch.Generator().manual_seed(11)
    out = []
    for labels in ([3, 1, 5, 1, 2], [1], [4, 6, 2], [1, 1, 1], [], [7, 1]):      # mixed order, n = 1, no human, humans only, empty, human last
        n = len(labels)
        xy = torch.rand(n, 2, generator=g) * 150
        out.append({"boxes": torch.cat([xy, xy + 10 + 60 * torch.rand(n, 2, generator=g)], 1), "scores": torch.rand(n, generator=g),
                    "labels": torch.tensor(labels, dtype=torch.int64)})
    return out


def test_plan_and_output_lists_match_the_reference_expressions():
    rp, NC = props(), 24
    perm, box_off, n_human, pair_off = interaction.plan_batch([p["labels"] for p in rp], HUMAN)
    assert box_off == [0, 5, 6, 9, 12, 12, 14] and n_human == [2, 1, 0, 3, 0, 1]
    assert list(np.diff(pair_off)) == [8, 0, 0, 6, 0, 1]
    boxes = torch.cat([p["boxes"][q] for p, q in zip(rp, perm)])
    labels = torch.cat([p["labels"][q] for p, q in zip(rp, perm)])
    # the batch arrays as the kernels' restatement gives them, through split_outputs
    pr = hb.batch_pairs(boxes.numpy(), labels.numpy().astype(np.int32), box_off, n_human)
    Pt = pair_off[-1]
    logits, prior = torch.arange(Pt * NC, dtype=torch.float32).reshape(Pt, NC), torch.rand(2, Pt, NC)
    lg, pri, bh, bo, obj = interaction.split_outputs(pair_off, logits, prior, torch.from_numpy(pr["pair_h"]), torch.from_numpy(pr["pair_o"]),
                                                     torch.from_numpy(pr["objects"]), torch.int64)
    assert len(lg) == len(pri) == len(bh) == len(bo) == len(obj) == len(rp)
    for b, p in enumerate(rp):
        ref = reference_image(p["boxes"], p["scores"], p["labels"], NC)
        lo, hi = pair_off[b], pair_off[b + 1]
        if ref is None:
            zero = torch.zeros(0, dtype=torch.int64)
            for t in (bh[b], bo[b], obj[b]):
                assert t.dtype == zero.dtype and t.shape == zero.shape
            assert pri[b].shape == torch.zeros(2, 0, NC).shape and lg[b].shape == (0, NC)
            continue
        bx, sc, lb, xk, yk, ub = ref
        assert torch.equal(bx, boxes[box_off[b]:box_off[b + 1]]) and torch.equal(lb, labels[box_off[b]:box_off[b + 1]])
        assert torch.equal(bh[b], xk) and torch.equal(bo[b], yk) and bh[b].dtype == xk.dtype
        assert torch.equal(obj[b], lb[yk]) and obj[b].dtype == lb.dtype
        assert torch.equal(torch.from_numpy(pr["union_boxes"][lo:hi]), ub)
        assert torch.equal(lg[b], logits[lo:hi]) and torch.equal(pri[b], prior[:, lo:hi]) and pri[b].shape == (2, hi - lo, NC)


def test_target_table():
    t = interaction.target_table([[0, 3], [], [2]], 4)
    assert t.dtype == torch.uint8 and t.tolist() == [[1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]]
    assert torch.equal(interaction.target_table(t.float() * 3, 4), t)
    with pytest.raises(ValueError):
        interaction.target_table(torch.zeros(3, 5), 4)


def test_refusals_without_a_device():
    head = interaction.HOIHead([], [[0], [1]], HUMAN, 2)
    rp = props()[:1]
    f = torch.zeros(1, 64, 14, 14)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(None, f, torch.tensor([[224, 224]]), rp)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference only"):
            head(None, f.clone().requires_grad_(True), torch.tensor([[224, 224]]), rp)
    with pytest.raises(RuntimeError, match="HOIHead call returned"):
        head.postprocess([], [], [], [torch.zeros(0, 2)], [], [], [])
    with pytest.raises(ValueError):
        interaction.HOIHead([("nowhere", None, 1.0)], [[0]], HUMAN, 2)
    with pytest.raises(TypeError):
        interaction.HOIHead([("union", object(), 1.0)], [[0]], HUMAN, 2)
    with pytest.raises(ValueError):
        interaction.HOIHead([("union", None, 1.0)] * 7, [[0]], HUMAN, 2)


def test_abi_symbol_and_struct_layout():
    src = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    assert re.search(r"int hg_hoi_head\(hg_ctx\*, const hg_hoi_head_args\* args, void\* stream\);", src)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hg_hoi_head") and "hg_hoi_head" in _lib.SIGNATURES
    bodies = dict((n, re.sub(r"/\*.*?\*/", "", b, flags=re.S)) for b, n in re.findall(r"typedef struct \{([^}]*)\} (\w+);", src))

    def n_fields(name):
        return sum(len(d.split(",")) for d in re.findall(r"[\w\s\*]+?\s\**([^;]+);", bodies[name]))

    assert n_fields("hg_hoi_branch") == 3 == len(_lib.hg_hoi_branch._fields_)
    assert n_fields("hg_hoi_head_args") == 30 == len(_lib.hg_hoi_head_args._fields_)
    assert int(re.search(r"#define HG_HOI_MAX_BRANCH (\d+)", src).group(1)) == _lib.HG_HOI_MAX_BRANCH
    for name, v in _lib.HG_HOI_SRC.items():
        assert int(re.search(rf"#define HG_HOI_SRC_{name.upper()} (\d+)", src).group(1)) == v
    assert ctypes.sizeof(_lib.hg_hoi_branch) == 12
    # 7 pointers, 5 + 1 + 1 words, 6 branches, pointer (8-aligned), 3 words (+ pad), 11 pointers
    assert ctypes.sizeof(_lib.hg_hoi_head_args) == 7 * 8 + 7 * 4 + 6 * 12 + 4 + 8 + 3 * 4 + 4 + 11 * 8
    assert _lib.hg_hoi_head_args.obj2target.offset == 160 and _lib.hg_hoi_head_args.pair_h.offset == 184


def test_the_build_does_not_fuse_the_kernels_operations():
    """hg_hoi_head.hip with build.sh's own flags: in the set-up and the pooling kernel the only fused multiply-adds are the five of
    each correctly rounded division (the restatement in tests/hoi_head_bound.py has one rounding per operation); the one fmaf of
    hoi_feats_kernel is l2_normalize_kernel's"""
    import shutil
    import subprocess
    import tempfile

    from asm_blocks import kernel_body

    csrc = os.path.join(REPO, "hoigen_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    script = open(os.path.join(csrc, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    extra = re.search(r'\[ \$f = hg_hoi_head \] && X="([^"]*)"', script)
    assert extra and "$HIPCC $FLAGS $X -c" in script and "hg_hoi_head" in script.split("for f in")[1].split(";")[0]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "hg_hoi_head.s")
        r = subprocess.run([hipcc] + flags + extra.group(1).split() + ["-S", "--cuda-device-only", os.path.join(csrc, "hg_hoi_head.hip"), "-o", out],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        txt = open(out).read()
    for kernel in ("hoi_setup_kernel", "hoi_pool_kernel"):
        body = kernel_body(txt, re.search(r"^(_ZN2hg\d+%s\w*):" % kernel, txt, re.M).group(1))
        fused = len(re.findall(r"\bv_(?:fma|fmac|pk_fma)_f32", body))
        divisions = len(re.findall(r"\bv_div_fixup_f32", body))
        assert divisions > 0 and fused == 5 * divisions, (kernel, fused, divisions)
        assert "scratch_" not in body, f"{kernel} spills or indexes private memory"
