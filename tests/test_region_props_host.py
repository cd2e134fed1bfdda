"""Host side of hoigen_amd.proposals (no GPU): the façade's list shapes and dtypes, its error paths, the C ABI of hg_load_priors /
hg_region_priors (symbols, struct layout against the header), and that the build keeps the kernels' operations unfused."""
import ctypes
import os
import re

import pytest
import torch

from hoigen_amd import _lib, interaction, proposals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_region_props_shapes_and_dtypes():
    B, cap = 3, 8
    counts = [[3, 1, 0, 5], [0, 0, 0, 0], [8, 4, 0, 9]]
    boxes, scores = torch.arange(B * cap * 4, dtype=torch.float32).reshape(B, cap, 4), torch.rand(B, cap)
    labels = torch.arange(B * cap, dtype=torch.int32).reshape(B, cap)
    for dt in (torch.int64, torch.int32):
        rp = proposals.split_region_props(counts, boxes, scores, labels, dt)
        assert [len(p["scores"]) for p in rp] == [3, 0, 8] and [p["n_human"] for p in rp] == [1, 0, 4]
        for b, p in enumerate(rp):
            n = counts[b][0]
            assert p["boxes"].shape == (n, 4) and p["scores"].shape == (n,) and p["labels"].shape == (n,) and p["labels"].dtype == dt
            assert torch.equal(p["boxes"], boxes[b, :n]) and torch.equal(p["labels"], labels[b, :n].to(dt))


def test_plan_from_counts_is_plan_batch_on_humans_first_lists():
    labels = [torch.tensor([1, 1, 3, 5]), torch.tensor([1]), torch.tensor([4, 2]), torch.zeros(0, dtype=torch.int64), torch.tensor([1, 1])]
    want = interaction.plan_batch(labels, 1)
    got = interaction.plan_from_counts([len(lb) for lb in labels], want[2])
    assert got[1:] == want[1:] and all(torch.equal(a, b) for a, b in zip(got[0], want[0]))


def test_host_sizes():
    assert proposals.host_sizes(torch.tensor([[480, 640], [333, 500]]), 2) == [480.0, 640.0, 333.0, 500.0]
    assert proposals.host_sizes([(480, 640)], 1) == [480.0, 640.0]
    with pytest.raises(ValueError, match="image_sizes"):
        proposals.host_sizes(torch.zeros(3, 2), 2)


def test_refusals_without_a_device():
    with pytest.raises(ValueError, match="max_instances"):
        proposals.RegionProposals(0, max_instances=33)
    with pytest.raises(ValueError, match="min_instances"):
        proposals.RegionProposals(0, min_instances=5, max_instances=4)
    assert proposals.RegionProposals(0).cap == 30
    mlp = torch.nn.Module()
    mlp.layers = torch.nn.ModuleList(torch.nn.Linear(i, o) for i, o in ((517, 128), (128, 128), (128, 64)))
    emb = torch.zeros(81, 512)
    free = list(proposals._free)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        proposals.InstancePriors(mlp, emb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        proposals.InstancePriors(mlp.state_dict(), emb)
    with pytest.raises(ValueError, match=r"E \+ 5"):
        proposals.InstancePriors(mlp, torch.zeros(81, 768))
    with pytest.raises(ValueError, match="layers.0"):
        proposals.InstancePriors({"weight": torch.zeros(1)}, emb)
    mlp.layers.append(torch.nn.Linear(64, 64))
    with pytest.raises(ValueError, match="exactly three"):
        proposals.InstancePriors(mlp, emb)
    assert proposals._free == free      # a failed construction gives its slot back
    with pytest.raises(TypeError):
        proposals.DetectorFrontEnd(object())
    with pytest.raises(TypeError):
        proposals.DetectorFrontEnd(proposals.RegionProposals(0), object())
    front = proposals.DetectorFrontEnd(proposals.RegionProposals(0))
    assert front([], []) == ([], None)
    res = [dict(scores=torch.rand(4), labels=torch.zeros(4, dtype=torch.int64), boxes=torch.rand(4, 4))]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        front(res, [(10, 10)])
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference only"):
            front([dict(res[0], scores=torch.rand(4, requires_grad=True))], [(10, 10)])


def test_abi_symbols_and_struct_layout():
    src = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    assert re.search(r"int hg_load_priors\(hg_ctx\*, int slot, const hg_prior_weights\* w\);", src)
    assert re.search(r"int hg_region_priors\(hg_ctx\*, const hg_region_priors_args\* args, void\* stream\);", src)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "hg_load_priors") and hasattr(lib, "hg_region_priors")
    bodies = dict((n, re.sub(r"/\*.*?\*/", "", b, flags=re.S)) for b, n in re.findall(r"typedef struct \{([^}]*)\} (\w+);", src))

    def n_fields(name):
        return sum(len(d.split(",")) for d in re.findall(r"[\w\s\*]+?\s\**([^;]+);", bodies[name]))

    assert n_fields("hg_prior_weights") == 11 == len(_lib.hg_prior_weights._fields_)
    assert n_fields("hg_region_priors_args") == 21 == len(_lib.hg_region_priors_args._fields_)
    assert int(re.search(r"#define HG_MAX_PRIOR_SLOTS (\d+)", src).group(1)) == _lib.HG_MAX_PRIOR_SLOTS
    assert ctypes.sizeof(_lib.hg_prior_weights) == 4 * 4 + 7 * 16
    # 5 pointers, B + 2 floats + 4 words (+ pad), 9 pointers
    assert ctypes.sizeof(_lib.hg_region_priors_args) == 5 * 8 + 7 * 4 + 4 + 9 * 8
    assert _lib.hg_region_priors_args.counts.offset == 72 and _lib.hg_region_priors_args.table_out.offset == 136


def test_the_build_does_not_fuse_the_kernels_operations():
    """hg_region_props.hip with build.sh's own flags: the only fused multiply-adds are the five of each correctly rounded division
    (the IoU; the four box columns of a prior row) - tests/props_bound.py has one rounding per operation - and no kernel uses scratch"""
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
    extra = re.search(r'\[ \$f = hg_region_props \] && X="([^"]*)"', script)
    assert extra and "hg_region_props" in script.split("for f in")[1].split(";")[0]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "hg_region_props.s")
        r = subprocess.run([hipcc] + flags + extra.group(1).split() + ["-S", "--cuda-device-only", os.path.join(csrc, "hg_region_props.hip"), "-o", out],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        txt = open(out).read()
    for kernel, min_div in (("props_select_kernel", 1), ("prior_mlp_kernel", 4), ("prior_table_kernel", 0)):
        body = kernel_body(txt, re.search(r"^(_ZN2hg\d+%s\w*):" % kernel, txt, re.M).group(1))
        fused = len(re.findall(r"\bv_(?:fma|fmac|pk_fma)_f32", body))
        divisions = len(re.findall(r"\bv_div_fixup_f32", body))
        assert divisions >= min_div and fused == 5 * divisions, (kernel, fused, divisions)
        assert "scratch_" not in body, f"{kernel} spills or indexes private memory"
