"""hg_detr_attn.hip and hg_detr_rows.hip as the product build compiles them - build.sh's own flags for gfx950 - cross-compiled, no GPU
needed: the compiler's resource-usage remarks show every kernel without a spill and without scratch, within the VGPR / SGPR figures of
DESIGN.md section 16's table, and the attention kernel's dynamic LDS within a compute unit's 160 KiB.  Nothing else is inspected."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# DESIGN.md section 16's table: VGPR / SGPR / LDS bytes at most (the attention kernel's LDS is dynamic: 128 B a key of the chunk)
FIGURES = {"hg_detr_attn": {"detr_attn_kernel": (64, 48, 163840)},
           "hg_detr_rows": {"detr_entry_kernel": (24, 40, 0), "detr_postnorm_kernel": (40, 32, 0), "detr_exit_kernel": (32, 32, 0)}}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(FIGURES))
def test_no_spill_no_scratch_within_the_design_table(src):
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    assert re.search(rf"\b{src}\b", script), "the source is in build.sh's list"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src + ".hip"), "-o",
                            os.path.join(tmp, src + ".o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = FIGURES[src]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in kernels if k in m.group(1)), None)
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert set(usage) == set(kernels), usage
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    hdr = open(os.path.join(CSRC, "hg_kernels.h")).read()
    for k, (vgpr, sgpr, lds) in kernels.items():
        u = usage[k]
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] <= vgpr and u["TotalSGPRs"] <= sgpr and u["LDS Size"] == 0, (k, u)      # (no static LDS anywhere)
        assert re.search(rf"`{k}` \|[^|]*\| {vgpr} / {sgpr} / ", design), k
    if src == "hg_detr_attn":      # the dynamic LDS of the longest resident chunk: 2 x 64 B x DETR_ATTN_RESIDENT_L
        resident = int(re.search(r"DETR_ATTN_RESIDENT_L = (\d+);", hdr).group(1))
        assert 2 * 64 * resident <= kernels["detr_attn_kernel"][2] <= 160 * 1024
