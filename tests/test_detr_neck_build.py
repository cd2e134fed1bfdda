"""hg_detr_neck.hip as the product build compiles it - build.sh's own flags for gfx950, with the flag build.sh adds for this file -
cross-compiled, no GPU needed: the compiler's resource-usage remarks show the kernels without a spill and without scratch, within the
VGPR / SGPR / LDS figures of DESIGN.md section 19's table, and the LDS within a compute unit's 160 KiB.  Nothing else is inspected."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = "hg_detr_neck"
# DESIGN.md section 19's table: VGPR / SGPR / LDS bytes at most (the LDS is static: two 32 x 72 fp16 blocks of x, the 1 792-byte grid, 32 x 2 floats)
FIGURES = {"detr_neck_kernelILi128E": (80, 96, 11264), "detr_neck_kernelILi256E": (128, 96, 11264), "detr_neck_sum_kernel": (16, 32, 0)}
NAMES = {"detr_neck_kernelILi128E": "detr_neck_kernel<128>", "detr_neck_kernelILi256E": "detr_neck_kernel<256>",
         "detr_neck_sum_kernel": "detr_neck_sum_kernel"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_spill_no_scratch_within_the_design_table():
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    assert re.search(rf"\b{SRC}\b", script), "the source is in build.sh's list"
    extra = re.search(rf'\[ \$f = {SRC} \] && X="([^"]*)"', script)
    assert extra, "build.sh compiles this file without contraction"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + extra.group(1).split() + ["-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(CSRC, SRC + ".hip"), "-o", os.path.join(tmp, SRC + ".o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in FIGURES if k in m.group(1)), None)
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert set(usage) == set(FIGURES), usage
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for k, (vgpr, sgpr, lds) in FIGURES.items():
        u = usage[k]
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] <= vgpr and u["TotalSGPRs"] <= sgpr and u["LDS Size"] <= lds <= 160 * 1024, (k, u)
        assert re.search(rf"`{re.escape(NAMES[k])}` \|[^|]*\| {vgpr} / {sgpr} / {lds} ", design), k
