"""hg_resnet_stem.hip as the product build compiles it - build.sh's own flags for gfx950 - cross-compiled, no GPU needed: the compiler's
resource-usage remarks show the kernels without a spill and without scratch, within the VGPR / SGPR / LDS figures of DESIGN.md section
21's table, and the LDS within a compute unit's 160 KiB.  Nothing else is inspected."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = "hg_resnet_stem"
# DESIGN.md section 21's table: VGPR / SGPR / LDS bytes at most (the LDS is static: the 3 x 23 x 40 fp16 patch and the 153 x 68 fp32 conv tile)
FIGURES = {"resnet_stem_kernel": (80, 56, 47136), "resnet_stem_pack_kernel": (16, 32, 0)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_spill_no_scratch_within_the_design_table():
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    assert re.search(rf"\b{SRC}\b", script), "the source is in build.sh's list"
    assert not re.search(rf"\[ \$f = {SRC} \]", script), "build.sh compiles this file with the default flags"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, SRC + ".hip"), "-o",
                            os.path.join(tmp, SRC + ".o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in sorted(FIGURES, key=len, reverse=True) if k in m.group(1)), None)
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert set(usage) == set(FIGURES), usage
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for k, (vgpr, sgpr, lds) in FIGURES.items():
        u = usage[k]
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] <= vgpr and u["TotalSGPRs"] <= sgpr and u["LDS Size"] <= lds <= 160 * 1024, (k, u)
        assert re.search(rf"`{re.escape(k)}` \|[^|]*\| {vgpr} / {sgpr} / {lds} ", design), k
