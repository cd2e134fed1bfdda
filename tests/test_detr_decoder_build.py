"""hg_detr_ffn.hip and the decoder's row kernels in hg_detr_rows.hip as the product build compiles them - build.sh's own flags for gfx950 -
cross-compiled, no GPU needed: the compiler's resource-usage remarks show every kernel without a spill and without scratch, within the
VGPR / SGPR / LDS figures of DESIGN.md section 17's table, and the LDS within a compute unit's 160 KiB.  Nothing else is inspected."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# DESIGN.md section 17's table: VGPR / SGPR / LDS bytes at most (the FFN kernel's LDS is static: 32 rows x 136 halfs)
FIGURES = {"hg_detr_ffn": {"detr_ffn_kernelILi128E": (64, 32, 8704), "detr_ffn_kernelILi256E": (64, 32, 8704)},
           "hg_detr_rows": {"detr_dec_entry_kernel": (24, 40, 0), "detr_dec_tail_kernel": (48, 56, 0)}}
NAMES = {"detr_ffn_kernelILi128E": "detr_ffn_kernel<128>", "detr_ffn_kernelILi256E": "detr_ffn_kernel<256>"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(FIGURES))
def test_no_spill_no_scratch_within_the_design_table(src):
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    assert re.search(rf"\b{src}\b", script), "the source is in build.sh's list"
    assert re.search(r"\bhg_detr_dec\b", script)
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
    for k, (vgpr, sgpr, lds) in kernels.items():
        u = usage[k]
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
        assert u["VGPRs"] <= vgpr and u["TotalSGPRs"] <= sgpr and u["LDS Size"] <= lds <= 160 * 1024, (k, u)
        assert re.search(rf"`{re.escape(NAMES.get(k, k))}` \|[^|]*\| {vgpr} / {sgpr} / {lds} ", design), k
