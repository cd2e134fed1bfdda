"""hg_detector_views.hip as the product build compiles it - build.sh's own flags for gfx950 with -ffp-contract=off - cross-compiled, no GPU
needed: the compiler's resource-usage remarks show two kernels without a spill and without scratch, with at most the VGPRs, SGPRs and
LDS of DESIGN.md §15's table."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import detector_views_model as dvm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("dv_tables_kernel", "dv_resample_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_spill_no_scratch_with_the_build_flags():
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    extra = re.search(r'\[ \$f = hg_detector_views \] && X="([^"]*)"', script)
    assert extra and extra.group(1) == "-ffp-contract=off"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + extra.group(1).split() + ["-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(CSRC, "hg_detector_views.hip"), "-o", os.path.join(tmp, "hg_detector_views.o")],
                           capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), None)
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert set(usage) == set(KERNELS), usage
    for k, u in usage.items():
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
    # DESIGN.md §15's table: VGPR / SGPR / LDS.  512-thread workgroups of the resample kernel: four a CU need 8 waves a SIMD (at most 64
    # VGPRs) and 4 x 19 200 bytes of the 160 KiB
    figures = {"dv_tables_kernel": (44, 35, 0), "dv_resample_kernel": (50, 72, 19200)}
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for k, (vgpr, sgpr, lds) in figures.items():
        assert usage[k]["VGPRs"] <= vgpr and usage[k]["TotalSGPRs"] <= sgpr and usage[k]["LDS Size"] <= lds and usage[k]["Occupancy"] >= 8, (k, usage[k])
        assert re.search(rf"`{k}` \|[^|]*\| {vgpr} / {sgpr} / ", design), k
    # the window, the weight words, the bounds and the 3 x 256 table are the kernel's whole LDS
    assert 3 * 256 * 4 + dvm.VW_WORDS * 4 + dvm.BAND * 2 * 4 + dvm.WIN_ROWS * dvm.STRIP * 3 == 19200
