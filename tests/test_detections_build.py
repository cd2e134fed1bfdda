"""hg_detections.hip as the product build compiles it - build.sh's own flags for gfx950, -ffp-contract=off among them - cross-compiled, no GPU
needed: the compiler's resource-usage remarks show four kernels without a spill and without scratch, inside the register and LDS
figures of DESIGN.md §13's table; and the new entry point is declared, bound and laid out as the header has it."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from hoigen_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("det_count_kernel", "det_scan_kernel", "det_write_kernel", "det_assoc_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_spill_no_scratch_with_the_build_flags():
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    extra = re.search(r'\[ \$f = hg_detections \] && X="([^"]*)"', script)
    assert extra and extra.group(1) == "-ffp-contract=off" and "hg_detections" in script.split("for f in")[1].split(";")[0]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + extra.group(1).split() + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "hg_detections.hip"),
                            "-o", os.path.join(tmp, "hg_detections.o")], capture_output=True, text=True, timeout=900)
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
        assert u["VGPRs"] <= 64 and u["Occupancy"] == 8, (k, u)              # eight waves a SIMD: nothing here is short of registers
    assert usage["det_assoc_kernel"]["LDS Size"] <= 16 * 1024                # 256 ground-truth pairs: boxes, areas, classes, keys
    assert max(usage[k]["LDS Size"] for k in KERNELS[:3]) <= 512


def test_entry_point_is_declared_bound_and_laid_out():
    header = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    assert re.search(r"^int hg_hoi_detections\(hg_ctx\*, const hg_hoi_detections_args\* args, void\* stream\);", header, re.M)
    assert "hg_hoi_detections" in _lib.SIGNATURES
    a = _lib.hg_hoi_detections_args
    # 8 pointers, B and num_classes, conversion and n_obj_classes (+ 4 bytes of padding), 5 pointers, gt_format, min_iou and cap (+ 4), 13 pointers
    assert ctypes.sizeof(a) == 8 * 8 + 2 * 4 + 8 + 8 + 5 * 8 + 16 + 13 * 8
    assert a.B.offset == 64 and a.conversion.offset == 72 and a.gt_boxes_h.offset == 88 and a.gt_format.offset == 128 and a.cap.offset == 136
    assert a.det_off.offset == 144 and a.status.offset == 240
    fields = [n for n, _ in a._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} hg_hoi_detections_args;", header).group(1)
    declared = [n for n in re.findall(r"\*?\s*\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body)) if n not in ("float", "int32_t", "const")]
    assert declared == fields, (declared, fields)


def test_symbol_is_exported():
    assert hasattr(_lib.lib(), "hg_hoi_detections")
