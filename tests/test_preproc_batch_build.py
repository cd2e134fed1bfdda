"""hg_preproc_batch.hip as the product build compiles it - build.sh's own flags for gfx950 with -ffp-contract=off - cross-compiled, no GPU
needed: the compiler's resource-usage remarks show two kernels without a spill and without scratch, with at most the VGPRs and SGPRs of
DESIGN.md §14's table; the LDS the resample kernel is launched with (dynamic: hg_preproc_geom.h's preb_lds_bytes, restated in
tests/preproc_batch_model.py) is within that table's figure and the 160 KiB of a CU; and the new entry point is declared, bound and
laid out as the header has it."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import preproc_batch_model as pbm
from hoigen_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("prebatch_tables_kernel", "prebatch_resample_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_spill_no_scratch_with_the_build_flags():
    script = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', script, re.M).group(1).replace("${HG_EXTRA_FLAGS}", "").split()
    extra = re.search(r'\[ \$f = hg_preproc_batch \] && X="([^"]*)"', script)
    assert extra and extra.group(1) == "-ffp-contract=off" and "hg_preproc_batch" in script.split("for f in")[1].split(";")[0]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC] + flags + extra.group(1).split() + ["-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(CSRC, "hg_preproc_batch.hip"), "-o", os.path.join(tmp, "hg_preproc_batch.o")],
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
    # DESIGN.md §14's table: 52 / 49 and 70 / 105 (VGPR / SGPR).  The resample kernel runs 512-thread workgroups, two a CU at n_px 224:
    # four waves a SIMD, which anything up to 128 VGPRs allows
    figures = {"prebatch_tables_kernel": (52, 49), "prebatch_resample_kernel": (70, 105)}
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for k, (vgpr, sgpr) in figures.items():
        assert usage[k]["VGPRs"] <= vgpr and usage[k]["TotalSGPRs"] <= sgpr and usage[k]["Occupancy"] >= 4, (k, usage[k])
        assert re.search(rf"`{k}` \|[^|]*\| {vgpr} / {sgpr} / ", design), k
    assert usage["prebatch_tables_kernel"]["LDS Size"] <= 128                  # the crop's header
    assert usage["prebatch_resample_kernel"]["LDS Size"] == 0                  # no static LDS in front of the dynamic region (16-byte base)


def test_lds_of_the_launch_is_within_the_design_table():
    """dynamic LDS = 3 KiB table + the band's vertical weights + row buffer + 72-row window + the crop's horizontal weights, from n_px alone (the header's own formula,
    evaluated): DESIGN.md §14 gives 78 688 bytes at 224, 145 664 at 518"""
    lds = pbm.header_functions()["preb_lds_bytes"]
    assert lds(224) == 78688 and lds(518) == 145664 <= 160 * 1024 and pbm.header_constants()["PREB_MAX_NPX"] == 518
    assert all(lds(n) <= 160 * 1024 and lds(n) % 16 == 0 for n in range(1, 519)) and 2 * lds(224) <= 160 * 1024      # two workgroups a CU at 224
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "78 688" in design and "145 664" in design


def test_entry_point_is_declared_bound_and_laid_out():
    header = open(os.path.join(REPO, "include", "hoigen_amd.h")).read()
    assert re.search(r"^int hg_preprocess_batch\(hg_ctx\*, const hg_preprocess_batch_args\* args, void\* stream\);", header, re.M)
    assert "hg_preprocess_batch" in _lib.SIGNATURES
    a = _lib.hg_preprocess_batch_args
    # 3 pointers, B (+ 4 bytes of padding), 2 pointers, n, n_px, flags, background, 3 pointers
    assert ctypes.sizeof(a) == 3 * 8 + 8 + 2 * 8 + 4 * 4 + 3 * 8
    assert a.B.offset == 24 and a.boxes.offset == 32 and a.n.offset == 48 and a.background.offset == 60 and a.out.offset == 64 and a.status.offset == 80
    fields = [n for n, _ in a._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} hg_preprocess_batch_args;", header).group(1)
    declared = [n for n in re.findall(r"\*?\s*\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body)) if n not in ("float", "int32_t", "const", "uint8_t", "uint32_t")]
    assert declared == fields, (declared, fields)
    assert (_lib.HG_PRE_MAX_IMAGES, _lib.HG_PRE_MAX_N, _lib.HG_PRE_MAX_NPX, _lib.HG_PRE_MAX_TAPS) == (pbm.MAX_IMAGES, pbm.MAX_N, pbm.MAX_NPX, pbm.MAX_TAPS)


def test_symbol_is_exported():
    assert hasattr(_lib.lib(), "hg_preprocess_batch")
