"""CPU checks of the MLP pair launch with c_proj on 256 x 256 tiles (hoigen_amd/csrc/hg_mlp_pair256.hip): the dealing of an XCD's tiles
to its work slots - in both pair launches -, emulated on the host from the very header the kernels' schedules use, and the kernel's code
as compiled for gfx950 - no GPU needed."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from asm_blocks import basic_blocks, kernel_body

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pair256_dealing_deals_every_tile_once():
    """tools/pair256_deal_check.cpp: M over 2 048 .. 60 000 in steps of 64 and the rows around every panel and half-panel edge, N_fc in
    {2048, 3072} (N_proj = N_fc / 4), chunks {1, 3, 8, 32}, work ratios 1 .. 6, 32 slots on each of 8 XCDs.  Every c_fc and every c_proj
    tile is dealt exactly once and nothing outside the grid; a slot is without a c_fc tile only where its XCD has fewer c_fc tiles than
    slots (M < 8 192 rows at width 768: a panel is 12 tiles; the first T slots then own one each); in every c_proj round the items of the
    slots that own one c_proj tile more - and no more c_fc tiles than anyone - come first; loads differ by at most ratio + 1 tile times.
    And the launch with c_proj on 128-row tiles (hoigen_amd/csrc/hg_mlp_pair.hip, whose schedules run the same header): the same M and
    N_fc, chunks {1, 3, 8, 32, 64}, 1, 24 or 32 of an XCD's 32 slots running c_fc tiles.  Every c_fc tile and every 128-row c_proj tile
    is dealt exactly once and nothing outside the grid - at a half-panel edge the chip's last panel has one 128-row half only -, a
    slot's c_fc positions and c_proj items lie in list order, and no slot's start stagger (slack) is negative."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "deal_check")
        r = subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(REPO, "tools", "pair256_deal_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-3000:]
    assert int(r.stdout.split()[1]) > 15000, r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mlp_pair256_kernel_codegen():
    """What tests/test_build_resources.py::test_mlp_pair_kernel_codegen holds off in hg_mlp_pair.hip, for the three instances (stream fp32,
    hi / lo, hi / lo -> fp32) of mlp_pair256_kernel:
      * no flat_ instruction, no scratch_ access;
      * one QuickGELU epilogue block, with its interleaved schedule (<= 100 s_nop);
      * no lane moves of spilled scalars in any block that issues MFMAs;
      * 512 MFMAs: c_fc's six K-tile kinds x 64, and the four-phase K-tile of the 256 x 256 c_proj body (4 x 16) twice - the compiler
        peels one K-tile off the loop."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pair256.s")
        r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
                            os.path.join(CSRC, "hg_mlp_pair256.hip"), "-o", out], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        txt = open(out).read()
    names = re.findall(r"^(_ZN2hg18mlp_pair256_kernel\S+):", txt, re.M)
    assert len(names) == 3, names
    for name in names:
        body = kernel_body(txt, name)
        assert "flat_" not in body, name
        assert "scratch_" not in body, name
        blocks = basic_blocks(body)
        n_mfma = sum(1 for b in blocks for x in b if x.startswith("v_mfma_f32_16x16x32_f16"))
        assert n_mfma == 512, (name, n_mfma)
        epilogues = [b for b in blocks if sum(1 for x in b if x.startswith("v_exp_f32")) >= 64]
        assert len(epilogues) == 1 and sum(1 for x in epilogues[0] if x.startswith("s_nop")) <= 100, name
        for b in blocks:
            if any(x.startswith("v_mfma") for x in b):
                assert not any(x.startswith(("v_readlane", "v_writelane")) for x in b), name
