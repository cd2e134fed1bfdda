"""CPU check of the MLP pair launch with c_proj on 256 x 256 tiles and the two-phase K loop (hoigen_amd/csrc/hg_mlp_pair256p.hip): the
kernel's code as compiled for gfx950 - no GPU needed."""
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


def labelled_blocks(body):
    """(label, instructions) per basic block of a kernel body, in text order; the entry block's label is None."""
    blocks, label, cur = [], None, []
    for line in body.split("\n"):
        m = re.match(r"^(\.LBB\S+):", line)
        if m:
            blocks.append((label, cur))
            label, cur = m.group(1), []
        else:
            ins = re.sub(r";.*", "", line).strip()
            if ins and not ins.startswith("."):
                cur.append(ins)
    blocks.append((label, cur))
    return blocks


def metadata(txt, name):
    """The numeric fields of kernel `name` in the assembly file's amdhsa.kernels metadata."""
    i = txt.index(".name:           " + name)
    j = txt.find("  - .agpr_count", i)
    entry = txt[i:j if j >= 0 else len(txt)]
    return {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", entry, re.M)}


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pair256p.s")
        r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only",
                            os.path.join(CSRC, "hg_mlp_pair256p.hip"), "-o", out], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return open(out).read()


def kernel_names(txt):
    return re.findall(r"^(_ZN2hg19mlp_pair256p_kernel\S+):", txt, re.M)


def test_three_instances_without_flat_scratch_or_spills(asm):
    """Stream fp32, hi / lo, hi / lo -> fp32: no flat_ instruction, no scratch_ access, no spilled VGPR, at most 3 spilled SGPRs, no
    private segment."""
    names = kernel_names(asm)
    assert len(names) == 3, names
    for name in names:
        body = kernel_body(asm, name)
        assert "flat_" not in body, name
        assert "scratch_" not in body, name
        md = metadata(asm, name)
        assert md["vgpr_spill_count"] == 0, (name, md)
        assert md["sgpr_spill_count"] <= 3, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)


def test_quickgelu_epilogue_and_no_lane_moves_beside_mfmas(asm):
    """As in mlp_pair256_kernel: one QuickGELU epilogue block with its interleaved schedule (<= 100 s_nop), and no lane moves of spilled
    scalars in any block that issues MFMAs."""
    for name in kernel_names(asm):
        blocks = basic_blocks(kernel_body(asm, name))
        epilogues = [b for b in blocks if sum(1 for x in b if x.startswith("v_exp_f32")) >= 64]
        assert len(epilogues) == 1 and sum(1 for x in epilogues[0] if x.startswith("s_nop")) <= 100, name
        for b in blocks:
            if any(x.startswith("v_mfma") for x in b):
                assert not any(x.startswith(("v_readlane", "v_writelane")) for x in b), name


def c_proj_loop(asm, name):
    """The steady-state loop of kernel `name`'s c_proj body (it lies behind c_fc's QuickGELU epilogue): the one block there that
    issues MFMAs and whose first branch goes back to its own label; its instructions up to and including that branch."""
    blocks = labelled_blocks(kernel_body(asm, name))
    i_epi = [i for i, (_, b) in enumerate(blocks) if sum(1 for x in b if x.startswith("v_exp_f32")) >= 64]
    assert len(i_epi) == 1, name
    loops = []
    for label, b in blocks[i_epi[0] + 1:]:
        # (the text behind a label runs on past a conditional branch: the block proper ends at its first branch)
        i_br = [i for i, x in enumerate(b) if x.startswith(("s_cbranch", "s_branch", "s_setpc", "s_call", "s_swappc"))]
        if not i_br:
            continue
        head = b[:i_br[0] + 1]
        if any(x.startswith("v_mfma") for x in head) and label and re.match(r"s_cbranch_\w+\s+" + re.escape(label) + r"$", head[-1]):
            loops.append(head)
    assert len(loops) == 1, (name, len(loops))
    return loops[0]


def test_c_proj_steady_state_loop(asm):
    """The c_proj steady-state loop is ONE block that branches back to itself, holds the 64 MFMAs of a two-phase K-tile, no other branch
    (its back edge is its last instruction, by construction of c_proj_loop) and no decision: the one comparison is the scalar one the
    back edge reads."""
    for name in kernel_names(asm):
        loop = c_proj_loop(asm, name)
        mfmas = [x for x in loop if x.startswith("v_mfma_f32_16x16x32_f16")]
        assert len(mfmas) == 64, (name, len(mfmas))
        compares = [x for x in loop if x.startswith(("s_cmp", "v_cmp", "s_cselect", "v_cndmask", "s_bitcmp"))]
        assert len(compares) == 1 and compares[0].startswith("s_cmp"), (name, compares)


def test_c_proj_loop_mfma_tuples_start_at_multiples_of_4(asm):
    """Every register tuple of the loop's MFMAs starts at a multiple of 4 registers (the fragments are read into fixed tuples,
    hg_gemm_ring_body.h: ds_read_fixed; left to the register allocator they start at 2 (mod 4), where MFMAs issue slower)."""
    for name in kernel_names(asm):
        for x in c_proj_loop(asm, name):
            if x.startswith("v_mfma_f32_16x16x32_f16"):
                firsts = [int(v) for v in re.findall(r"v\[(\d+):\d+\]", x)]
                assert len(firsts) == 4 and all(v % 4 == 0 for v in firsts), (name, x)
