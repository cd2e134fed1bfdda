"""Resources of the text tower's fused in_proj + causal attention kernel (hoigen_amd/csrc/hg_qkv_attn_text.hip), from the code object
cross-compiled for gfx950 - no GPU needed: no scratch, no register spill to memory, the LDS it is launched with inside a CU's 160 KiB,
its K loop free of vmcnt(0), and none of the scalar-store / scalar-atomic / scalar-cache-write-back instructions in source or assembly."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hoigen_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=fast"]
SOURCES = ("hg_qkv_attn_text.hip", "hg_qkv_attn_text_body.inc", "hg_seq_dev.h", "hg_seq_kloop.inc", "hg_seq_kloop_run.inc", "hg_attn_dev.h")
KERNELS = ("qkv_attn_kernel_text", "qkv_attn_kernel_text_k2")
# scalar memory writes, spelled in pieces (this file is source too)
_S = "s" + "_"
FORBIDDEN = [_S + x for x in ("store" + "_dword", "buffer" + "_store", "scratch" + "_store", "atomic" + "_", "buffer" + "_atomic",
                              "dcache" + "_wb", "dcache" + "_discard")]
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def asm():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "qt.s")
        r = subprocess.run([HIPCC, *FLAGS, "-S", "--cuda-device-only", os.path.join(CSRC, "hg_qkv_attn_text.hip"), "-o", out],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        return open(out).read()


def _kernel_descriptors(asm):
    """{kernel: {directive: value}} from the .amdhsa_kernel blocks."""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        out[m.group(1)] = {k: v for k, v in re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2))}
    return out


def _metadata(asm, name):
    """The kernel's entry of the amdhsa.kernels metadata as {key: int}."""
    blocks = re.split(r"\n  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):])
    blk = next(b for b in blocks if re.search(r"\.name:\s+" + re.escape(name) + r"\s", b))
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s", blk)}


def test_no_scratch_no_spill_and_lds_inside_160_kib(asm):
    desc = _kernel_descriptors(asm)
    names = [n for n in desc if any(f"{len(k)}{k}E" in n for k in KERNELS)]
    assert len(names) == 2, list(desc)
    m = re.search(r"hg_qkv_attn_text_lds_bytes:\s*\n\s*\.long\s+(\d+)", asm)
    assert m, "the launch's LDS size was not found in the code object"
    dynamic = int(m.group(1))
    for n in names:
        md = _metadata(asm, n)
        assert md["private_segment_fixed_size"] == 0 and desc[n]["private_segment_fixed_size"] == "0", (n, md)
        assert md["vgpr_spill_count"] == 0, (n, md)
        assert md["group_segment_fixed_size"] == 0, "the kernel's LDS is the launch's dynamic size alone"
        assert 0 < dynamic + md["group_segment_fixed_size"] <= 163840, dynamic
        assert md["vgpr_count"] <= 256 and md["max_flat_workgroup_size"] == 512, md
        body = asm[asm.index(n + ":"):]
        body = body[:body.index("s_endpgm")]
        assert "scratch_" not in body, n


def test_k_loop_keeps_its_counted_waits(asm):
    """10 row blocks: 2 k-steps x 10 x 3 = 60 MFMAs per K-tile body; the 3 m instance has six bodies, the 3 m + 2 one as well (first,
    three middle phases, second-to-last, last).  Between the first and the last counted wait of the K loop: no vmcnt(0), no scratch."""
    for k, bodies in zip(KERNELS, (6, 6)):
        name = next(n for n in _kernel_descriptors(asm) if f"{len(k)}{k}E" in n)
        body = asm[asm.index(name + ":"):]
        body = body[:body.index("s_endpgm")].split("\n")
        assert sum("v_mfma_f32_16x16x32_f16" in l for l in body) == 60 * bodies, k
        counted = [i for i, l in enumerate(body) if re.search(r"s_waitcnt vmcnt\([356]\)", l)]
        assert len(counted) >= 12, "the counted waits of the K loop were not found"
        loop = body[counted[0]:counted[-1] + 1]
        assert not [l for l in loop if "s_waitcnt vmcnt(0)" in l], f"{k}: vmcnt(0) inside the K loop"


def test_no_scalar_memory_writes_in_source_or_assembly(asm):
    texts = {"assembly": asm}
    for f in SOURCES:
        texts[f] = open(os.path.join(CSRC, f)).read()
    for where, text in texts.items():
        low = text.lower()
        for word in FORBIDDEN:
            assert not re.search(r"(?<![a-z0-9_])" + re.escape(word), low), f"{word} in {where}"

