"""Resources of the instance adapter's kernels for 225 .. 640 tokens (hoigen_amd/csrc/hg_adapter_long.hip), from the code object
cross-compiled for gfx950 - no GPU needed: no scratch, no register spill, the decoder inside 256 VGPRs at its 512-thread bound, the LDS
it is launched with equal to the short decoder's map (148 992 B) and inside a CU's 160 KiB."""
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
DECODER, KV = "adapter_decoder_long", "adapter_kv16_kernel"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def asm():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "adl.s")
        r = subprocess.run([HIPCC, *FLAGS, "-S", "--cuda-device-only", os.path.join(CSRC, "hg_adapter_long.hip"), "-o", out],
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


def _body(asm, name):
    body = asm[asm.index(name + ":"):]
    return body[:body.index("s_endpgm")]


def test_both_kernels_are_there_without_scratch_or_spill(asm):
    desc = _kernel_descriptors(asm)
    dec = sorted(n for n in desc if f"{len(DECODER)}{DECODER}" in n)
    kv = [n for n in desc if f"{len(KV)}{KV}" in n]
    assert len(dec) == 2 and len(kv) == 1, list(desc)      # SELF = false / true, and the K / V projection
    for n in dec + kv:
        md = _metadata(asm, n)
        assert md["private_segment_fixed_size"] == 0 and desc[n]["private_segment_fixed_size"] == "0", (n, md)
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (n, md)
        assert "scratch_" not in _body(asm, n), n
        print(f"\n{n}: vgpr {md['vgpr_count']} agpr {md.get('agpr_count', 0)} sgpr {md['sgpr_count']} lds {md['group_segment_fixed_size']}")


def test_decoder_fits_512_threads_and_the_short_kernels_lds_map(asm):
    m = re.search(r"hg_adapter_long_lds_bytes:\s*\n\s*\.long\s+(\d+)", asm)
    assert m, "the launch's LDS size was not found in the code object"
    dynamic = int(m.group(1))
    assert dynamic == 148992, dynamic
    for n in _kernel_descriptors(asm):
        if f"{len(DECODER)}{DECODER}" not in n:
            continue
        md = _metadata(asm, n)
        assert md["max_flat_workgroup_size"] == 512 and md["vgpr_count"] <= 256, md
        assert md["group_segment_fixed_size"] == 0, "the decoder's LDS is the launch's dynamic size alone"
        assert dynamic <= 163840
        body = _body(asm, n)
        assert "v_mfma_f32_16x16x32_f16" in body and "s_barrier" in body, n


def test_kv_kernel_lds_is_static_and_small(asm):
    n = next(n for n in _kernel_descriptors(asm) if f"{len(KV)}{KV}" in n)
    md = _metadata(asm, n)
    # four waves x (32 rows of 136 halfs + 64 rows of 40 halfs)
    assert md["group_segment_fixed_size"] == 4 * (32 * 136 + 64 * 40) * 2, md
    assert md["max_flat_workgroup_size"] == 256, md
