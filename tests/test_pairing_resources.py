"""Compile-time guard on the two batch kernels of csrc/pairing.hip (no GPU needed): their register, scratch and LDS figures, read from
the code-object metadata in the gfx950 assembly `build.device_asm` produces, stay inside what the hardware can launch at all --
at most 512 registers per lane (256 architectural + 256 accumulation VGPRs) and at most 160 KiB of LDS per workgroup.  The scratch
figure is printed and recorded in profiles/pairing/notes.md; no number chosen in advance is asserted for it: the running Fq12 values
of a lane (576 bytes each on BLS12-381) live there by design (csrc/pairing.cuh)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("pairing_check_batch", "pairing_gt_batch")
# Wavefronts of these kernels that one SIMD holds at once: 512 registers per lane // .vgpr_count of the line printed below, which is
# 404 (BN254) and 511 (BLS12-381) for both kernels: 1.  tests/test_pairing_gpu.py sizes its more-waves-than-the-card-holds batch by it
# (4 SIMDs per CU, one wavefront per workgroup); the assertion below keeps it an upper bound of what the compiler allows.
WAVES_PER_SIMD = 1


def kernel_metadata(asm):
    """{kernel symbol: {field: int}} from the amdhsa.kernels list of the assembly's metadata note"""
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n  - \.", meta)[1:]:
        block = "    ." + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_pairing_kernels_fit_the_register_file_and_the_lds():
    from ark_plonk_amd import build
    assert ("pairing.o", "pairing.hip") in [(obj, src) for obj, src, _, _ in build.jobs()]
    meta = kernel_metadata(build.device_asm("pairing.hip"))
    hits = {k: v for k, v in meta.items() if any(name in k for name in KERNELS)}
    assert len(hits) == 4 == len(meta), sorted(meta)                   # two kernels, two curves, nothing else in the unit
    for k, v in sorted(hits.items()):
        regs = v["vgpr_count"]              # gfx950's unified file: .vgpr_count is the whole allocation, .agpr_count its accumulation part
        print(k, "vgpr", v["vgpr_count"], "agpr", v.get("agpr_count", 0), "sgpr", v["sgpr_count"], "scratch bytes/lane",
              v["private_segment_fixed_size"], "lds bytes/workgroup", v["group_segment_fixed_size"])
        assert v.get("agpr_count", 0) <= regs <= 512, (k, v)
        assert v["group_segment_fixed_size"] <= 160 * 1024, (k, v)
        assert v["max_flat_workgroup_size"] == 64 and v["wavefront_size"] == 64, (k, v)
        assert 1 <= 512 // regs <= WAVES_PER_SIMD, (k, regs)
