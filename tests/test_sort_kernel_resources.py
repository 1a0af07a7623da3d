"""Compile-time guard on the kernels of the table sort (csrc/msm_sort.hip; gfx950 device code, hipcc's own
`-Rpass-analysis=kernel-resource-usage` remarks; no GPU needed).  The compact form (csort_*): no register spill, no scratch, and at
least as many workgroups of the launch shape resident per CU as the psort_* kernel (int32 digits, uint16 low bits) each replaces.
The 16-bit table: the generic digit kernel on int16 digits neither spills nor uses scratch, nor do its instantiations of the scatter
and the placement kernel (psort_scatter<int16_t, uint8_t, 7> / psort_final<uint8_t, 7>); the scatter keeps two workgroups of 1024
lanes per CU.  The placement kernel holds ONE (at most 128 registers = 4 wavefronts per SIMD, and 83524 bytes of static LDS): its
sorted tile and keys alone are 80 KiB, half a CU's LDS, so a second one cannot fit at PS_TILE = 16384 whatever the counters beside
them take.  The test pins that one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

LDS_PER_CU = 160 * 1024          # gfx950
WAVES_PER_SIMD, SIMDS = 8, 4
PS_T, PS_SLABS, PS_STILE, PS_TILE = 1024, 1024, 8192, 16384        # csrc/msm_common.cuh
W, NB17 = 15, 256                                                   # the flagship geometry: 15 windows of 17 bits, 2^8 buckets per partition


def psort_final_lds(lob, lo_bytes):
    """LDS of psort_final<Lo, LOB>: psort_final_lds in csrc/msm_sort.hip -- dynamic, set by the launch, at LOB = 0; static at LOB = 7"""
    return (3 * (1 << lob) + 1 + 16 + PS_TILE) * 4 + PS_TILE * lo_bytes


def workgroups_per_cu(k, threads, dynamic_lds):
    """resident workgroups of `threads` lanes: by wavefront slots at the kernel's occupancy, and by LDS (static + dynamic)"""
    waves = threads // 64
    by_waves = (min(k["Occupancy"], WAVES_PER_SIMD) * SIMDS) // waves
    lds = k["LDS Size"] + dynamic_lds
    return min(by_waves, LDS_PER_CU // lds if lds else by_waves)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_compact_sort_kernels_registers_spills_and_residency():
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "msm_sort.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1000000", "--cuda-device-only",
           "-DZK_CURVE_SEL=0", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=1500).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))

    def find(name, *more):
        # Itanium mangling inside the anonymous namespace: <length><name>E for a plain function, <length><name>I... for a template
        tag = f"{len(name)}{name}" + ("I" if more else "E")
        hits = [v for k, v in kernels.items() if tag in k and all(p in k for p in more)]
        assert len(hits) == 1, (name, more, [k for k in kernels if name in k])
        return hits[0]

    new = {"fold_t": find("csort_fold_hist", "Lb1E"), "fold_f": find("csort_fold_hist", "Lb0E"), "scatter": find("csort_scatter"),
           "final": find("csort_final"), "long": find("csort_final_long")}
    for name, k in new.items():
        assert k["VGPRs Spill"] == 0 and k["ScratchSize"] == 0, (name, k)
    # launch shapes and dynamic LDS as pre_queue_digits / pre_queue_sort_rest set them
    old_digits = workgroups_per_cu(find("psort_digits_hist", "Lb1EiE"), 256, 0)
    assert workgroups_per_cu(new["fold_t"], 256, 0) >= old_digits, (new["fold_t"], old_digits)
    assert workgroups_per_cu(new["fold_f"], 256, 0) >= workgroups_per_cu(find("psort_digits_hist", "Lb0EiE"), 256, 0)
    old_scatter = workgroups_per_cu(find("psort_scatter", "IitLj0EE"), PS_T, 0)
    assert workgroups_per_cu(new["scatter"], PS_T, W * PS_T * 4) >= old_scatter, (new["scatter"], old_scatter)
    assert psort_final_lds(8, 2) == (3 * NB17 + 1 + 16 + PS_TILE) * 4 + PS_TILE * 2
    old_final = workgroups_per_cu(find("psort_final", "ItLj0EE"), PS_T, psort_final_lds(8, 2))
    assert workgroups_per_cu(new["final"], PS_T, (PS_SLABS + 1 + PS_TILE) * 4 + PS_TILE * 3) >= old_final, (new["final"], old_final)
    assert workgroups_per_cu(new["long"], PS_T, (PS_SLABS + PS_TILE) * 4 + PS_TILE) >= old_final, (new["long"], old_final)
    # the 16-bit instantiations: lob = 16 - 9
    for mont in ("Lb1EsE", "Lb0EsE"):
        k = find("psort_digits_hist", mont)
        assert k["VGPRs Spill"] == 0 and k["ScratchSize"] == 0, (mont, k)
    narrow_scatter = find("psort_scatter", "IshLj7EE")
    narrow_final = find("psort_final", "IhLj7EE")
    for k in (narrow_scatter, narrow_final):
        assert k["VGPRs Spill"] == 0 and k["ScratchSize"] == 0, k
    assert workgroups_per_cu(narrow_scatter, PS_T, 0) >= 2, narrow_scatter
    # one workgroup by LDS whatever the registers; 128 registers is what a 1024-lane workgroup can have at all without spilling
    assert narrow_final["VGPRs"] <= 128, narrow_final
    # (its LDS of psort_final_lds(7, 1) bytes is static, so "LDS Size" holds it and the launch adds none)
    assert psort_final_lds(7, 1) == 83524 and narrow_final["LDS Size"] >= psort_final_lds(7, 1), narrow_final
    assert workgroups_per_cu(narrow_final, PS_T, 0) == 1, narrow_final
