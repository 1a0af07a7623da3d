"""Compile-time guard on the kernels of the IPA key derivation (csrc/ipa_setup.hip, gfx950 device code, hipcc's own
`-Rpass-analysis=kernel-resource-usage` remarks; no GPU needed): on both curves every kernel of the unit -- the wave-local candidate
search for either digest, the cofactor clearing, from_random_bytes -- keeps its hash state and its field arithmetic in registers: no
scratch memory, no spilled VGPR, at most 256 VGPRs.  The unit is in the library's build list, which is also the list the host-side
sanitizer build compiles (tests/test_sanitize.py)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("curve_sel, name", [(0, "CurveBls"), (1, "CurveBn")])
def test_setup_kernels_registers_and_spills(curve_sel, name):
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "ipa_setup.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-pragma-unroll-threshold=1000000", "--cuda-device-only",
           f"-DZK_CURVE_SEL={curve_sel}", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    # the selected curve's kernels are in the unit, and no other curve's: two searches (one per digest), from_random_bytes, and the
    # cofactor clearing where the cofactor is not 1
    assert all(name in k for k in kernels), kernels.keys()
    assert len([k for k in kernels if "h2c_search" in k]) == 2 and len([k for k in kernels if "g1_from_random_bytes" in k]) == 1
    assert len([k for k in kernels if "g1_clear_cofactor" in k]) == (1 if curve_sel == 0 else 0)
    for k, res in kernels.items():
        print(k, res)
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["VGPRs"] <= 256, (k, res)


def test_unit_is_in_the_build_list():
    from ark_plonk_amd import build
    job = [(obj, src, hdrs) for obj, src, _, hdrs in build.jobs() if src == "ipa_setup.hip"]
    assert len(job) == 1 and job[0][0] == "ipa_setup.o" and {"h2c.cuh", "block_inverse.cuh", "ecu.cuh"} <= set(job[0][2])
    assert not any(src == "ipa_setup.hip" for units in build.PMC_UNITS.values() for src, _ in units)
