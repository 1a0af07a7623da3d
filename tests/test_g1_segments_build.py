"""Compile-time guard on the segmented MSM's kernel (csrc/g1_segments.hip, gfx950 device code, hipcc's own
`-Rpass-analysis=kernel-resource-usage` remarks; no GPU needed): on both curves every kernel of the unit keeps its point arithmetic in
registers -- no scratch memory, no spilled VGPR, at most 256 VGPRs."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("curve_sel, name", [(0, "CurveBls"), (1, "CurveBn")])
def test_segments_kernel_registers_and_spills(curve_sel, name):
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "g1_segments.hip")
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
    assert [k for k in kernels if "g1_segments" in k and name in k], kernels.keys()      # the selected curve's kernel is in the unit
    for k, res in kernels.items():
        assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0 and res["VGPRs"] <= 256, (k, res)
