"""Compile-time guard on the kernels of the device composer (csrc/gadgets.hip; hipcc's `-Rpass-analysis=kernel-resource-usage`
remarks, no GPU needed): no kernel of the unit, for either curve, uses scratch memory or spills a vector register.  The prefix shifts
and the NAF walk index their word arrays with compile-time indices only; a run-time index would send the array to scratch memory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("gadget_layout", "gadget_insertions", "gadget_w_poly", "gadget_w_range", "gadget_w_logic", "gadget_w_curve", "gadget_w_fixed_walk",
           "gadget_w_fixed_norm")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gadget_kernels_use_no_scratch():
    from ark_plonk_amd import build
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "gadgets.hip")
    cmd = [HIPCC] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
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
    for name in KERNELS:
        hits = {k: v for k, v in kernels.items() if f"{len(name)}{name}I" in k}        # Itanium mangling: <length><name>, then the curve
        assert len(hits) == 2, (name, sorted(kernels))
        for k, v in hits.items():
            print(name, v)
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert len(kernels) == 2 * len(KERNELS), sorted(kernels)
