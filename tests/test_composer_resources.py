"""Compile-time guard on the kernels of the device composer's two units (csrc/gadget_layout.hip, csrc/gadget_witness.hip; hipcc's
`-Rpass-analysis=kernel-resource-usage` remarks, no GPU needed): no kernel of either unit, for either curve, uses scratch memory or
spills a vector register.  The prefix shifts and both scalar walks (the NAF digits of the fixed base, the bits of the variable base)
read their word arrays with compile-time indices only; a run-time index would send the array to scratch memory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = {
    "gadget_layout.hip": ("gadget_layout", "gadget_insertions", "lookup_table_fill"),
    "gadget_witness.hip": ("gadget_w_poly", "gadget_w_range", "gadget_w_logic", "gadget_w_curve", "gadget_w_fixed_walk", "gadget_w_fixed_norm",
                           "gadget_w_select", "gadget_w_is_zero", "gadget_w_var_bits", "gadget_w_var_walk", "gadget_w_var_norm"),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_gadget_kernels_use_no_scratch(unit):
    from ark_plonk_amd import build
    names = UNITS[unit]
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", unit)
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
    for name in names:
        hits = {k: v for k, v in kernels.items() if f"{len(name)}{name}I" in k}        # Itanium mangling: <length><name>, then the curve
        assert len(hits) == 2, (name, sorted(kernels))
        for k, v in hits.items():
            print(name, v)
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert len(kernels) == 2 * len(names), sorted(kernels)
