"""Compile-time guard on the kernels of the device composer's second unit (csrc/gadgets_ext.hip), by the method of
tests/test_composer_resources.py (hipcc's `-Rpass-analysis=kernel-resource-usage` remarks, no GPU needed): no kernel of the unit,
for either curve, uses scratch memory or spills a vector register.  The variable-base walk reads the scalar's bits off the top of a
word array that is shifted with compile-time indices; a run-time index would send the array to scratch memory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("gadget_layout_ext", "gadget_insertions_ext", "gadget_w_select", "gadget_w_is_zero", "gadget_w_var_bits", "gadget_w_var_walk",
           "gadget_w_var_norm", "lookup_table_fill")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gadget_ext_kernels_use_no_scratch():
    from ark_plonk_amd import build
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "gadgets_ext.hip")
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
