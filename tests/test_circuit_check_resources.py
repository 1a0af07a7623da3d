"""Compile-time guard on the kernels of the circuit check (csrc/check.hip; hipcc's `-Rpass-analysis=kernel-resource-usage`
remarks, no GPU needed): no kernel of the unit, for either curve, uses scratch memory or spills a register.  The gate kernel holds the
terms of five widgets; a spill there would put it behind the quotient kernel it is a subset of."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("check_gates", "check_id_keys", "map_build", "check_copy", "check_lookup", "check_summary", "check_finish")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_check_kernels_use_no_scratch():
    from ark_plonk_amd import build
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "check.hip")
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
        hits = {k: v for k, v in kernels.items() if f"{len(name)}{name}" in k}         # Itanium mangling: <length><name>
        # the field kernels exist once per curve, the map kernels once per key width
        want = 2 if name in ("check_gates", "check_id_keys", "map_build") else 1
        assert len(hits) == want, (name, sorted(kernels))
        for k, v in hits.items():
            print(name, v)
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert len(kernels) == 2 + 2 + 2 + 4, sorted(kernels)
