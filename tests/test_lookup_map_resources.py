"""Compile-time guard on the kernels of csrc/lookup_map.hip (hipcc's `-Rpass-analysis=kernel-resource-usage` remarks, no GPU needed):
the unit holds exactly the build and the query kernel -- compiled once, for both curves: they compare 32-byte words --, neither uses
scratch memory or spills a vector register, and the unit is part of the library build (and of no committed counter file)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("lookup_map_build", "lookup_map_query")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_lookup_map_kernels_use_no_scratch():
    from ark_plonk_amd import build
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "lookup_map.hip")
    cmd = [HIPCC] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
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
        hits = {k: v for k, v in kernels.items() if f"{len(name)}{name}" in k}          # Itanium mangling: <length><name>
        assert len(hits) == 1, (name, sorted(kernels))
        for k, v in hits.items():
            print(name, v)
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert len(kernels) == len(KERNELS), sorted(kernels)


def test_unit_is_part_of_the_library_build():
    from ark_plonk_amd import build
    mine = [j for j in build.jobs() if j[1] == "lookup_map.hip"]
    assert [(j[0], j[2]) for j in mine] == [("lookup_map.o", [])]
    assert "fr_io.cuh" in mine[0][3] and "api_internal.h" in mine[0][3]
    assert all(src != "lookup_map.hip" for units in build.PMC_UNITS.values() for src, _ in units)
