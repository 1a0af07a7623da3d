"""Compile-time guard on the device replay's kernel (csrc/replay.hip; hipcc's `-Rpass-analysis=kernel-resource-usage` remarks, no GPU
needed): for both curves no scratch memory, no spilled register, and 12.8 KB of LDS -- 200 sponge bytes for each of a wave's 64 lanes.
Scratch would mean that an array of the sponge or of the walk is indexed at run time, or that a function the kernel calls (the
permutation, the field product) calls another one: both are what csrc/strobe.cuh and csrc/replay_walk.cuh are written to avoid."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_replay_kernel_uses_no_scratch():
    from ark_plonk_amd import build
    assert ("replay.o", "replay.hip") in [(obj, src) for obj, src, _, _ in build.jobs()]
    assert not any(src == "replay.hip" for units in build.PMC_UNITS.values() for src, _ in units)
    src = os.path.join(ROOT, "ark_plonk_amd", "csrc", "replay.hip")
    cmd = [HIPCC] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    hits = {k: v for k, v in kernels.items() if "12proof_replay" in k}                    # Itanium mangling: <length><name>
    assert len(hits) == 2 == len(kernels), sorted(kernels)                                # one per curve, nothing else in the unit
    for k, v in hits.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["LDS Size"] == 200 * 64, (k, v)
