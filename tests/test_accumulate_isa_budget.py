"""Instruction budget of the MSM accumulation loop (csrc/msm_accumulate.hip: accumulate_chunk inside msm_accumulate_batch), counted
from the gfx950 assembly with tools/loop_isa_count.py; no GPU needed.

What is pinned is the common trip of the loop -- what one reference costs when no lane of its wave is at a run's start or end or
at P == +-Q (the tool's docstring defines it).  The counts of the build before the loop was restructured come from the same tool
(profiles/accumulate_lean/isa_parent.txt; the issue's hand count of that build was 4520 vector instructions, the tool's is 4445
because it walks past two conditional blocks the hand count took in).  profiles/accumulate_lean/notes.md claims a saving of 88 vector
instructions per reference on BLS12-381 and 57 on BN254; the arithmetic itself is untouched, so the multiply-adds stay what they were."""
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from ark_plonk_amd import build as zk_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#            curve: (v_mad_i64_i32, vector instructions before, claimed saving, v_mov_* of the build the notes describe)
BUDGET = {0: (3055, 4445, 88, 17),
          1: (1467, 2432, 57, 15)}


def _tool():
    spec = importlib.util.spec_from_file_location("loop_isa_count", os.path.join(ROOT, "tools", "loop_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not os.path.exists(zk_build.HIPCC), reason="hipcc not found")
def test_accumulation_loop_instruction_budget():
    tool = _tool()
    with ThreadPoolExecutor(max_workers=2) as ex:
        asm = list(ex.map(lambda c: zk_build.device_asm("msm_accumulate.hip", [f"-DZK_CURVE_SEL={c}"]), (0, 1)))
    for cid, (mads, before, saving, movs) in BUDGET.items():
        for kernel in ("msm_accumulate_batch", "msm_accumulateI"):       # the table path and the per-window path: one function
            t = tool.count_loop(asm[cid], kernel)["totals"]
            print(f"curve {cid} {kernel}: {t}")
            assert t["mad"] == mads, (cid, kernel, t)
            assert t["vector"] <= before - saving, (cid, kernel, t)
            assert t["mov"] <= movs, (cid, kernel, t)
