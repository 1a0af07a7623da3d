"""Instruction budget of the MSM accumulation loop over the chained field products of csrc/fields.cuh (Fs<P, true>: one multiply-add
chain per column, Fs::link, with a three-instruction end of every high-half column, Fs::finish_high); counted from the gfx950 assembly with
tools/loop_isa_count.py, no GPU needed.  profiles/field_chains/notes.md has the table of the forms that were tried.

What is pinned, on the common trip of the loop (the tool's docstring defines it), for both curves and both kernels:
  * the multiply-adds are exactly the formula's: a form of the high-half digit that lets the optimiser see a sign extension trades
    v_mad_i64_i32 for v_mad_u64_u32 + v_mul_lo_u32 (the trap of the notes' table), so neither of those may exceed the parent's count;
  * the register copies are no more than the parent's;
  * the vector instructions are at most what this build shows (the parent's are given beside them)."""
import collections
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from ark_plonk_amd import build as zk_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (curve, kernel): (v_mad_i64_i32, parent's v_mad_u64_u32, parent's v_mul_lo_u32, v_mov_*, vector instructions of this build, of the parent)
BUDGET = {(0, "msm_accumulate_batch"): (3055, 2, 117, 17, 4104, 4357),
          (0, "msm_accumulateI"): (3055, 0, 117, 15, 4098, 4351),
          (1, "msm_accumulate_batch"): (1467, 4, 81, 15, 2207, 2375),
          (1, "msm_accumulateI"): (1467, 1, 81, 12, 2199, 2367)}


def _tool():
    spec = importlib.util.spec_from_file_location("loop_isa_count", os.path.join(ROOT, "tools", "loop_isa_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trip_opcodes(tool, asm, kernel, res):
    """opcode -> count over the blocks of the common trip"""
    trip = {name for name, _, tag in res["blocks"] if tag == "trip"}
    _, body = tool.kernel_body(asm, kernel)
    ops = collections.Counter()
    for name, ins in tool.basic_blocks(body):
        if name in trip:
            ops.update(l.split()[0] for l in ins)
    return ops


@pytest.mark.skipif(not os.path.exists(zk_build.HIPCC), reason="hipcc not found")
def test_field_chain_instruction_budget():
    tool = _tool()
    with ThreadPoolExecutor(max_workers=2) as ex:
        asm = list(ex.map(lambda c: zk_build.device_asm("msm_accumulate.hip", [f"-DZK_CURVE_SEL={c}"]), (0, 1)))
    for (cid, kernel), (mads, umads, mul_lo, movs, vector, parent_vector) in BUDGET.items():
        res = tool.count_loop(asm[cid], kernel)
        t = res["totals"]
        ops = _trip_opcodes(tool, asm[cid], kernel, res)
        print(f"curve {cid} {kernel}: {t} v_mad_u64_u32 {ops['v_mad_u64_u32']} v_mul_lo_u32 {ops['v_mul_lo_u32']} "
              f"v_lshl_add_u64 {ops['v_lshl_add_u64']} s_nop {ops['s_nop']} (parent: {parent_vector} vector)")
        assert sum(n for o, n in ops.items() if o.startswith("v_mad_i64_i32")) == t["mad"]
        assert t["mad"] == mads, (cid, kernel, t)
        assert ops["v_mad_u64_u32"] <= umads and ops["v_mul_lo_u32"] <= mul_lo, (cid, kernel, ops["v_mad_u64_u32"], ops["v_mul_lo_u32"])
        assert t["mov"] <= movs, (cid, kernel, t)
        assert t["vector"] <= vector < parent_vector, (cid, kernel, t)
