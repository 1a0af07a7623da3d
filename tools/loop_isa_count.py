#!/usr/bin/env python3
"""Instruction counts of a kernel's hot loop, per basic block, from the gfx950 assembly the library build would produce.
usage: tools/loop_isa_count.py <unit.hip> <kernel-name substring> [-DNAME=VALUE ...] [--asm file.s]
  e.g. tools/loop_isa_count.py msm_accumulate.hip msm_accumulate_batch -DZK_CURVE_SEL=0
Needs hipcc and no GPU (ark_plonk_amd.build.device_asm); --asm counts an assembly file that is already there.

The hot loop is the loop of the kernel (a strongly connected set of basic blocks) that holds the most v_mad_i64_i32; loops nested in it
are part of it.  Per block: all instructions, vector instructions (v_*, memory instructions are listed apart), v_mad_i64_i32, v_mov_*,
v_cmp_*.  Divergent code is laid out in line and skipped on the wave's vote, so the control flow alone does not say which arithmetic
a reference normally runs.  The rule used here: of the blocks that hold multiply-adds and can be skipped, the one(s) from which no
further multiply-add block is reached before the loop header comes round again while another multiply-add block leads to them are an
exceptional exit -- the doubling of P == Q in the MSM accumulation, which starts only after the general formula has found ZZ3 = 0 --
(check the common trip's v_mad_i64_i32 against the formula's count, 3055 for BLS12-381, to see that the rule picked the right block).
The "common trip" is what a reference costs when no lane of its wave needs a conditional block: from the loop header through every
block of the ordinary arithmetic and back, by the way with the fewest instructions between them.  "whole loop" sums every block."""
import os
import re
import sys

BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\S+)")
MEM = ("global_", "flat_", "buffer_", "scratch_", "ds_", "s_load", "s_buffer_load")


def kernel_body(asm, name):
    """lines of the first kernel whose symbol contains `name` (kernels are the symbols that have an .amdhsa_kernel record)"""
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    hit = [k for k in kernels if name in k]
    if not hit:
        raise SystemExit(f"no kernel matching {name!r}; kernels: {kernels}")
    sym = hit[0]
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return sym, lines[start + 1:end]


def basic_blocks(body):
    """[(name, [instruction, ...])], split at labels and after branches"""
    blocks, cur, name, sub = [], [], "entry", 0
    for raw in body:
        l = raw.split(";")[0].strip()
        if not l:
            continue
        m = re.match(r"^(\.L\w+):", l)
        if m:
            if cur or name == "entry":
                blocks.append((name, cur))
            name, cur, sub = m.group(1), [], 0
            continue
        if l.startswith("."):
            continue
        cur.append(l)
        if BRANCH.match(l) or l.startswith("s_endpgm") or l.startswith("s_setpc"):
            blocks.append((name, cur))
            sub += 1
            name, cur = f"{name.split('+')[0]}+{sub}", []
    if cur:
        blocks.append((name, cur))
    return blocks


def successors(blocks):
    idx = {n: i for i, (n, _) in enumerate(blocks)}
    succ = []
    for i, (_, ins) in enumerate(blocks):
        s = []
        last = ins[-1] if ins else ""
        m = BRANCH.match(last)
        if m and m.group(2) in idx:
            s.append(idx[m.group(2)])
        if not (last.startswith("s_branch") or last.startswith("s_endpgm") or last.startswith("s_setpc")) and i + 1 < len(blocks):
            s.append(i + 1)
        succ.append(s)
    return succ


def sccs(succ):
    """Tarjan, iterative; returns the components that are loops"""
    n = len(succ)
    index, low, on, stack, out, counter = [None] * n, [0] * n, [False] * n, [], [], [0]
    for root in range(n):
        if index[root] is not None:
            continue
        work = [(root, 0)]
        while work:
            v, pi = work.pop()
            if pi == 0:
                index[v] = low[v] = counter[0]
                counter[0] += 1
                stack.append(v)
                on[v] = True
            recurse = False
            for j in range(pi, len(succ[v])):
                w = succ[v][j]
                if index[w] is None:
                    work.append((v, j + 1))
                    work.append((w, 0))
                    recurse = True
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            if recurse:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    out.append(sorted(comp))
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return out


def reach_in_trip(loop, succ, header, b):
    """blocks of the loop reached from b before the header comes round again"""
    inside = set(loop) - {header}
    seen, todo = set(), [s for s in succ[b] if s in inside]
    while todo:
        v = todo.pop()
        if v in seen:
            continue
        seen.add(v)
        todo += [s for s in succ[v] if s in inside]
    return seen


def exceptional_exits(loop, succ, header, counts):
    arith = [b for b in loop if counts[b]["mad"]]
    reach = {b: reach_in_trip(loop, succ, header, b) for b in arith}
    last = [b for b in arith if not any(a in reach[b] for a in arith if a != b)]
    return {b for b in last if any(b in reach[a] and any(o in reach[a] for o in arith if o not in (a, b)) for a in arith if a != b)} \
        if len(arith) > 1 else set()


def count_block(ins):
    c = dict(total=len(ins), vector=0, mad=0, mov=0, cmp=0, mem=0)
    for l in ins:
        op = l.split()[0]
        if op.startswith(MEM):
            c["mem"] += 1
        elif op.startswith("v_"):
            c["vector"] += 1
            if op.startswith("v_mad_i64_i32"):
                c["mad"] += 1
            elif op.startswith("v_mov_"):
                c["mov"] += 1
            elif op.startswith("v_cmp"):
                c["cmp"] += 1
    return c


def cheapest_path(loop, succ, counts, src, dst):
    """the blocks after src, up to and including dst, on the way inside the loop with the fewest instructions (dst may be src: a cycle)"""
    import heapq
    inside = set(loop)
    done, heap = {}, [(counts[w]["total"], [w]) for w in succ[src] if w in inside]
    heapq.heapify(heap)
    while heap:
        cost, path = heapq.heappop(heap)
        v = path[-1]
        if v == dst:
            return path
        if v in done:
            continue
        done[v] = cost
        for w in succ[v]:
            if w in inside and w not in done:
                heapq.heappush(heap, (cost + counts[w]["total"], path + [w]))
    raise SystemExit("no path inside the loop")


def count_loop(asm, name):
    """{'kernel', 'blocks': [(name, counts, tag)], 'totals': counts of the common trip, 'all': counts of every block of the loop}
    tag: 'trip' (on the common trip), 'side' (a conditional block off it) or 'exit' (exceptional arithmetic)"""
    sym, body = kernel_body(asm, name)
    blocks = basic_blocks(body)
    succ = successors(blocks)
    counts = [count_block(ins) for _, ins in blocks]
    loops = sccs(succ)
    if not loops:
        raise SystemExit("kernel has no loop")
    loop = max(loops, key=lambda comp: sum(counts[b]["mad"] for b in comp))
    inside = set(loop)
    entered = [b for b in loop if any(b in succ[o] for o in range(len(blocks)) if o not in inside)]
    header = entered[0] if entered else loop[0]      # where the loop is entered from outside (block placement may put other blocks first)
    exits = exceptional_exits(loop, succ, header, counts)
    # the common trip: header -> every block of the ordinary arithmetic in turn -> header, by the cheapest way between them
    # (and the block that requests the next point: 16-byte loads, no store, ordinary arithmetic still to come in the same trip --
    # without it the cheapest way would walk past a prefetch that sits in a conditional block)
    arith = [b for b in loop if counts[b]["mad"] and b not in exits]
    def prefetch(b):
        ops = [l.split()[0] for l in blocks[b][1]]
        return any(o.startswith("global_load_dwordx4") for o in ops) and not any("store" in o for o in ops) \
            and any(a in reach_in_trip(loop, succ, header, b) for a in arith)
    stops = [b for b in loop if (b in arith or prefetch(b)) and b != header]
    trip, at = [header], header
    for stop in stops + [header]:
        leg = cheapest_path(loop, succ, counts, at, stop)
        trip += leg
        at = stop
    trip = trip[:-1]                       # the header once
    zero = dict(total=0, vector=0, mad=0, mov=0, cmp=0, mem=0)
    rows, totals, whole = [], dict(zero), dict(zero)
    for b in loop:
        tag = "exit" if b in exits else "trip" if b in trip else "side"
        rows.append((blocks[b][0], counts[b], tag))
        for k in zero:
            whole[k] += counts[b][k]
            if tag == "trip":
                totals[k] += counts[b][k]
    return {"kernel": sym, "blocks": rows, "totals": totals, "all": whole}


def render(res):
    fmt = "%-14s %7d %7d %14d %8d %8d %6d"
    out = [f"kernel {res['kernel']}", "%-14s %7s %7s %14s %8s %8s %6s" % ("block", "total", "vector", "v_mad_i64_i32", "v_mov_*", "v_cmp_*", "mem")]
    note = {"trip": "", "side": "   (conditional, off the common trip)", "exit": "   (exceptional arithmetic, off the common trip)"}
    for n, c, tag in res["blocks"]:
        out.append(fmt % (n, c["total"], c["vector"], c["mad"], c["mov"], c["cmp"], c["mem"]) + note[tag])
    for label, t in (("common trip", res["totals"]), ("whole loop", res["all"])):
        out.append(fmt % (label, t["total"], t["vector"], t["mad"], t["mov"], t["cmp"], t["mem"]))
    return "\n".join(out)


def main():
    args = sys.argv[1:]
    asm_file = None
    if "--asm" in args:
        i = args.index("--asm")
        asm_file = args[i + 1]
        del args[i:i + 2]
    defs = [a for a in args if a.startswith("-D")]
    pos = [a for a in args if not a.startswith("-D")]
    if len(pos) != 2:
        raise SystemExit(__doc__)
    if asm_file:
        asm = open(asm_file).read()
    else:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        from ark_plonk_amd import build
        asm = build.device_asm(pos[0], defs)
    print(f"unit {pos[0]} {' '.join(defs)}")
    print(render(count_loop(asm, pos[1])))


if __name__ == "__main__":
    main()
