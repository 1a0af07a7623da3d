"""Timings of lookup outputs on the device and of the reference's benchmark circuit (ark_plonk_amd/composer.py: LookupTable.lookup,
lookup_gate with c=None, bench_circuit; csrc/lookup_map.hip) on one GPU:

  * per table xor_table(0, bits) and per B: the map build (zk_lookup_map_build_dev, columns already on the device), B queries
    (`LookupTable.lookup`: zk_lookup_map_query_dev, its one read-back included) and the two kernels from the ctx's event profile;
    next to them, where the table fits a circuit of B rows, a circuit of B - 5 `lookup_gate(a, b, c=None, d)` calls (B rows with the composer's own):
    its witness replay (`Composer.assign`) and the lookup phase of `zk_circuit_check_dev` over it (check_lookup, and check_maps, which
    builds the W = 4 map of the table rows and the identity map) from the event profile;
  * `bench_circuit(log_n)`: building it, `compile`, one witness replay, the gather, `check_circuit`, and `prove` (lean and not);
  * --bench-py: `bench.py --gpus 1 --steps 20 --warmup 5` as a child process afterwards, its result line copied into the output, so
    that the figures above have the flagship workload of the same session next to them.

One JSON line per measurement; --out writes them to a file.  Every timed call ends in a device synchronise; the median of --reps calls
after --warmup calls is reported.  No threshold is asserted: there is no earlier device path to compare with.

    python tools/lookup_out_bench.py [--bits 8 10 12] [--log-b 16 18 20 22] [--bench-log-n 18 20] [--curve 0] [--reps 5] [--warmup 2]
                                     [--no-circuits] [--bench-py] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.gadget_bench import below, make_key, median_ms, timed  # noqa: E402


def profile_of(ctx, names):
    out = {}
    for ph in names:
        ms, cnt = ctx.profile_get(ph)
        if cnt:
            out[ph + "_ms"] = ms / cnt
    return out


def table_lines(zk, ctx, cid, coeffs, a, emit):
    import torch
    from ark_plonk_amd import _lib
    from ark_plonk_amd import compile as zc
    from ark_plonk_amd.composer import LookupTable
    from ark_plonk_amd.curves import fr_to_mont
    dev = torch.device("cuda", ctx.device)
    ca_m, cd_m = fr_to_mont(cid, [coeffs[0]])[0], fr_to_mont(cid, [coeffs[1]])[0]
    minus_one = torch.from_numpy(fr_to_mont(cid, [-1 % zk.get_curve(cid).r]).view(np.int64)).to(dev)
    for bits in a.bits:
        table = LookupTable.xor_table(0, bits)
        rows = table.size()
        cols = table.columns(cid, ctx, dev)
        slots = int(_lib.lib().zk_lookup_map_slots(rows))
        smap = torch.empty(slots, dtype=torch.int32, device=dev)

        def build():
            _lib.check(_lib.lib().zk_lookup_map_build_dev(ctx.handle, cid, cols[0].data_ptr(), cols[1].data_ptr(), cols[3].data_ptr(), rows,
                                                          smap.data_ptr(), slots))
        ctx.use_torch_stream()
        ctx.profile(True)
        ctx.profile_reset()
        build_ms = median_ms(build, a.reps, a.warmup)
        line = {"what": "map_build", "bits": bits, "rows": rows, "slots": slots, "map_bytes": 4 * slots, "build_ms": build_ms,
                **profile_of(ctx, ["lookup_map_build"])}
        ctx.profile(False)
        emit(line)
        del cols, smap
        for lb in a.log_b:
            B = 1 << lb
            xs, ys, ds = below(ctx, cid, B, bits, 10 + lb), below(ctx, cid, B, bits, 20 + lb), minus_one.repeat(B, 1)
            table.lookup(xs[:64].contiguous(), ys[:64].contiguous(), ds[:64].contiguous(), cid, ctx)      # the table's own map, built once
            ctx.profile(True)
            ctx.profile_reset()
            query_ms = median_ms(lambda: table.lookup(xs, ys, ds, cid, ctx), a.reps, a.warmup)
            line = {"what": "map_query", "bits": bits, "rows": rows, "queries": B, "query_ms": query_ms, **profile_of(ctx, ["lookup_map_query"])}
            ctx.profile(False)
            if a.no_circuits or rows > B:
                line["circuit"] = "not measured: " + ("--no-circuits" if a.no_circuits else "the table has more rows than the circuit")
                emit(line)
                continue
            c = zk.Composer(cid, ctx, coeffs=coeffs)
            c.lookup_table = table
            calls = B - 4 - 1                              # the composer's four rows and the row of the constant -1
            x, y = c.inputs(calls), c.inputs(calls)
            c.lookup_gate(x, y, None, c.add_witness_to_circuit_description(-1))
            desc = c.description()
            assert desc.size() == B
            ins = [xs[:calls].contiguous(), ys[:calls].contiguous()]
            ctx.profile(True)
            ctx.profile_reset()
            line["witness_replay_ms"] = median_ms(lambda: c.assign(ins), a.reps, a.warmup)
            line["witness_lookup_map_query_ms"] = profile_of(ctx, ["lookup_map_query"]).get("lookup_map_query_ms")
            ctx.profile(False)
            ck = make_key(ctx, cid, B, lb)
            pk, vk, pre = zc.compile(desc, ck, b"lookup out bench", cid, ctx)
            wires = zc.assign(desc, c.assign(ins), ctx)
            rep = zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx)
            assert rep.ok, str(rep)
            ctx.profile(True)
            ctx.profile_reset()
            line["check_circuit_ms"] = median_ms(lambda: zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx), a.reps, a.warmup)
            line.update({"check_" + k: v for k, v in profile_of(ctx, ["check_maps", "check_lookup"]).items()})
            ctx.profile(False)
            ck.close()
            emit(line)
            del c, desc, pk, vk, pre, wires, ins
            torch.cuda.empty_cache()
        del table
        torch.cuda.empty_cache()


def bench_circuit_lines(zk, ctx, cid, coeffs, a, emit):
    import torch
    from ark_plonk_amd import compile as zc
    from ark_plonk_amd import prover
    from ark_plonk_amd.composer import bench_circuit
    from ark_plonk_amd.curves import fr_to_mont
    ca_m, cd_m = fr_to_mont(cid, [coeffs[0]])[0], fr_to_mont(cid, [coeffs[1]])[0]
    for lg in a.bench_log_n:
        build_ms = median_ms(lambda: bench_circuit(lg, cid, ctx, coeffs).description(), a.reps, a.warmup)
        c = bench_circuit(lg, cid, ctx, coeffs)
        desc = c.description()
        assert desc.size() == 1 << lg and c.n_gates == (1 << (lg - 1)) + 2
        line = {"what": "bench_circuit", "log_n": lg, "rows": c.n_gates, "vars": c.num_vars, "build_ms": build_ms,
                "witness_replay_ms": median_ms(lambda: c.assign([]), a.reps, a.warmup)}
        ck = make_key(ctx, cid, 1 << lg, lg)
        t, (pk, vk, pre) = timed(lambda: zc.compile(desc, ck, b"bench circuit", cid, ctx))
        line["compile_ms"] = t * 1e3
        values = c.assign([])
        line["gather_ms"] = median_ms(lambda: zc.assign(desc, values, ctx), a.reps, a.warmup)
        wires = zc.assign(desc, values, ctx)
        rep = zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx)
        assert rep.ok, str(rep)
        line["check_circuit_ms"] = median_ms(lambda: zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx), a.reps, a.warmup)
        line["prove_ms"] = median_ms(lambda: prover.prove(pk, ck, wires, {}, pre, ca_m, cd_m), a.reps, a.warmup)
        line["prove_lean_ms"] = median_ms(lambda: prover.prove(pk, ck, wires, {}, pre, ca_m, cd_m, lean=True), a.reps, a.warmup)
        ck.close()
        emit(line)
        del c, desc, pk, vk, pre, wires, values
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="*", default=[8, 10, 12])
    ap.add_argument("--log-b", type=int, nargs="*", default=[16, 18, 20, 22])
    ap.add_argument("--bench-log-n", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-circuits", action="store_true", help="skip the circuits next to the standalone queries (compile at every B)")
    ap.add_argument("--bench-py", action="store_true", help="run bench.py --gpus 1 --steps 20 --warmup 5 afterwards, as a child process")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ark_plonk_amd as zk
    from tests import composer_ref as cr            # the embedded curves' coefficients
    cid = a.curve
    name = zk.get_curve(cid).name
    _, ca, cd = cr.EMBEDDED[name]
    ctx = zk.Context(0)
    lines = []

    def emit(line):
        line = {"curve": name, "reps": a.reps, **line}
        print(json.dumps(line), flush=True)
        lines.append(line)
    table_lines(zk, ctx, cid, (ca, cd), a, emit)
    bench_circuit_lines(zk, ctx, cid, (ca, cd), a, emit)
    ctx.close()
    if a.bench_py:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True)
        tail = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        line = {"what": "bench.py", "returncode": r.returncode, "result": json.loads(tail[-1]) if tail else None}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
