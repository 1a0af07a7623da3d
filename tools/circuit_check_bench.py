"""Timings of the circuit check (ark_plonk_amd/circuit_check.py) on one GPU against a proof of the same circuit in the same process:
the whole `check_circuit` (eleven selector NTTs + zk_circuit_check_dev), the C call alone with its phases from the ctx's event profile,
and one `prover.prove`.  The circuit is `prover.example_circuit` (every gate kind, lookups, copy constraints; satisfied).
Prints one JSON line per size; --out writes them to a file.  Kernel times for the record come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (add --no-prove --reps 3 there to keep the trace short; --prove-only gives the
quotient kernel's time for the same size).

    python tools/circuit_check_bench.py [--log-n 18 20 22] [--curve 0] [--reps 10] [--warmup 2] [--no-prove | --prove-only] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ("check_gates", "check_maps", "check_copy", "check_lookup", "check_summary")


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def make_key(ctx, cid, n, seed):
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    cv = zk.get_curve(cid)
    sc = np.random.default_rng(seed).integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    pts = torch.empty((n, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, d_sc.data_ptr(), n, pts.data_ptr()))
    return zk.CommitterKey(pts, cid, ctx).precompute()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[18, 20, 22])
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-prove", action="store_true")
    ap.add_argument("--prove-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import circuit_check, prover, transcript
    from ark_plonk_amd.curves import fr_to_mont
    cid = a.curve
    ctx = zk.Context(0)
    ca, cd = fr_to_mont(cid, [1])[0], fr_to_mont(cid, [1])[0]
    med = lambda v: float(np.median(v)) * 1e3  # noqa: E731
    lines = []
    for lg in a.log_n:
        n = 1 << lg
        pk, wires, pub = prover.example_circuit(lg, cid, ctx)
        line = {"curve": zk.get_curve(cid).name, "log_n": lg, "reps": a.reps}
        if not a.prove_only:
            t_all, t_call = [], []
            prof = dict.fromkeys(PHASES, 0.0)
            for it in range(a.warmup + a.reps):
                t, rep = timed(lambda: zk.check_circuit(pk, wires, pub, ca, cd, ctx=ctx))
                assert rep.ok
                if it >= a.warmup:
                    t_all.append(t)
            sel = circuit_check.selector_evaluations(pk)
            pi = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
            for pos, v in pub.items():
                pi[pos] = torch.from_numpy(np.asarray(v, dtype=np.uint64).view(np.int64)).cuda()
            call = lambda: circuit_check.check_columns(zk.get_curve(cid), lg, wires, sel, pk.sigma_evals, pk.table_cols, n, pi, ca, cd, ctx)  # noqa: E731
            for it in range(a.warmup + a.reps):
                keep = it >= a.warmup
                ctx.profile(True)
                ctx.profile_reset()
                t, _ = timed(call)
                if keep:
                    t_call.append(t)
                    for k in PHASES:
                        prof[k] += ctx.profile_get(k)[0] / a.reps
                ctx.profile(False)
            del sel, pi
            line.update({"check_circuit_ms": med(t_all), "c_call_ms": med(t_call), **{k + "_ms": v for k, v in prof.items()}})
        if not a.no_prove:
            ck = make_key(ctx, cid, n, lg)
            vk = pk.verifier_key(ck)
            pre = transcript.seed_transcript(transcript.Transcript(b"bench", cid), vk, n)
            t_prove = []
            for it in range(1 + 3):
                t, _ = timed(lambda: prover.prove(pk, ck, wires, pub, pre, ca, cd))
                if it >= 1:
                    t_prove.append(t)
            line["prove_ms"] = med(t_prove)
            if "check_circuit_ms" in line:
                line["check_share_of_prove"] = line["check_circuit_ms"] / line["prove_ms"]
            ck.close()
        print(json.dumps(line), flush=True)
        lines.append(line)
        del pk, wires
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
