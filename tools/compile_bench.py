"""Timings of circuit compilation (ark_plonk_amd/compile.py) on one GPU: zk_perm_sigma_dev alone (wall clock and its three phases
from the ctx's event profile), the key's transforms, the 16 + 4 commitments, the whole `compile`, and `assign`, per size and curve.
The circuit is synthetic: n gates, 40 % of all wire cells on variable 0, the rest on n random variables, a table of n / 4 rows.
Prints one JSON line per configuration; --out writes them to a file.  Kernel times for the record come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/compile_bench.py [--log-n 18 20 22] [--curves 0 1] [--reps 3] [--warmup 1] [--out FILE]
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

PHASES = ("perm_sigma_sort", "perm_sigma_rotate", "perm_sigma_encode")


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
    ap.add_argument("--curves", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import compile as zc
    from ark_plonk_amd.prover import SELECTORS, ProverKey
    ctx = zk.Context(0)
    lines = []
    for cid in a.curves:
        cv = zk.get_curve(cid)
        for lg in a.log_n:
            n = 1 << lg
            g = torch.Generator(device="cuda").manual_seed(lg)
            ids = torch.randint(1, n, (4, n), device="cuda", generator=g, dtype=torch.int64)
            ids[torch.rand((4, n), device="cuda", generator=g) < 0.4] = 0

            def rnd(rows):
                t = torch.randint(0, 1 << 62, (rows, 4), dtype=torch.int64, device="cuda", generator=g)
                t[:, 3] &= (1 << 60) - 1
                return t
            desc = zc.CircuitDescription.from_gates({k: rnd(n) for k in SELECTORS}, *ids, num_vars=n, table_cols=[rnd(n // 4) for _ in range(4)],
                                                    curve=cid)
            vals = rnd(n)
            vals[0] = 0
            ck = make_key(ctx, cid, n, lg)
            dom = zk.Radix2EvaluationDomain.new(n, cid, ctx)
            dom4 = zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
            t_sigma, t_tr, t_commit, t_compile, t_assign = [], [], [], [], []
            prof = dict.fromkeys(PHASES, 0.0)
            for it in range(a.warmup + a.reps):
                keep = it >= a.warmup
                ctx.profile(True)
                ctx.profile_reset()
                t, sig = timed(lambda: zc.sigma_evals(dom, desc.ins_var, desc.ins_pos, desc.num_vars, ctx))
                if keep:
                    t_sigma.append(t)
                    for k in PHASES:
                        prof[k] += ctx.profile_get(k)[0] / a.reps
                ctx.profile(False)
                t, pk = timed(lambda: ProverKey(dom, dom4, desc.selectors, sig, [zc._pad_rows(c, n, True) for c in desc.table_cols]))
                if keep:
                    t_tr.append(t)

                def rounds():
                    ck.commit_begin([pk.polys[k] for k in SELECTORS] + list(pk.sigma_polys))
                    first = ck.round_end(16)
                    ck.commit_begin(dom.batch(1, pk.table_cols))
                    return first + ck.round_end(4)
                t, _ = timed(rounds)
                if keep:
                    t_commit.append(t)
                del pk, sig
                t, out = timed(lambda: zc.compile(desc, ck, b"bench", cid, ctx))
                if keep:
                    t_compile.append(t)
                del out
                t, w = timed(lambda: zc.assign(desc, vals, ctx))
                if keep:
                    t_assign.append(t)
                del w
            med = lambda v: float(np.median(v))  # noqa: E731
            line = {"curve": cv.name, "log_n": lg, "sigma_s": med(t_sigma), **{k + "_s": v / 1e3 for k, v in prof.items()},
                    "transforms_s": med(t_tr), "commit_rounds_20_s": med(t_commit), "compile_s": med(t_compile), "assign_s": med(t_assign),
                    "sigma_share_of_compile": med(t_sigma) / med(t_compile), "reps": a.reps}
            print(json.dumps(line), flush=True)
            lines.append(line)
            ck.close()
            del desc, vals, ids
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
