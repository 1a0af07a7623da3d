"""Timings of PLONK verification over the IPA commitment on one GPU, three tables of JSON lines:

  segments   `msm.segments_msm` alone: 2 B segments of 32 and 10 terms (the aw and saw openings of B proofs) over 20 + 15 B bases,
             device events around the one launch
  verify     `IpaBatchVerifier.verify` of B proofs of one 2^--log-n-row circuit, whole and per stage: split (host), head stages (decode,
             replay, scalars x 2), combined commitments (the segmented MSM), L / R decode, host conversions, `batch_check`
  prepare    `IpaCommitterKey._prepare` of the 2 B openings next to the parent commit's way to the same C_j, one blocking
             `_msm_host` per opening, in the same process (the parent's whole `_prepare` is `tools/ipa_bench.py --batch-check` run on
             a checkout of the parent)

The batch is ONE real proof (prover.example_circuit) repeated B times: every stage does per proof what it does for distinct proofs.
Steady state: median, minimum and maximum of --reps runs after --warmup.  `verify` must return True for everything it times.

    python tools/ipa_verify_bench.py [--log-n 10] [--batches 1 64 1024 4096] [--reps 5] [--warmup 2] [--curve 0] [--out FILE]
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

TAU = 0x7A5C0DE
SEG_TERMS = (32, 10)                  # terms of the aw and of the saw opening's combined commitment


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def stats(xs):
    return {"median_ms": 1e3 * float(np.median(xs)), "min_ms": 1e3 * float(np.min(xs)), "max_ms": 1e3 * float(np.max(xs))}


def segments_lines(ctx, cid, batches, reps, warmup, key_xy):
    """segments_msm at the verifier's shape with random canonical scalars over real points"""
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd.msm import segments_msm
    cv = zk.get_curve(cid)
    rng = np.random.default_rng(5)
    out = []
    for B in batches:
        n_bases = 20 + 15 * B
        bases = key_xy[torch.arange(n_bases, device="cuda") % key_xy.shape[0]].contiguous()
        lens = np.tile(np.array(SEG_TERMS), B)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
        n_terms = int(lens.sum())
        index = torch.from_numpy(rng.integers(0, n_bases, size=n_terms).astype(np.int32)).cuda()
        sc = rng.integers(0, 1 << 62, size=(n_terms, 4), dtype=np.uint64)           # below 2^254: canonical on both curves
        d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
        ts = []
        for it in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            xy, inf, st = segments_msm(bases, None, off, index, d_sc, cid, ctx)
            e1.record()
            torch.cuda.synchronize()
            assert int(st.max()) == 0
            if it >= warmup:
                ts.append(e0.elapsed_time(e1) / 1e3)
        line = {"table": "segments", "curve": cv.name, "proofs": B, "segments": 2 * B, "terms": n_terms, "reps": reps, **stats(ts)}
        line["terms_per_s"] = n_terms / float(np.median(ts))
        print(json.dumps(line), flush=True)
        out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024, 4096])
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib, prover, transcript, verifier
    from ark_plonk_amd.curves import fq_from_mont, fr_to_mont, ints_to_limbs
    from ark_plonk_amd.ipa import IpaCommitterKey
    cid, lg = a.curve, a.log_n
    n = 1 << lg
    cv = zk.get_curve(cid)
    ctx = zk.Context(0)
    ca, cd = 0x1234567, 0x89ABCDE
    pk, wires, pub_m = prover.example_circuit(lg, cid, ctx, coeffs=(ca, cd))
    pw, x = [], 1
    for _ in range(n + 1):
        pw.append(x)
        x = x * TAU % cv.r
    d_pw = torch.from_numpy(ints_to_limbs(pw, 4).view(np.int64)).cuda()
    srs = torch.empty((n + 1, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, d_pw.data_ptr(), n + 1, srs.data_ptr()))
    torch.cuda.synchronize()
    h = tuple(fq_from_mont(cid, srs[n].cpu().numpy().view(np.uint64).reshape(2, -1)))
    ik = IpaCommitterKey(srs[:n].contiguous(), h, cid, ctx)
    vk = pk.verifier_key(ik.key)
    seed = lambda: transcript.seed_transcript(transcript.Transcript(b"ipa verify bench", cid), vk, n)      # noqa: E731
    ca_m, cd_m = fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0]
    t_prove, proof = timed(lambda: prover.prove(pk, ik, wires, pub_m, seed(), ca_m, cd_m))
    data = proof.to_bytes()
    print(json.dumps({"table": "prove", "curve": cv.name, "log_n": lg, "first_call_ms": 1e3 * t_prove, "proof_bytes": len(data)}), flush=True)
    lines = segments_lines(ctx, cid, a.batches, a.reps, a.warmup, srs)
    for B in a.batches:
        proofs, pis = [data] * B, [pub_m] * B
        routes = ["host"] + (["device"] if B >= 64 else [])
        for route in routes:
            v = verifier.IpaBatchVerifier(vk, n, seed(), ca_m, cd_m, ik, cid, ctx, replay=route)
            t = {k: [] for k in ("whole_s", "split_s", "head_s", "segments_s", "openings_s", "batch_check_s")}
            for it in range(a.warmup + a.reps):
                dt_w, ok = timed(lambda: v.verify(proofs, pis))
                assert ok
                dt_split, (shaped, parts, bad) = timed(lambda: v.split(proofs))
                dt_head, (pts, inf, rows, ch) = timed(lambda: v._stages(shaped, pis))
                dt_seg, _ = timed(lambda: v.combined_commitments(pts, inf, rows))
                dt_open, (ops, good, bad) = timed(lambda: v.openings(proofs, pis))          # stages 1-4 with the host conversions
                dt_bc, ok = timed(lambda: ik.batch_check(ops))
                assert ok and not bad
                if it >= a.warmup:
                    for k, x in zip(t, (dt_w, dt_split, dt_head, dt_seg, dt_open, dt_bc)):
                        t[k].append(x)
            line = {"table": "verify", "curve": cv.name, "log_n": lg, "proofs": B, "replay": route, "reps": a.reps}
            line.update({k.replace("_s", "_ms"): 1e3 * float(np.median(x)) for k, x in t.items()})
            line["whole_min_ms"], line["whole_max_ms"] = 1e3 * float(np.min(t["whole_s"])), 1e3 * float(np.max(t["whole_s"]))
            line["us_per_proof"] = 1e3 * line["whole_ms"] / B
            print(json.dumps(line), flush=True)
            lines.append(line)
        # _prepare of the 2 B openings: the segmented launch against the parent's one blocking MSM per opening
        t_new, t_seg, t_old = [], [], []
        for it in range(a.warmup + a.reps):
            dt_n, _ = timed(lambda: ik._prepare(ops, None, "blake2b"))
            dt_s, c_new = timed(lambda: ik._combined_commitments(ops))
            if B <= 1024 or it == a.warmup:
                dt_o, c_old = timed(lambda: [ik._msm_host(o.commitments, [1]) for o in ops])
                assert c_old == c_new
                t_old.append(dt_o)
            if it >= a.warmup:
                t_new.append(dt_n)
                t_seg.append(dt_s)
        line = {"table": "prepare", "curve": cv.name, "openings": 2 * B, "reps": a.reps, "prepare_ms": 1e3 * float(np.median(t_new)),
                "combined_commitments_ms": 1e3 * float(np.median(t_seg)), "msm_host_loop_ms": 1e3 * float(np.median(t_old)),
                "msm_host_loop_runs": len(t_old)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
