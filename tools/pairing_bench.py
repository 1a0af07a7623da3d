"""Timings of the KZG pairing check, three tables of JSON lines:

  host       `PairingKey.check` and `PairingKey.gt` on the host, ms per call, both curves (no GPU in the timed window)
  batch      `PairingKey.check_batch` at n = 64, 1024, 16384 valid pairs, both curves: device events around the one launch, checks/s
  verdicts   on a 2^--log-n-row circuit at B = --batch proofs with k = 0, 1, 8 of them invalid (one evaluation changed):
             `BatchVerifier.verdicts` (one segmented MSM + one launch of B checks) against `BatchVerifier.locate_invalid` with the
             host pairing (a bisection: 1 + up to 2 k ceil(log2 B) folds and host checks), each whole, prepare included; both must
             name exactly the k changed proofs

The batch is ONE real proof (prover.example_circuit) repeated, as in tools/verify_bench.py.  Steady state: median, minimum and maximum
of --reps runs after --warmup.

    python tools/pairing_bench.py [--tables host batch verdicts] [--log-n 14] [--batch 1024] [--reps 5] [--warmup 2] [--out FILE]
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
CURVES = ("bls12_381", "bn254")


def stats(xs):
    return {"median_ms": 1e3 * float(np.median(xs)), "min_ms": 1e3 * float(np.min(xs)), "max_ms": 1e3 * float(np.max(xs))}


def g1(cv, k):
    from ark_plonk_amd.curves import fq_to_mont, g1_mul
    from ark_plonk_amd.msm import G1Affine
    m = fq_to_mont(cv, list(g1_mul(cv, k)))
    return G1Affine(m[0], m[1], False, cv.name)


def host_lines(reps, warmup):
    import ark_plonk_amd as zk
    from ark_plonk_amd.pairing import PairingKey
    out = []
    for name in CURVES:
        cv = zk.get_curve(name)
        t0 = time.perf_counter()
        key = PairingKey.from_trapdoor(TAU, name)
        t_key = time.perf_counter() - t0                      # g2_mul in Python included
        L, R = g1(cv, 0xC0FFEE), g1(cv, 0xC0FFEE * TAU)
        tc, tg = [], []
        for it in range(warmup + reps * 4):
            t0 = time.perf_counter()
            ok = key.check(L, R)
            t1 = time.perf_counter()
            key.gt(L, 1)
            t2 = time.perf_counter()
            assert ok
            if it >= warmup:
                tc.append(t1 - t0)
                tg.append(t2 - t1)
        line = {"table": "host", "curve": name, "check": stats(tc), "gt": stats(tg), "key_from_trapdoor_ms": 1e3 * t_key, "calls": len(tc)}
        print(json.dumps(line), flush=True)
        out.append(line)
        key.close()
    return out


def batch_lines(ctx, sizes, reps, warmup):
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib
    from ark_plonk_amd.curves import ints_to_limbs
    from ark_plonk_amd.pairing import PairingKey
    out = []
    for name in CURVES:
        cv = zk.get_curve(name)
        key = PairingKey.from_trapdoor(TAU, name)
        for n in sizes:
            rng = np.random.default_rng(n)
            ks = [int.from_bytes(rng.bytes(31), "little") % cv.r or 1 for _ in range(n)]
            pts = []
            ctx.use_torch_stream()
            for scal in (ks, [k * TAU % cv.r for k in ks]):         # L_j = k_j G, R_j = tau k_j G: every check is valid
                d = torch.from_numpy(ints_to_limbs(scal, 4).view(np.int64)).cuda()
                xy = torch.empty((n, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
                _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cv.curve_id, d.data_ptr(), n, xy.data_ptr()))
                pts.append(xy)
            ts = []
            for it in range(warmup + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ok = key.check_batch(pts[0], None, pts[1], None, ctx)
                e1.record()
                torch.cuda.synchronize()
                assert bool(ok.all())
                if it >= warmup:
                    ts.append(e0.elapsed_time(e1) / 1e3)
            bad = key.check_batch(pts[0], None, pts[0], None, ctx)   # tau != 1: every one of these is invalid
            assert not bool(bad.any())
            line = {"table": "batch", "curve": name, "n": n, "reps": reps, **stats(ts), "checks_per_s": n / float(np.median(ts))}
            print(json.dumps(line), flush=True)
            out.append(line)
        key.close()
    return out


def verdict_lines(ctx, lg, B, ks, reps, warmup, cid=0):
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib, prover, transcript
    from ark_plonk_amd.curves import fr_to_mont, ints_to_limbs
    from ark_plonk_amd.pairing import PairingKey
    cv = zk.get_curve(cid)
    n = 1 << lg
    ca, cd = 0x1234567, 0x89ABCDE
    pk, wires, pub_m = prover.example_circuit(lg, cid, ctx, coeffs=(ca, cd))
    pw, x = [], 1
    for _ in range(n + 8):
        pw.append(x)
        x = x * TAU % cv.r
    d_pw = torch.from_numpy(ints_to_limbs(pw, 4).view(np.int64)).cuda()
    srs = torch.empty((n + 8, 2 * cv.fq_limbs), dtype=torch.int64, device="cuda")
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_g1_fixed_base_batch_dev(ctx.handle, cid, d_pw.data_ptr(), n + 8, srs.data_ptr()))
    ck = zk.CommitterKey(srs, cid, ctx)
    vk = pk.verifier_key(ck)
    seed = lambda: transcript.seed_transcript(transcript.Transcript(b"pairing bench", cid), vk, n)      # noqa: E731
    ca_m, cd_m = fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0]
    data = prover.prove(pk, ck, wires, pub_m, seed(), ca_m, cd_m).to_bytes()
    g, f = 8 * cv.fq_limbs, 32
    o = 15 * g + 2 + 2 * f                                    # the third evaluation, plus one
    v = (int.from_bytes(data[o:o + f], "little") + 1) % cv.r
    bad_data = data[:o] + v.to_bytes(f, "little") + data[o + f:]
    key = PairingKey.from_trapdoor(TAU, cv)
    bv = zk.BatchVerifier(vk, n, seed(), ca_m, cd_m, cid, ctx, pairing_key=key)
    out = []
    for k in ks:
        where = sorted({(j * B) // k + (B // (2 * k)) for j in range(k)}) if k else []
        proofs = [bad_data if j in where else data for j in range(B)]
        pis = [pub_m] * B
        tv, tl, tf = [], [], []
        n_checks = 0
        for it in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = bv.verdicts(proofs, pis)
            t1 = time.perf_counter()
            calls = []

            def accepts(L, R):
                calls.append(1)
                return key.check(L, R)
            loc = bv.locate_invalid(proofs, pis, accepts)
            t2 = time.perf_counter()
            yes = bv.verify(proofs, pis)
            t3 = time.perf_counter()
            assert np.nonzero(~got)[0].tolist() == where == loc and yes == (k == 0)
            n_checks = len(calls)
            if it >= warmup:
                tv.append(t1 - t0)
                tl.append(t2 - t1)
                tf.append(t3 - t2)
        line = {"table": "verdicts", "curve": cv.name, "log_n": lg, "B": B, "invalid": k, "reps": reps, "verdicts": stats(tv),
                "locate_invalid": stats(tl), "verify": stats(tf), "host_checks_of_the_bisection": n_checks,
                "verdicts_over_locate": float(np.median(tv)) / float(np.median(tl))}
        print(json.dumps(line), flush=True)
        out.append(line)
    bv.close()
    key.close()
    ck.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="+", choices=("host", "batch", "verdicts"), default=["host", "batch", "verdicts"])
    ap.add_argument("--log-n", type=int, default=14)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--invalid", type=int, nargs="+", default=[0, 1, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    if "host" in a.tables:
        lines += host_lines(a.reps, a.warmup)
    if "batch" in a.tables or "verdicts" in a.tables:
        import ark_plonk_amd as zk
        ctx = zk.Context(0)
        if "batch" in a.tables:
            lines += batch_lines(ctx, a.sizes, a.reps, a.warmup)
        if "verdicts" in a.tables:
            lines += verdict_lines(ctx, a.log_n, a.batch, a.invalid, a.reps, a.warmup)
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
