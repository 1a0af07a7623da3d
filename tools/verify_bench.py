"""Timings of the batch verifier (ark_plonk_amd/verifier.py) on one GPU: B proofs of one 2^14-row circuit folded to the two pairing
inputs, wall time per stage -- point decode (device), parse + transcript replay (host, serial; or on the device, upload included),
per-proof scalars (device), fold (column sum + three MSMs + host sum) -- and of the whole `BatchVerifier.fold` by either route
(--replay host device): with the host replay the decode overlaps it, with the device replay everything is queued behind one upload.
The batch is ONE real proof (prover.example_circuit, every widget in it) repeated B times under distinct weights: every stage does per
proof exactly what it does for distinct proofs.  The SRS is synthetic with a known tau, so the tool checks what it timed, for every
route: tau L == R.  Steady state: median, minimum and maximum of --reps runs after --warmup, the routes taking turns inside every
run.  Prints one JSON line per (B, route); --out writes them to a file.

    python tools/verify_bench.py [--log-n 14] [--batches 1 8 16 32 64 128 256 1024 4096] [--replay host device] [--reps 5] [--warmup 2]
                                 [--curve 0] [--out FILE]
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
REFERENCE_VERIFY_MS = 8.15            # the reference's README, one proof at 2^18 on its authors' CPU: for the reader, not a criterion


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def affine_mul(cv, k, P):
    """k * P on y^2 = x^3 + b over Python integers (None: infinity): the one check of the result, not a compute path"""
    q = cv.q

    def plus(p1, p2):
        if p1 is None:
            return p2
        if p2 is None:
            return p1
        (x1, y1), (x2, y2) = p1, p2
        if x1 == x2:
            if (y1 + y2) % q == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, q) % q
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, q) % q
        x3 = (lam * lam - x1 - x2) % q
        return x3, (lam * (x1 - x3) - y1) % q

    acc = None
    while k:
        if k & 1:
            acc = plus(acc, P)
        P = plus(P, P)
        k >>= 1
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=14)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 16, 32, 64, 128, 256, 1024, 4096])
    ap.add_argument("--replay", nargs="+", choices=("host", "device"), default=["host", "device"], help="where stage 2 runs")
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib, prover, transcript, verifier
    from ark_plonk_amd.curves import fq_from_mont, fr_to_mont, ints_to_limbs
    cid, lg = a.curve, a.log_n
    n = 1 << lg
    cv = zk.get_curve(cid)
    ctx = zk.Context(0)
    # a proof of a circuit with every widget, over tau^i G
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
    seed = lambda: transcript.seed_transcript(transcript.Transcript(b"verify bench", cid), vk, n)      # noqa: E731
    ca_m, cd_m = fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0]
    data = prover.prove(pk, ck, wires, pub_m, seed(), ca_m, cd_m).to_bytes()
    bvs = {mode: zk.BatchVerifier(vk, n, seed(), ca_m, cd_m, cid, ctx, replay=mode) for mode in a.replay}
    seeded = seed()
    point = lambda P: None if P.infinity else (fq_from_mont(cid, P.x.reshape(1, -1))[0], fq_from_mont(cid, P.y.reshape(1, -1))[0])   # noqa: E731
    lines = []
    for B in a.batches:
        proofs, pis = [data] * B, [pub_m] * B
        # the stages of the host route one by one; of the device route its stage 2 (one upload + the kernel); the whole fold of each
        stages = {"host": {k: [] for k in ("gather_s", "decode_s", "replay_s", "scalars_s", "register_s", "fold_s", "whole_s")},
                  "device": {k: [] for k in ("replay_s", "fold_s", "whole_s")}}
        last = {}
        for it in range(a.warmup + a.reps):
            ws = bvs[a.replay[0]].random_weights(B)
            for mode in a.replay:
                bv = bvs[mode]
                if mode == "host":
                    t_g, enc = timed(lambda: verifier.proof_point_bytes(proofs, cid))
                    t_d, (pts, inf, pst) = timed(lambda: verifier.decompress_batch(enc, cid, ctx))
                    t_r, (ch, ev, parse_st) = timed(lambda: verifier.replay_batch(seeded, proofs, pis, cid))
                    t_s, rows = timed(lambda: verifier.scalar_rows(lg, ch, ev, pis, ca_m, cd_m, ws, parse_st, pst, cid, ctx))
                    assert not rows[3].any()
                    # the two registrations of the decoded points as MSM bases are inside the whole; timed here on their own
                    t_reg, cks = timed(lambda: (zk.CommitterKey(pts, cid, ctx, infinity=inf), ))
                    cks[0].close()
                    t = {"gather_s": t_g, "decode_s": t_d, "replay_s": t_r, "scalars_s": t_s, "register_s": t_reg}
                else:
                    t_r, dev_rows = timed(lambda: verifier.replay_batch_dev(seeded, proofs, pis, cid, ctx))
                    assert not dev_rows[3].any()
                    t = {"replay_s": t_r}
                t["whole_s"], (L, R, st) = timed(lambda: bv.fold(proofs, pis, ws))
                t["fold_s"], (L2, R2) = timed(lambda: bv.fold_range(0, B))
                assert L2 == L and R2 == R and not st.any()
                last[mode] = (L, R)
                if it >= a.warmup:
                    for k, v in t.items():
                        stages[mode][k].append(v)
        for mode in a.replay:
            L, R = last[mode]
            assert affine_mul(cv, TAU, point(L)) == point(R), f"{mode} replay: the folded pair does not satisfy tau L == R"
        assert len({(point(L), point(R)) for L, R in last.values()}) == 1, "the two routes fold the same weights to different pairs"
        for mode in a.replay:
            v = stages[mode]
            med = {k: float(np.median(x)) for k, x in v.items()}
            line = {"curve": cv.name, "log_n": lg, "B": B, "replay": mode, **med, "min": {k: float(min(x)) for k, x in v.items()},
                    "max": {k: float(max(x)) for k, x in v.items()}, "per_proof_ms": med["whole_s"] / B * 1e3,
                    "replay_share_of_whole": med["replay_s"] / med["whole_s"], "proof_bytes": len(data), "reps": a.reps,
                    "reference_single_verify_ms": REFERENCE_VERIFY_MS}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    for bv in bvs.values():
        bv.close()
    ctx.close()


if __name__ == "__main__":
    main()
