"""Timings of the IPA key derivation (ark_plonk_amd/ipa.py: sample_generators over csrc/ipa_setup.hip) on one GPU: per curve, digest
and n = 2^log_n generators, the candidate search and the cofactor kernel (the ctx's event profile), generators per second, the lane-slots
of square root the wavefronts ran per index (64 * sum(wave_rounds) / n: 2 is what the candidates need), and -- in the same run, as a
yardstick -- the per-point time of zk_g1_decompress_batch_dev at the same n: that kernel costs one square root and a 255-bit
multiplication per point.  Its input is the first 4096 derived generators, compressed on the host and repeated to n encodings.
Prints one JSON line per configuration; --out writes them to a file.

    python tools/ipa_setup_bench.py [--log-n 16 20 21] [--curves 0 1] [--digests blake2s blake2b] [--reps 3] [--warmup 1] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def profiled(ctx, names, fn):
    """kernel milliseconds by profile scope of one call of fn"""
    import torch
    torch.cuda.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    out = fn()
    torch.cuda.synchronize()
    ms = {k: ctx.profile_get(k)[0] for k in names}
    ctx.profile(False)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 21])
    ap.add_argument("--curves", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--digests", nargs="+", default=["blake2s", "blake2b"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import _lib, ipa
    ctx = zk.Context(0)
    lines = []
    for cid in a.curves:
        cv = zk.get_curve(cid)
        L = cv.fq_limbs
        for digest in a.digests:
            for lg in a.log_n:
                n = 1 << lg
                search, clear, slots = [], [], 0.0
                for k in range(a.warmup + a.reps):
                    ms, (xy, inf, tries, st, rounds) = profiled(ctx, ("h2c_search", "g1_clear_cofactor"),
                                                                lambda: ipa._sample_generators_raw(cv, n, 0, digest, ctx, 0))
                    assert int(st.max()) == 0
                    if k >= a.warmup:
                        search.append(ms["h2c_search"])
                        clear.append(ms["g1_clear_cofactor"])
                    slots = 64.0 * int(rounds.sum()) / n
                # the yardstick: decode n compressed points
                m = min(n, 4096)
                host = xy[:m].cpu().numpy().view(np.uint64)
                enc = b"".join(ipa.g1_compress(cv, tuple(zk.curves.fq_from_mont(cv, host[i].reshape(2, L)))) for i in range(m))
                d_in = torch.from_numpy(np.frombuffer(enc, dtype=np.uint8).copy()).cuda().repeat(n // m)
                d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
                dec = []
                for k in range(a.warmup + a.reps):
                    ms, _ = profiled(ctx, ("g1_decompress",), lambda: _lib.check(_lib.lib().zk_g1_decompress_batch_dev(
                        ctx.handle, cid, d_in.data_ptr(), n, xy.data_ptr(), inf.data_ptr(), d_st.data_ptr())))
                    assert int(d_st.max()) == 0
                    if k >= a.warmup:
                        dec.append(ms["g1_decompress"])
                s_ms, c_ms, d_ms = float(np.median(search)), float(np.median(clear)), float(np.median(dec))
                line = {"curve": cv.name, "digest": digest, "log_n": lg, "search_ms": s_ms, "cofactor_ms": c_ms,
                        "generators_per_s": n / ((s_ms + c_ms) / 1e3), "ns_per_generator": (s_ms + c_ms) * 1e6 / n,
                        "sqrt_lane_slots_per_index": slots, "attempts_per_index": float(tries.sum()) / n,
                        "decompress_ms": d_ms, "decompress_ns_per_point": d_ms * 1e6 / n, "reps": a.reps,
                        "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del xy, inf, tries, st, rounds, d_in, d_st
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
