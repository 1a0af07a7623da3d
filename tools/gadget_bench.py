"""Timings of the device composer (ark_plonk_amd/composer.py, csrc/gadget_layout.hip, csrc/gadget_witness.hip) on one GPU:

  * per gadget kind, one segment of B calls: the layout call (zk_gadget_layout_dev) and the witness call (zk_gadget_witness_dev), the
    two phases of the fixed-base witness (gadget_w_fixed_walk, gadget_w_fixed_norm) and gadget_w_curve from the ctx's event profile;
  * a program that fills n = 2^log_n rows with every kind (half of the rows fixed-base products, a quarter range gates, an eighth logic gates,
    the rest curve additions and arithmetic): building it (every layout call + `description()`), one witness replay (`Composer.assign`), and --
    in the same process, on the same circuit -- `compile`, one `check_circuit` and one `prove`.

  * --ext: two more kinds -- `variable_base_scalar_mul` at B = 1, 64, 4096 and `is_zero_with_output` at B = 2^20: layout, witness, the
    kernels of the variable-base witness (gadget_w_var_bits, gadget_w_var_walk, gadget_w_var_norm) and gadget_w_is_zero from the event
    profile, and, where the circuit pads to at most 2^--ext-prove-log-n rows, `compile` and one `prove` of the same circuit.

One JSON line per measurement; --out writes them to a file.  Every timed call ends in a device synchronise; the median of --reps calls
after --warmup calls is reported.  Kernel times for the record come from a separate `rocprofv3 --kernel-trace --stats` run of this
script (add --no-prove --reps 3 there to keep the trace short).

    python tools/gadget_bench.py [--log-n 18 20 22] [--curve 0] [--reps 5] [--warmup 1] [--no-kinds] [--no-prove] [--out FILE]
                                 [--ext] [--ext-calls 1 64 4096] [--ext-prove-log-n 21]
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


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def median_ms(fn, reps, warmup):
    ts = [timed(fn)[0] for _ in range(warmup + reps)][warmup:]
    return float(np.median(ts)) * 1e3


def below(ctx, cid, rows, bits, seed):
    """`rows` Montgomery elements whose canonical value is a random integer below 2^bits (bits <= 250): random words, the top ones
    masked, through zk_fr_to_mont_dev"""
    import torch
    from ark_plonk_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(0, 1 << 62, (rows, 4), dtype=torch.int64, device="cuda", generator=g)
    for k in range(4):
        keep = min(max(bits - 64 * k, 0), 62)
        t[:, k] &= (1 << keep) - 1
    out = torch.empty_like(t)
    ctx.use_torch_stream()
    _lib.check(_lib.lib().zk_fr_to_mont_dev(ctx.handle, cid, t.data_ptr(), rows, out.data_ptr()))
    return out


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


def kinds(zk, ctx, cid, coeffs, G, a, emit):
    """one segment per kind on a fresh composer: layout, then the witness"""
    cases = [("arithmetic", 1 << 20, lambda c, x, y: c.arithmetic_gate(x, y, q_m=3, q_l=5, q_r=7, q_c=9)),
             ("range_64", 1 << 16, lambda c, x, y: c.range_gate(x, 64)),
             ("xor_64", 1 << 16, lambda c, x, y: c.xor_gate(x, y, 64)),
             ("fixed_base", 4096, lambda c, x, y: c.fixed_base_scalar_mul(x, G)),
             ("fixed_base_then_add", 4096, lambda c, x, y: c.point_addition_gate(*[c.fixed_base_scalar_mul(x, G)] * 2))]
    for name, B, fn in cases:
        def build():
            c = zk.Composer(cid, ctx, coeffs=coeffs)
            x, y = c.inputs(B), c.inputs(B)
            fn(c, x, y)
            return c
        layout_ms = median_ms(build, a.reps, a.warmup)
        c = build()
        xs, ys = below(ctx, cid, B, 64, 1), below(ctx, cid, B, 64, 2)
        ctx.profile(True)
        ctx.profile_reset()
        witness_ms = median_ms(lambda: c.assign([xs, ys]), a.reps, a.warmup)
        line = {"what": "kind", "kind": name, "calls": B, "rows": c.n_gates, "vars": c.num_vars, "layout_ms": layout_ms, "witness_ms": witness_ms}
        for ph in ("gadget_w_fixed_walk", "gadget_w_fixed_norm", "gadget_w_curve"):
            ms, cnt = ctx.profile_get(ph)
            if cnt:
                line[ph + "_ms"] = ms / cnt
        ctx.profile(False)
        emit(line)


def ext_kinds(zk, ctx, cid, coeffs, G, a, emit):
    """--ext: one segment per case on a fresh composer -- layout, witness, and compile + prove of that circuit"""
    from ark_plonk_amd import compile as zc
    from ark_plonk_amd import prover
    from ark_plonk_amd.curves import fr_to_mont
    ca_m, cd_m = fr_to_mont(cid, [coeffs[0]])[0], fr_to_mont(cid, [coeffs[1]])[0]
    gx, gy = (fr_to_mont(cid, [v])[0].view(np.int64) for v in G)
    cases = [("variable_base", B) for B in a.ext_calls] + [("is_zero", 1 << 20)]
    for name, B in cases:
        def build():
            c = zk.Composer(cid, ctx, coeffs=coeffs)
            x = c.inputs(B)
            if name == "variable_base":
                c.variable_base_scalar_mul(x, (c.inputs(B), c.inputs(B)))
            else:
                c.is_zero_with_output(x)
            return c
        import torch
        layout_ms = median_ms(build, a.reps, a.warmup)
        c = build()
        ins = [below(ctx, cid, B, 250, 5)]
        if name == "variable_base":
            ins += [torch.from_numpy(col).cuda().reshape(1, 4).repeat(B, 1) for col in (gx, gy)]
        ctx.profile(True)
        ctx.profile_reset()
        witness_ms = median_ms(lambda: c.assign(ins), a.reps, a.warmup)
        line = {"what": "ext_kind", "kind": name, "calls": B, "rows": c.n_gates, "vars": c.num_vars, "layout_ms": layout_ms, "witness_ms": witness_ms}
        for ph in ("gadget_w_var_bits", "gadget_w_var_walk", "gadget_w_var_norm", "gadget_w_is_zero"):
            ms, cnt = ctx.profile_get(ph)
            if cnt:
                line[ph + "_ms"] = ms / cnt
        ctx.profile(False)
        desc = c.description()
        n = desc.size()
        if not a.no_prove and 32 <= n <= 1 << a.ext_prove_log_n:
            ck = make_key(ctx, cid, n, 77)
            t, (pk, vk, pre) = timed(lambda: zc.compile(desc, ck, b"bench", cid, ctx))
            line["log_n"], line["compile_ms"] = n.bit_length() - 1, t * 1e3
            wires = zc.assign(desc, c.assign(ins), ctx)
            rep = zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx)
            assert rep.ok, str(rep)
            line["prove_ms"] = median_ms(lambda: prover.prove(pk, ck, wires, {}, pre, ca_m, cd_m), 3, 1)
            line["witness_share_of_prove"] = witness_ms / line["prove_ms"]
            ck.close()
            del pk, vk, wires
        emit(line)
        del c, desc, ins
        torch.cuda.empty_cache()


def fill(zk, ctx, cid, coeffs, G, lg):
    """a composer whose circuit pads to 2^lg rows, and its input tensors"""
    n = 1 << lg
    c = zk.Composer(cid, ctx, coeffs=coeffs)
    M = c.m_bits
    Bf, Br, Bl = (n // 2) // (M + 5), (n // 4) // 10, (n // 16) // 33
    e, x, y = c.inputs(Bf), c.inputs(Br), c.inputs(Bl)
    pt = c.fixed_base_scalar_mul(e, G)
    c.point_addition_gate(c.point_addition_gate(pt, pt), pt)
    c.range_gate(x, 64)
    z = c.xor_gate(y, x[:Bl].clone(), 64)
    c.and_gate(z, y, 64)
    Ba = (n - 64 - c.n_gates) // 3                    # three arithmetic segments follow
    s = c.arithmetic_gate(x[:1].clone(), y[:1].clone(), q_m=3, q_l=5, q_r=7, q_c=9, B=Ba)
    c.boolean_gate(c.arithmetic_gate(s, 0, q_l=0, q_c=1))
    ins = [below(ctx, cid, Bf, 250, lg), below(ctx, cid, Br, 64, lg + 1), below(ctx, cid, Bl, 64, lg + 2)]
    return c, ins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="*", default=[18, 20, 22])
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-kinds", action="store_true")
    ap.add_argument("--no-prove", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--ext", action="store_true", help="also time variable_base_scalar_mul (at --ext-calls) and is_zero_with_output")
    ap.add_argument("--ext-calls", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--ext-prove-log-n", type=int, default=21)
    a = ap.parse_args()
    import torch
    import ark_plonk_amd as zk
    from ark_plonk_amd import compile as zc
    from ark_plonk_amd import prover
    from ark_plonk_amd.curves import fr_to_mont
    from tests import composer_ref as cr            # the embedded curves' coefficients and a base point solved from the curve equation
    cid = a.curve
    name = zk.get_curve(cid).name
    p, ca, cd = cr.EMBEDDED[name]
    G = cr.te_point(p, ca, cd)
    ctx = zk.Context(0)
    lines = []

    def emit(line):
        line = {"curve": name, "reps": a.reps, **line}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if not a.no_kinds:
        kinds(zk, ctx, cid, (ca, cd), G, a, emit)
    if a.ext:
        ext_kinds(zk, ctx, cid, (ca, cd), G, a, emit)
    ca_m, cd_m = fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0]
    for lg in a.log_n:
        build_ms = median_ms(lambda: fill(zk, ctx, cid, (ca, cd), G, lg)[0].description(), a.reps, a.warmup)
        c, ins = fill(zk, ctx, cid, (ca, cd), G, lg)
        desc = c.description()
        assert desc.size() == 1 << lg
        assign_ms = median_ms(lambda: c.assign(ins), a.reps, a.warmup)
        line = {"what": "program", "log_n": lg, "rows": c.n_gates, "vars": c.num_vars, "build_ms": build_ms, "witness_replay_ms": assign_ms}
        if not a.no_prove:
            ck = make_key(ctx, cid, 1 << lg, lg)
            t, (pk, vk, pre) = timed(lambda: zc.compile(desc, ck, b"bench", cid, ctx))
            line["compile_ms"] = t * 1e3
            values = c.assign(ins)
            line["gather_ms"] = median_ms(lambda: zc.assign(desc, values, ctx), a.reps, a.warmup)
            wires = zc.assign(desc, values, ctx)
            t, rep = timed(lambda: zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx))
            assert rep.ok, str(rep)
            line["check_circuit_ms"] = median_ms(lambda: zk.check_circuit(pk, wires, {}, ca_m, cd_m, ctx=ctx), a.reps, a.warmup)
            line["prove_ms"] = median_ms(lambda: prover.prove(pk, ck, wires, {}, pre, ca_m, cd_m), 3, 1)
            line["witness_share_of_prove"] = line["witness_replay_ms"] / line["prove_ms"]
            ck.close()
            del pk, vk, wires, values
        emit(line)
        del c, ins, desc
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
