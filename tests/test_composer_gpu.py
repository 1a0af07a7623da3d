"""GPU suite of the device composer (ark_plonk_amd/composer.py; csrc/gadget_layout.hip: gadget_layout, gadget_insertions;
csrc/gadget_witness.hip: gadget_w_poly, gadget_w_range, gadget_w_logic, gadget_w_curve, gadget_w_fixed_walk, gadget_w_fixed_norm) for the
arithmetic family, the range and logic gates, curve addition and the fixed base: descriptions and values against the sequential
restatement of the reference's composer (tests/composer_ref.py), the reference's own gadget tests end to end (compile -> assign ->
check_circuit -> prove -> the oracle's verifier), localisation of failing calls, a circuit that fills 2^14 rows, and the refusals.
Every comparison is exact equality."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib, prover
from ark_plonk_amd import compile as zc
from ark_plonk_amd.circuit_check import CircuitNotSatisfied
from ark_plonk_amd.curves import fr_to_mont
from oracle import bigint_oracle as bo
from oracle import verifier_oracle as vo
from oracle import wire_oracle as wo
from tests import composer_ref as cr
from tests.conftest import TAU, srs_from_powers, tau_powers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gadget_reference_cases.json")))
NAMES = {0: "bls12_381", 1: "bn254"}
BLINDING = (11, 12, 13, 14, 15, 16, 17, 18)
_BASE = {}


def setup(cid):
    if cid not in _BASE:
        p, ca, cd = cr.EMBEDDED[NAMES[cid]]
        _BASE[cid] = (p, ca, cd, cr.te_point(p, ca, cd))
    return _BASE[cid]


def dev_fr(cid, ints):
    import torch
    return torch.from_numpy(fr_to_mont(cid, ints).view(np.int64)).cuda()


def new_pair(cid, ctx):
    p, ca, cd, _ = setup(cid)
    return zk.Composer(cid, ctx, coeffs=(ca, cd)), cr.RefComposer(p, ca, cd, BLINDING)


def assign(cid, dev, inputs, **kw):
    """(values, {row: limbs}) whether or not the circuit has public inputs"""
    out = dev.assign([dev_fr(cid, v) for v in inputs], blinding=dev_fr(cid, BLINDING), **kw)
    return out if isinstance(out, tuple) else (out, {})


def assert_equal_to_reference(cid, dev, ref, values):
    desc = dev.description()
    n = desc.size()
    assert (desc.n_gates, desc.num_vars, n) == (ref.n, len(ref.values), ref.size())
    for w in range(4):
        assert desc.wires[w].cpu().tolist() == ref.w[w], f"wire {w}"
    for name in cr.SELECTORS:
        assert np.array_equal(desc.selectors[name].cpu().numpy().view(np.uint64), fr_to_mont(cid, ref.q[name])), name
    assert desc.ins_var.cpu().tolist() == ref.ins_var
    assert desc.ins_pos.cpu().numpy().view(np.uint32).tolist() == ref.ins_pos(n)
    assert sorted(desc.public_inputs) == sorted(ref.pi)
    for row, v in ref.pi.items():
        assert np.array_equal(np.asarray(desc.public_inputs[row], dtype=np.uint64), fr_to_mont(cid, [v])[0])
    got = values.cpu().numpy().view(np.uint64)
    want = fr_to_mont(cid, ref.values)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} values differ, first at variable {bad[0]}"
    return desc


def edge_values(p, rng, B, bits):
    vals = [0, 1, (1 << bits) - 1, (1 << bits) % p, p - 1, (1 << 64) - 1, 1 << 32]
    return ([rng.randrange(p) for _ in range(B)] if B < 8 else vals + [rng.randrange(p) for _ in range(B - len(vals))])[:B]


# ---- 1. per gadget kind: description and values equal the sequential composer's
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("B", [1, 2, 3, 63, 64, 65, 257])
def test_segments_equal_the_reference_composer(cid, B, ctx):
    p, ca, cd, G = setup(cid)
    M = p.bit_length()
    rng = random.Random(100 * cid + B)
    dev, ref = new_pair(cid, ctx)
    xs, ys = edge_values(p, rng, B, 64), [rng.randrange(p) for _ in range(B)]
    x, y = dev.inputs(B), dev.inputs(B)
    rx, ry = [ref.add_input(v) for v in xs], [ref.add_input(v) for v in ys]
    inputs = [xs, ys]
    if B != 3:
        # the arithmetic family: constant and per-call coefficients, a public input per call, a fourth wire, given and computed outputs
        qm, qc, pis = [rng.randrange(p) for _ in range(B)], [rng.randrange(p) for _ in range(B)], [rng.randrange(p) for _ in range(B)]
        s1 = dev.arithmetic_gate(x, y, q_m=3, q_l=5, q_r=p - 2, q_c=9)
        r1 = [ref.arithmetic_gate(rx[k], ry[k], q_m=3, q_l=5, q_r=p - 2, q_c=9) for k in range(B)]
        s2 = dev.arithmetic_gate(s1, x, None, y, q_m=qm, q_l=1, q_r=7, q_o=1, q_c=dev_fr(cid, qc), q_4=11, pi=pis)
        r2 = [ref.arithmetic_gate(r1[k], rx[k], None, ry[k], q_m=qm[k], q_l=1, q_r=7, q_o=1, q_c=qc[k], q_4=11, pi=pis[k]) for k in range(B)]
        dev.arithmetic_gate(x, y, s2, 0, q_m=1, q_o=p - 1)
        for k in range(B):
            ref.arithmetic_gate(rx[k], ry[k], r2[k], None, q_m=1, q_o=p - 1)
        dev.constrain_to_constant(s1, qc, pi=5)
        dev.assert_equal(s2, 0)
        dev.boolean_gate(y)
        for fn in (lambda k: ref.constrain_to_constant(r1[k], qc[k], 5), lambda k: ref.assert_equal(r2[k], 0), lambda k: ref.boolean_gate(ry[k])):
            for k in range(B):
                fn(k)
        for bits in (2, 10, 34, 64, 254):
            dev.range_gate(x, bits)
            for k in range(B):
                ref.range_gate(rx[k], bits)
        for bits in (2, 10, 64, 256):
            for xor in (True, False):
                z = (dev.xor_gate if xor else dev.and_gate)(x, y, bits)
                rz = [ref.logic_gate(rx[k], ry[k], bits, xor) for k in range(B)]
                assert z.cpu().tolist() == rz
    if B in (1, 64, 65):
        pts = [[cr.te_mul(p, ca, cd, rng.randrange(1, 1 << 16), G) for _ in range(B)] for _ in range(2)]
        cols = [[q[0] for q in pts[0]], [q[1] for q in pts[0]], [q[0] for q in pts[1]], [q[1] for q in pts[1]]]
        h = [dev.inputs(B) for _ in range(4)]
        rh = [[ref.add_input(v) for v in col] for col in cols]
        inputs += cols
        s = dev.point_addition_gate((h[0], h[1]), (h[2], h[3]))
        rs = [ref.point_addition_gate((rh[0][k], rh[1][k]), (rh[2][k], rh[3][k])) for k in range(B)]
        assert s[0].cpu().tolist() == [q[0] for q in rs] and s[1].cpu().tolist() == [q[1] for q in rs]
    if B in (1, 3, 65):
        # scalars below 2^252 (none has more than M digits) and the edges; the last edge is the largest scalar with M digits
        # (floor(2^256 / 3) on BLS12-381)
        edges = [((1 << (M + 1)) - 1) // 3, 0, 1, 1 << 251]
        es = (edges[:1] if B == 1 else edges[1:] if B == 3 else edges + [rng.randrange(1 << 252) for _ in range(B - 4)])
        e = dev.inputs(B)
        re_ = [ref.add_input(v) for v in es]
        inputs.append(es)
        s = dev.fixed_base_scalar_mul(e, G)
        rs = [ref.fixed_base_scalar_mul(re_[k], G) for k in range(B)]
        assert s[0].cpu().tolist() == [q[0] for q in rs] and s[1].cpu().tolist() == [q[1] for q in rs]
    values, _ = assign(cid, dev, inputs)
    assert_equal_to_reference(cid, dev, ref, values)


# ---- 2. a mixed program with every kind chained, padded to 2^10
@pytest.mark.parametrize("cid", [0, 1])
def test_mixed_program(cid, ctx):
    p, ca, cd, G = setup(cid)
    rng = random.Random(5 + cid)
    B = 2
    dev, ref = new_pair(cid, ctx)
    xs, ys = [rng.randrange(1 << 64) for _ in range(B)], [rng.randrange(1 << 64) for _ in range(B)]
    other = [cr.te_mul(p, ca, cd, 77 + k, G) for k in range(B)]
    x, y, ox, oy = dev.inputs(B), dev.inputs(B), dev.inputs(B), dev.inputs(B)
    rx, ry = [ref.add_input(v) for v in xs], [ref.add_input(v) for v in ys]
    rox, roy = [ref.add_input(q[0]) for q in other], [ref.add_input(q[1]) for q in other]
    dev.range_gate(x, 64)
    dev.range_gate(y, 64)
    z = dev.xor_gate(x, y, 64)
    dev.constrain_to_constant(z, [a ^ b for a, b in zip(xs, ys)])
    pt = dev.fixed_base_scalar_mul(z, G)
    sm = dev.point_addition_gate(pt, (ox, oy))
    want = [cr.te_mul(p, ca, cd, (xs[k] ^ ys[k]) + 77 + k, G) for k in range(B)]
    dev.constrain_to_constant(sm[0], 0, pi=[-q[0] for q in want])
    dev.boolean_gate(dev.arithmetic_gate(x, 0, q_l=0, q_c=1))
    for k in range(B):
        ref.range_gate(rx[k], 64)
    for k in range(B):
        ref.range_gate(ry[k], 64)
    rz = [ref.xor_gate(rx[k], ry[k], 64) for k in range(B)]
    for k in range(B):
        ref.constrain_to_constant(rz[k], xs[k] ^ ys[k])
    rpt = [ref.fixed_base_scalar_mul(rz[k], G) for k in range(B)]
    rsm = [ref.point_addition_gate(rpt[k], (rox[k], roy[k])) for k in range(B)]
    for k in range(B):
        ref.constrain_to_constant(rsm[k][0], 0, -want[k][0])
    rb = [ref.arithmetic_gate(rx[k], 0, q_l=0, q_c=1) for k in range(B)]
    for k in range(B):
        ref.boolean_gate(rb[k])
    values, pi = assign(cid, dev, [xs, ys, [q[0] for q in other], [q[1] for q in other]])
    desc = assert_equal_to_reference(cid, dev, ref, values)
    assert desc.size() == 1 << 10 and sorted(pi) == sorted(ref.pi)


# ---- 3. the reference-held cases, end to end
class DevApi:
    """tests/composer_ref.run_program on the device composer: one call per segment"""

    def __init__(self, comp):
        self.c, self.inputs = comp, []

    def input(self, v):
        self.inputs.append([v])
        return self.c.inputs(1)

    def zero(self):
        return 0

    def range(self, x, bits):
        self.c.range_gate(x, bits)

    def logic(self, a, b, bits, is_xor):
        return (self.c.xor_gate if is_xor else self.c.and_gate)(a, b, bits)

    def constant(self, x, v, pi):
        self.c.constrain_to_constant(x, v, pi)

    def boolean(self, x):
        self.c.boolean_gate(x)

    def fixed_base(self, s, base):
        return self.c.fixed_base_scalar_mul(s, base)

    def point_add(self, a, b):
        return self.c.point_addition_gate(a, b)

    def arith(self, a, b, d, q, pi):
        return self.c.arithmetic_gate(a, b, None, d, q["q_m"], q["q_l"], q["q_r"], -1, q["q_c"], q["q_4"], pi)


def committer(ctx, oracle_cpu, cid, n):
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    return zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)


def prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, pi_ints, label, check=False):
    """one proof through the oracle's verifier: (accepted, proof)"""
    from tests.test_prover_gpu import dlogs, oracle_points
    cv = bo.CURVES[cid]
    p, ca, cd, _ = setup(cid)
    proof = prover.prove(pk, ck, wires, pi_limbs, pre, fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0], check=check)
    t = vo.seed_transcript(cv, wo.PlonkTranscript(label, cv), oracle_points(cid, vk), vk.n)
    ok, _, _ = vo.verify_with_trapdoor(cv, vk.n.bit_length() - 1, proof.to_bytes(), t, pi_ints, dlogs(cid, ctx, pk, proof), TAU, ca, cd)
    return ok, proof


def check_of(cid, ctx, pk, wires, pi_limbs):
    _, ca, cd, _ = setup(cid)
    return zk.check_circuit(pk, wires, pi_limbs, fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0], ctx=ctx)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("case", CASES["cases"], ids=lambda c: c["name"])
def test_reference_held_cases_end_to_end(cid, case, ctx, oracle_cpu):
    import torch
    p, ca, cd, G = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    api = DevApi(dev)
    cr.run_program(case["program"], api, p, ca, cd, G)
    rows = sorted(dev.n_gates + r for r in case["rows"])
    if dev.n_gates <= 16:                                   # inert rows behind the program, so that the domain has the prover's minimum of 32
        dev.arithmetic_gate(0, 0, 0, B=17)
    desc = dev.description()
    ck = committer(ctx, oracle_cpu, cid, desc.size())
    pk, vk, pre = zc.compile(desc, ck, b"gadget case", cid, ctx)
    values, pi_limbs = assign(cid, dev, api.inputs)
    pi_ints = dict(dev.public_inputs)
    wires = zc.assign(desc, values, ctx)
    rep = check_of(cid, ctx, pk, wires, pi_limbs)
    if case["expect"] == "accept":
        assert rep.ok, str(rep)
        ok, _ = prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, pi_ints, b"gadget case", check=True)
        assert ok
    else:
        assert not rep.ok and rep.rows(None) == [(r, [CASES["reject_bit"]]) for r in rows], str(rep)
        with pytest.raises(CircuitNotSatisfied):
            prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, pi_ints, b"gadget case", check=True)
        ok, _ = prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, pi_ints, b"gadget case")
        assert not ok
    torch.cuda.synchronize()
    ck.close()


# ---- 4. localisation at scale: judged by check_circuit alone
@pytest.mark.parametrize("cid", [0, 1])
def test_failing_range_calls_are_localised(cid, ctx, oracle_cpu):
    import torch
    p, ca, cd, _ = setup(cid)
    rng = random.Random(40 + cid)
    B, bits = 1000, 32
    chosen = sorted(rng.sample(range(B), 7))
    xs = [rng.randrange(1 << bits) for _ in range(B)]
    for j, k in enumerate(chosen):
        xs[k] = (1 << bits) + j if j < 3 else rng.randrange(1 << bits, p)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    x = dev.inputs(B)
    row0 = dev.n_gates
    dev.range_gate(x, bits)
    R = (dev.n_gates - row0) // B
    assert R == 6
    desc = dev.description()
    ck = committer(ctx, oracle_cpu, cid, desc.size())
    pk, _, _ = zc.compile(desc, ck, b"localise", cid, ctx)
    values, pi = assign(cid, dev, [xs])
    rep = check_of(cid, ctx, pk, zc.assign(desc, values, ctx), pi)
    assert rep.rows(None) == [(row0 + k * R + R - 1, ["arith"]) for k in chosen]
    assert rep.failing_rows == 7 and rep.counts["arith"] == 7 and sum(rep.counts.values()) == 7
    torch.cuda.synchronize()
    ck.close()


# ---- 5. a program that fills 2^14 rows: check, one proof, a second assignment on the same key
@pytest.mark.parametrize("cid", [0, 1])
def test_circuit_of_16384_rows(cid, ctx, oracle_cpu):
    import torch
    p, ca, cd, G = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    Bf, Br, Bl = 40, 200, 50
    e, x, y = dev.inputs(Bf), dev.inputs(Br), dev.inputs(Bl)
    pt = dev.fixed_base_scalar_mul(e, G)
    sm = dev.point_addition_gate(pt, pt)
    dev.range_gate(x, 64)
    z = dev.xor_gate(y, x[:Bl].clone(), 64)
    w = dev.and_gate(z, y, 32)
    s = dev.arithmetic_gate(w, z, None, y, q_m=2, q_l=3, q_r=4, q_c=5, q_4=6, pi=list(range(Bl)))
    dev.boolean_gate(dev.arithmetic_gate(s, 0, q_l=0, q_c=1))
    dev.assert_equal(sm[0], sm[0])
    desc = dev.description()
    assert desc.size() == 1 << 14 and desc.n_gates > 1 << 13
    ck = committer(ctx, oracle_cpu, cid, desc.size())
    pk, vk, pre = zc.compile(desc, ck, b"2^14", cid, ctx)
    for seed in (1, 2):
        rng = random.Random(seed)
        ins = [[rng.randrange(1 << 252) for _ in range(Bf)], [rng.randrange(1 << 64) for _ in range(Br)], [rng.randrange(1 << 64) for _ in range(Bl)]]
        values, pi_limbs = assign(cid, dev, ins)
        wires = zc.assign(desc, values, ctx)
        rep = check_of(cid, ctx, pk, wires, pi_limbs)
        assert rep.ok, str(rep)
        ok, _ = prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, dict(dev.public_inputs), b"2^14")
        assert ok
    torch.cuda.synchronize()
    ck.close()


# ---- 6. refusals
@pytest.mark.parametrize("cid", [0, 1])
def test_refusals(cid, ctx, oracle_cpu):
    import torch
    p, ca, cd, G = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    x = dev.inputs(4)
    before = (dev.n_gates, dev.num_vars)
    undefined = torch.tensor([9, 10, dev.num_vars, 11], dtype=torch.int32, device="cuda")       # an id at the segment's var0
    with pytest.raises(zk._lib.ZkError) as ei:
        dev.range_gate(undefined, 8)
    assert ei.value.code == _lib.ZK_ERR_BAD_ARG and (dev.n_gates, dev.num_vars) == before
    for bad_bits in (7, 0, 258):
        with pytest.raises(ValueError):
            dev.range_gate(x, bad_bits)
        with pytest.raises(ValueError):
            dev.xor_gate(x, x, bad_bits)
    other = zk.Composer(cid, ctx, coeffs=(ca, cd))
    with pytest.raises(ValueError):
        dev.boolean_gate(other.inputs(4))
    assert (dev.n_gates, dev.num_vars) == before
    # a scalar whose NAF has more than M digits: the reference asserts, the device sets the flag
    dev.fixed_base_scalar_mul(x, G)
    with pytest.raises(zk._lib.ZkError) as ei:
        dev.assign([dev_fr(cid, [1, 2, p - 1, 3])])
    assert ei.value.code == _lib.ZK_ERR_BAD_ARG
    assert dev.assign([dev_fr(cid, [1, 2, ((1 << (p.bit_length() + 1)) - 1) // 3, 3])]).shape[0] == dev.num_vars
    # null ctx / args, null buffers
    L = _lib.lib()
    a = _lib.GadgetArgs()
    assert L.zk_gadget_layout_dev(None, cid, ctypes.addressof(a), None, None, None, None) == _lib.ZK_ERR_BAD_ARG
    assert L.zk_gadget_layout_dev(ctx.handle, cid, None, None, None, None, None) == _lib.ZK_ERR_BAD_ARG
    assert L.zk_gadget_witness_dev(None, cid, ctypes.addressof(a), None, 0) == _lib.ZK_ERR_BAD_ARG
    assert L.zk_gadget_witness_dev(ctx.handle, cid, None, None, 0) == _lib.ZK_ERR_BAD_ARG
    vals = torch.zeros((16, 4), dtype=torch.int64, device="cuda")
    assert L.zk_gadget_witness_dev(ctx.handle, cid, ctypes.addressof(a), vals.data_ptr(), 16) == _lib.ZK_ERR_BAD_ARG      # calls = 0


def test_inside_an_open_deferred_round(ctx, oracle_cpu):
    """a segment built and a witness replayed while a deferred round is open on the ctx: the same bytes as outside, and the round's
    commitments are what they are without the calls in between"""
    import torch
    cid = 0
    p, ca, cd, G = setup(cid)
    rng = random.Random(9)
    xs = [rng.randrange(1 << 200) for _ in range(5)]

    def build():
        dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
        x = dev.inputs(5)
        dev.range_gate(x, 34)
        dev.point_addition_gate(dev.fixed_base_scalar_mul(x, G), (0, dev.arithmetic_gate(x, 0, q_c=1, q_l=0)))
        desc = dev.description()
        values, _ = assign(cid, dev, [xs])
        return [t.cpu().numpy().tobytes() for t in list(desc.wires) + [desc.selectors[k] for k in cr.SELECTORS] + [desc.ins_var, desc.ins_pos, values]]
    outside = build()
    ck = committer(ctx, oracle_cpu, cid, 64)
    polys = [dev_fr(cid, bo.seeded_scalars(bo.CURVES[cid], 900 + k, 64)) for k in range(2)]
    want = ck.commit_batch(polys)
    ck.commit_begin(polys)
    assert ck.round_pending() == 2
    inside = build()
    assert ck.round_pending() == 2
    assert ck.round_end(2) == want and inside == outside
    torch.cuda.synchronize()
    ck.close()
