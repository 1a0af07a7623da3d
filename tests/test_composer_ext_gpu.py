"""GPU suite of the device composer (ark_plonk_amd/composer.py; csrc/gadget_layout.hip: gadget_layout, gadget_insertions,
lookup_table_fill; csrc/gadget_witness.hip: gadget_w_select, gadget_w_is_zero, gadget_w_var_bits, gadget_w_var_walk, gadget_w_var_norm) for
the kinds from add_witness_to_circuit_description on: is_zero / is_eq, the
conditional selects, variable-base scalar multiplication, lookup gates and the lookup-table builders -- descriptions and values
against the sequential restatement of the reference's composer (tests/composer_ref_ext.py), the reference's own gadget tests end to
end (compile -> assign -> check_circuit -> prove -> the oracle's verifier), and the refusals.  Every comparison is exact equality."""
import json
import os
import random

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib, prover
from ark_plonk_amd import compile as zc
from ark_plonk_amd.circuit_check import CircuitNotSatisfied
from ark_plonk_amd.composer import LookupTable
from ark_plonk_amd.curves import fr_to_mont
from oracle import bigint_oracle as bo
from tests import composer_ref as cr
from tests import composer_ref_ext as cx
from tests.test_composer_gpu import (BLINDING, NAMES, DevApi, assert_equal_to_reference, assign, check_of, committer, dev_fr, prove_and_verify,
                                     setup)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gadget_reference_cases_ext.json")))


def new_pair(cid, ctx):
    p, ca, cd, _ = setup(cid)
    return zk.Composer(cid, ctx, coeffs=(ca, cd)), cx.RefComposerExt(p, ca, cd, BLINDING)


def assert_equal_ext(cid, dev, ref, values):
    """assert_equal_to_reference, and the table columns"""
    desc = assert_equal_to_reference(cid, dev, ref, values)
    assert len(desc.table_cols) == (4 if ref.lookup_table.size() else 0)
    for got, want in zip(desc.table_cols, ref.lookup_table.columns()):
        assert np.array_equal(got.cpu().numpy().view(np.uint64), fr_to_mont(cid, want))
    return desc


def zero_edges(p, rng, B):
    """zeros at lane 0 and on both sides of the 256-lane block edge, non-zero values elsewhere"""
    vals = [rng.randrange(1, p) for _ in range(B)]
    for k in (0, 2, 255, 256):
        if k < B:
            vals[k] = 0
    return vals


# ---- 1. per gadget kind: description and values equal the sequential composer's
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_segments_equal_the_reference_composer_ext(cid, B, ctx):
    p, ca, cd, G = setup(cid)
    rng = random.Random(300 * cid + B)
    dev, ref = new_pair(cid, ctx)
    xs = zero_edges(p, rng, B)
    ys = [xs[k] if k % 3 == 0 else rng.randrange(p) for k in range(B)]              # equal pairs, (0, 0) among them
    zs = [0] * min(B, 256) + [5] * max(B - 256, 0)                                  # a block of zeros only
    bits = [(k + 1) % 2 for k in range(B)] if B > 1 else [1]
    us, vs = [rng.randrange(p) for _ in range(B)], [rng.randrange(p) for _ in range(B)]
    consts = [0, 1, p - 1][:B] + [rng.randrange(p) for _ in range(B - 3)]
    cols = [xs, ys, zs, bits, us, vs]
    h = [dev.inputs(B) for _ in cols]
    rh = [[ref.add_input(v) for v in col] for col in cols]
    x, y, z, bit, u, v = h
    rx, ry, rz, rbit, ru, rv = rh
    each = lambda fn: [fn(k) for k in range(B)]  # noqa: E731
    same = lambda got, want: got.cpu().tolist() == want  # noqa: E731

    w = dev.add_witness_to_circuit_description(consts)
    rw = each(lambda k: ref.add_witness_to_circuit_description(consts[k]))
    assert same(w, rw)
    assert same(dev.add_witness_to_circuit_description(7, B), each(lambda k: ref.add_witness_to_circuit_description(7)))
    b1, rb1 = dev.is_zero_with_output(x), each(lambda k: ref.is_zero_with_output(rx[k]))
    assert same(b1, rb1)
    assert same(dev.is_zero_with_output(z), each(lambda k: ref.is_zero_with_output(rz[k])))
    assert same(dev.is_zero_with_output(0), [ref.is_zero_with_output(0)])           # a single call on the zero variable
    e1, re1 = dev.is_eq_with_output(x, y), each(lambda k: ref.is_eq_with_output(rx[k], ry[k]))
    assert same(e1, re1)
    assert same(dev.is_eq_with_output(z, 0), each(lambda k: ref.is_eq_with_output(rz[k], 0)))
    s, rs = dev.conditional_select(bit, x, y), each(lambda k: ref.conditional_select(rbit[k], rx[k], ry[k]))
    assert same(s, rs)
    s2, rs2 = dev.conditional_select(e1, s, w), each(lambda k: ref.conditional_select(re1[k], rs[k], rw[k]))     # chained through handles
    assert same(s2, rs2)
    ps = dev.conditional_point_select((x, y), (u, v), bit)
    rps = each(lambda k: ref.conditional_point_select((rx[k], ry[k]), (ru[k], rv[k]), rbit[k]))
    assert same(ps[0], [q[0] for q in rps]) and same(ps[1], [q[1] for q in rps])
    pn = dev.conditional_point_neg(b1, ps)
    rpn = each(lambda k: ref.conditional_point_neg(rb1[k], rps[k]))
    assert same(pn[0], [q[0] for q in rpn]) and same(pn[1], [q[1] for q in rpn])
    # the compositions with the reference's names
    assert same(dev.conditional_select_zero(bit, u), each(lambda k: ref.conditional_select_zero(rbit[k], ru[k])))
    assert same(dev.conditional_select_one(bit, v), each(lambda k: ref.conditional_select_one(rbit[k], rv[k])))
    idp, ridp = dev.identity(B), each(lambda k: ref.identity())
    assert idp[0] == 0 and same(idp[1], [q[1] for q in ridp])
    dp = dev.add_affine_to_circuit_description((us, vs))
    rdp = each(lambda k: ref.add_affine_to_circuit_description((us[k], vs[k])))
    assert same(dp[0], [q[0] for q in rdp]) and same(dp[1], [q[1] for q in rdp])
    dev.assert_equal_point(dp, (u, v))
    each(lambda k: ref.assert_equal_point(rdp[k], (ru[k], rv[k])))
    dev.assert_equal_public_point(pn, (us, 9))
    each(lambda k: ref.assert_equal_public_point(rpn[k], (us[k], 9)))
    pa = dev.add_public_affine((vs, us), B)
    rpa = each(lambda k: ref.add_public_affine((vs[k], us[k])))
    assert same(pa[0], [q[0] for q in rpa]) and same(pa[1], [q[1] for q in rpa])
    cols.append([c_ for k in range(B) for c_ in (vs[k], us[k])])                    # add_affine's values: x_0 y_0 x_1 y_1 ...
    # lookup gates against a concatenated table
    dev.lookup_table.insert_multi_xor(0, 3)
    dev.lookup_table.insert_row(1, 2, 3, 4)
    dev.lookup_table.insert_multi_and(5, 3)
    ref.lookup_table.insert_multi_xor(0, 3)
    ref.lookup_table.insert_row(1, 2, 3, 4)
    ref.lookup_table.insert_multi_and(5, 3)
    assert same(dev.lookup_gate(x, y, s, bit), each(lambda k: ref.lookup_gate(rx[k], ry[k], rs[k], rbit[k])))
    assert same(dev.lookup_gate(x, bit, u, pi=list(range(B))), each(lambda k: ref.lookup_gate(rx[k], rbit[k], ru[k], None, k)))
    values, _ = assign(cid, dev, cols)
    assert_equal_ext(cid, dev, ref, values)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_block_inversion_at_the_edges_of_a_workgroup(cid, B, ctx):
    """is_zero_with_output and point_addition_gate share one field inversion per 256-lane workgroup (csrc/block_inverse.cuh): one call,
    one call short of a workgroup, a whole one, one call into the second.  is_zero's zeros -- which enter the workgroup's product as 1
    -- stand at lanes 0, 255 and 256.  Description and values equal the sequential composer's exactly."""
    p, ca, cd, G = setup(cid)
    rng = random.Random(700 * cid + B)
    dev, ref = new_pair(cid, ctx)
    xs = zero_edges(p, rng, B)
    pool = [cr.te_mul(p, ca, cd, rng.randrange(1, 1 << 16), G) for _ in range(16)]
    pts = [[pool[rng.randrange(16)] for _ in range(B)] for _ in range(2)]
    cols = [xs, [q[0] for q in pts[0]], [q[1] for q in pts[0]], [q[0] for q in pts[1]], [q[1] for q in pts[1]]]
    h = [dev.inputs(B) for _ in cols]
    rh = [[ref.add_input(v) for v in col] for col in cols]
    b, rb = dev.is_zero_with_output(h[0]), [ref.is_zero_with_output(rh[0][k]) for k in range(B)]
    assert b.cpu().tolist() == rb
    s = dev.point_addition_gate((h[1], h[2]), (h[3], h[4]))
    rs = [ref.point_addition_gate((rh[1][k], rh[2][k]), (rh[3][k], rh[4][k])) for k in range(B)]
    assert s[0].cpu().tolist() == [q[0] for q in rs] and s[1].cpu().tolist() == [q[1] for q in rs]
    values, _ = assign(cid, dev, cols)
    assert_equal_ext(cid, dev, ref, values)


# ---- 2. variable-base scalar multiplication
def var_base_points(cid):
    p, ca, cd, G = setup(cid)
    return [G, ((-G[0]) % p, G[1]), (0, 1)]


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_variable_base_equals_the_reference_composer(cid, B, ctx):
    p, ca, cd, G = setup(cid)
    M = p.bit_length()
    rng = random.Random(70 * cid + B)
    pts = var_base_points(cid)
    five = [0, 1, p - 1, 1 << (M - 1), rng.randrange(p)]
    rounds = [[e] for e in five] if B == 1 else [five[:3], five[3:] + [rng.randrange(p)]]
    for r, es in enumerate(rounds):
        ps = [pts[(k + r) % 3] for k in range(B)]          # the base point, its negative, the identity
        dev, ref = new_pair(cid, ctx)
        e, (hx, hy) = dev.inputs(B), dev.add_affine(B)
        re_ = [ref.add_input(v) for v in es]
        rp = [ref.add_affine(q) for q in ps]
        out = dev.variable_base_scalar_mul(e, (hx, hy))
        rout = [ref.variable_base_scalar_mul(re_[k], rp[k]) for k in range(B)]
        assert out[0].cpu().tolist() == [q[0] for q in rout] and out[1].cpu().tolist() == [q[1] for q in rout]
        values, _ = assign(cid, dev, [es, [c_ for q in ps for c_ in q]])
        assert_equal_ext(cid, dev, ref, values)
        for k in range(B):
            assert (ref.values[rout[k][0]], ref.values[rout[k][1]]) == cr.te_mul(p, ca, cd, es[k], ps[k])


@pytest.mark.parametrize("cid", [0, 1])
def test_variable_base_257_calls(cid, ctx):
    """the whole segment of 257 calls built and replayed; calls 0, 255 and 256 (both sides of the 256-lane block edge of the walk) equal
    the restatement run on each of them alone, at the offsets the fixed per-call shape gives; check_circuit: the whole circuit holds"""
    import torch
    p, ca, cd, G = setup(cid)
    M = p.bit_length()
    B, R, V = 257, 8 * M + 2, 9 * M + 257
    rng = random.Random(90 + cid)
    pts = var_base_points(cid)
    es = [rng.randrange(p) for _ in range(B)]
    es[0], es[255], es[256] = p - 1, 1 << (M - 1), rng.randrange(p)
    ps = [pts[0] if k % 5 else pts[1 + (k // 5) % 2] for k in range(B)]
    ps[255], ps[256] = pts[1], pts[0]
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    e, hx, hy = dev.inputs(B), dev.inputs(B), dev.inputs(B)
    row0, var0 = dev.n_gates, dev.num_vars
    out = dev.variable_base_scalar_mul(e, (hx, hy))
    assert (dev.n_gates, dev.num_vars) == (row0 + B * R, var0 + B * V)
    assert out[0].cpu().tolist() == [var0 + k * V + V - 2 for k in range(B)] and out[1].cpu().tolist() == [var0 + k * V + V - 1 for k in range(B)]
    values, _ = assign(cid, dev, [es, [q[0] for q in ps], [q[1] for q in ps]])
    desc = dev.description()
    n = desc.size()
    got_w = [w.cpu().numpy() for w in desc.wires]
    got_q = {name: desc.selectors[name].cpu().numpy().view(np.uint64) for name in cr.SELECTORS}
    got_iv, got_ip = desc.ins_var.cpu().numpy(), desc.ins_pos.cpu().numpy().view(np.uint32)
    got_v = values.cpu().numpy().view(np.uint64)
    ins0 = 16                                               # the prelude's insertions; inputs() maps nothing
    for k in (0, 255, 256):
        ref = cx.RefComposerExt(p, ca, cd, BLINDING)
        rin = [ref.add_input(es[k]), ref.add_input(ps[k][0]), ref.add_input(ps[k][1])]
        r0, v0 = ref.n, len(ref.values)
        ref.variable_base_scalar_mul(rin[0], (rin[1], rin[2]))
        assert (ref.n - r0, len(ref.values) - v0) == (R, V)
        ids = {0: 0, rin[0]: 9 + k, rin[1]: 9 + B + k, rin[2]: 9 + 2 * B + k}
        tr = lambda v: ids[v] if v < v0 else var0 + k * V + (v - v0)  # noqa: E731
        lo = row0 + k * R
        for w in range(4):
            assert got_w[w][lo:lo + R].tolist() == [tr(v) for v in ref.w[w][r0:]], (k, w)
        for name in cr.SELECTORS:
            assert np.array_equal(got_q[name][lo:lo + R], fr_to_mont(cid, ref.q[name][r0:])), (k, name)
        i_lo = ins0 + k * 4 * R
        assert got_iv[i_lo:i_lo + 4 * R].tolist() == [tr(v) for v in ref.ins_var[16:]]
        assert got_ip[i_lo:i_lo + 4 * R].tolist() == [w * n + lo + (r - r0) for w, r in zip(ref.ins_wire[16:], ref.ins_row[16:])]
        assert np.array_equal(got_v[var0 + k * V:var0 + (k + 1) * V], fr_to_mont(cid, ref.values[v0:])), k
    # the key without its commitments (compile's first half): the check needs the selector, sigma and table columns only
    domain, domain_4n = zk.Radix2EvaluationDomain.new(n, cid, ctx), zk.Radix2EvaluationDomain.new(4 * n, cid, ctx)
    sel = {name: zc._pad_rows(desc.selectors[name], n, False) for name in cr.SELECTORS}
    sig = zc.sigma_evals(domain, desc.ins_var, desc.ins_pos, desc.num_vars, ctx)
    pk = prover.ProverKey(domain, domain_4n, sel, sig, [torch.zeros((n, 4), dtype=torch.int64, device="cuda") for _ in range(4)])
    rep = zk.check_circuit(pk, zc.assign(desc, values, ctx), {}, fr_to_mont(cid, [ca])[0], fr_to_mont(cid, [cd])[0], selector_evals=sel, ctx=ctx)
    assert rep.ok, str(rep)
    torch.cuda.synchronize()


# ---- 3. a mixed program, segments chained through handles
@pytest.mark.parametrize("cid", [0, 1])
def test_mixed_program_ext(cid, ctx):
    p, ca, cd, G = setup(cid)
    rng = random.Random(15 + cid)
    B = 2
    dev, ref = new_pair(cid, ctx)
    H = cr.te_mul(p, ca, cd, 31, G)
    xs, ys = [rng.randrange(1 << 64), 12345], [rng.randrange(1 << 64), 12345]      # call 0 unequal, call 1 equal
    las, lbs = [3, 14], [9, 7]
    cols = [xs, ys, [G[0]] * B, [G[1]] * B, [H[0]] * B, [H[1]] * B, las, lbs, [a ^ b for a, b in zip(las, lbs)], [p - 1] * B]
    h = [dev.inputs(B) for _ in cols]
    rh = [[ref.add_input(v) for v in col] for col in cols]
    dev.lookup_table = LookupTable.xor_table(0, 4)
    ref.lookup_table = cx.LookupTable.xor_table(p, 0, 4)
    dev.range_gate(h[0], 64)
    eq = dev.is_eq_with_output(h[0], h[1])
    dev.lookup_gate(h[6], h[7], h[8], h[9])
    pt = dev.conditional_point_select((h[2], h[3]), (h[4], h[5]), eq)
    out = dev.variable_base_scalar_mul(h[0], pt)
    want = [cr.te_mul(p, ca, cd, xs[k], G if xs[k] == ys[k] else H) for k in range(B)]
    dev.assert_equal_public_point(out, ([q[0] for q in want], [q[1] for q in want]))
    for k in range(B):
        ref.range_gate(rh[0][k], 64)
    req = [ref.is_eq_with_output(rh[0][k], rh[1][k]) for k in range(B)]
    for k in range(B):
        ref.lookup_gate(rh[6][k], rh[7][k], rh[8][k], rh[9][k])
    rpt = [ref.conditional_point_select((rh[2][k], rh[3][k]), (rh[4][k], rh[5][k]), req[k]) for k in range(B)]
    rout = [ref.variable_base_scalar_mul(rh[0][k], rpt[k]) for k in range(B)]
    for k in range(B):
        ref.assert_equal_public_point(rout[k], want[k])
    values, pi = assign(cid, dev, cols)
    desc = assert_equal_ext(cid, dev, ref, values)
    assert desc.size() == 1 << 13 and sorted(pi) == sorted(ref.pi)
    assert [ref.values[v] for v in req] == [0, 1]


# ---- 4. the reference-held cases, end to end
class DevApiExt(DevApi):
    """tests/composer_ref_ext.run_program on the device composer: one call per segment"""

    def identity(self):
        return self.c.identity()

    def is_zero(self, a):
        return self.c.is_zero_with_output(a)

    def is_eq(self, a, b):
        return self.c.is_eq_with_output(a, b)

    def assert_equal(self, a, b):
        self.c.assert_equal(a, b)

    def select(self, bit, a, b):
        return self.c.conditional_select(bit, a, b)

    def point_select(self, p1, p0, bit):
        return self.c.conditional_point_select(p1, p0, bit)

    def point_neg(self, bit, pt):
        return self.c.conditional_point_neg(bit, pt)

    def var_base(self, scalar, pt):
        return self.c.variable_base_scalar_mul(scalar, pt)

    def table(self, kind, lower_bound, n):
        getattr(self.c.lookup_table, f"insert_multi_{kind}")(lower_bound, n)

    def lookup(self, a, b, c, d):
        return self.c.lookup_gate(a, b, c, d)


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("case", CASES["cases"], ids=lambda c: c["name"])
def test_reference_held_cases_end_to_end_ext(cid, case, ctx, oracle_cpu):
    import torch
    p, ca, cd, G = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    api = DevApiExt(dev)
    cx.run_program(case["program"], api, p, ca, cd, G)
    rows = sorted(dev.n_gates + r for r in case["rows"])
    if dev.n_gates <= 16:                                   # inert rows behind the program, so that the domain has the prover's minimum of 32
        dev.arithmetic_gate(0, 0, 0, B=17)
    desc = dev.description()
    assert desc.size() <= case["n"]                        # the reference sizes its setup by n; the circuit itself may be smaller
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
        assert not rep.ok and rep.rows(None) == [(r, [case.get("bit", CASES["reject_bit"])]) for r in rows], str(rep)
        with pytest.raises(CircuitNotSatisfied):
            prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, pi_ints, b"gadget case", check=True)
    torch.cuda.synchronize()
    ck.close()


# ---- 5. table builders
@pytest.mark.parametrize("cid", [0, 1])
def test_table_builders(cid, ctx):
    p = setup(cid)[0]

    def same(dev_table, ref_table):
        cols = dev_table.columns(cid, ctx, "cuda")
        assert dev_table.size() == ref_table.size() == int(cols[0].shape[0])
        for got, want in zip(cols, ref_table.columns()):
            assert np.array_equal(got.cpu().numpy().view(np.uint64), fr_to_mont(cid, want))
    same(LookupTable.xor_table(0, 4), cx.LookupTable.xor_table(p, 0, 4))
    same(LookupTable.add_table(3, 5), cx.LookupTable.add_table(p, 3, 5))
    same(LookupTable.mul_table(4000, 12), cx.LookupTable.mul_table(p, 4000, 12))   # products beyond 2^16
    d, r = LookupTable(), cx.LookupTable(p)
    for t in (d, r):
        t.insert_multi_add(1, 3)
        t.insert_multi_mul(0, 2)
        t.insert_row(p - 1, 5, 6, 7)
        t.insert_row(8, 9, 10, 11)
        t.insert_multi_xor(6, 4)
        t.insert_multi_and(0, 3)
    same(d, r)
    # a table larger than the gate count sets the size of the circuit
    dev = zk.Composer(cid, ctx)
    x = dev.inputs(3)
    dev.lookup_table = LookupTable.xor_table(0, 4)
    dev.lookup_gate(x, x, 0)
    desc = dev.description()
    assert dev.n_gates == 7 and desc.size() == 256 and [int(t.shape[0]) for t in desc.table_cols] == [256] * 4


# ---- 6. refusals
@pytest.mark.parametrize("cid", [0, 1])
def test_refusals_ext(cid, ctx):
    import torch
    p, ca, cd, G = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    x = dev.inputs(4)
    before = (dev.n_gates, dev.num_vars)
    other = zk.Composer(cid, ctx, coeffs=(ca, cd))
    for call in (lambda h: dev.is_zero_with_output(h), lambda h: dev.conditional_select(x, h, x), lambda h: dev.variable_base_scalar_mul(x, (x, h)),
                 lambda h: dev.conditional_point_select((x, x), (x, h), x), lambda h: dev.lookup_gate(x, x, x, h)):
        with pytest.raises(ValueError):
            call(other.inputs(4))                           # a handle of another composer
        undefined = torch.tensor([9, 10, dev.num_vars, 11], dtype=torch.int32, device="cuda")   # an id at the segment's var0
        with pytest.raises(zk._lib.ZkError) as ei:
            call(undefined)
        assert ei.value.code == _lib.ZK_ERR_BAD_ARG
        with pytest.raises(ValueError):
            call(dev.num_vars)                              # an undefined id given as an integer
        assert (dev.n_gates, dev.num_vars) == before
    # lookup gates with no table: refused when the description is asked for
    dev.lookup_gate(x, x, x)
    with pytest.raises(ValueError):
        dev.description()
    dev.lookup_table.insert_multi_and(0, 2)
    assert dev.description().size() == 16
    # a table beyond the limit
    for bad in (lambda: LookupTable.xor_table(0, 13), lambda: LookupTable().insert_multi_mul(0, 64), lambda: LookupTable.add_table(9, 3)):
        with pytest.raises(ValueError):
            bad()
    L = _lib.lib()
    buf = torch.zeros((16, 4), dtype=torch.int64, device="cuda")
    ptr = buf.data_ptr()
    assert L.zk_lookup_table_dev(None, cid, 0, 0, 1, ptr, ptr, ptr, ptr) == _lib.ZK_ERR_BAD_ARG
    for op, lower, n in ((4, 0, 1), (-1, 0, 1), (0, 0, 13), (0, 2, 1)):
        assert L.zk_lookup_table_dev(ctx.handle, cid, op, lower, n, ptr, ptr, ptr, ptr) == _lib.ZK_ERR_BAD_ARG
    assert L.zk_lookup_table_dev(ctx.handle, cid, 0, 0, 1, ptr, ptr, None, ptr) == _lib.ZK_ERR_BAD_ARG
    # a zero denominator of the group law: on the curve (a, d) = (1, -1) the doubling of (1, 1) has 1 + d x^2 y^2 = 0, which the scalar
    # 2 reaches in its last iteration; the scalar 1 never doubles the point and is accepted
    odd = zk.Composer(cid, ctx, coeffs=(1, p - 1))
    e, px, py = odd.inputs(3), odd.inputs(3), odd.inputs(3)
    odd.variable_base_scalar_mul(e, (px, py))
    ones = dev_fr(cid, [1, 1, 1])
    with pytest.raises(zk._lib.ZkError) as ei:
        odd.assign([dev_fr(cid, [1, 2, 1]), ones, ones])
    assert ei.value.code == _lib.ZK_ERR_BAD_ARG
    assert odd.assign([dev_fr(cid, [1, 1, 0]), ones, ones]).shape[0] == odd.num_vars
    torch.cuda.synchronize()


def test_ext_inside_an_open_deferred_round(ctx, oracle_cpu):
    """new-kind segments built and their witnesses replayed while a deferred round is open on the ctx: the same bytes as outside, and
    the round's commitments are what they are without the calls in between"""
    import torch
    cid = 0
    p, ca, cd, G = setup(cid)
    rng = random.Random(19)
    xs = [rng.randrange(p) for _ in range(5)]
    xs[3] = 0

    def build():
        dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
        x, gx, gy = dev.inputs(5), dev.inputs(5), dev.inputs(5)
        b = dev.is_zero_with_output(x)
        pt = dev.conditional_point_neg(b, dev.variable_base_scalar_mul(x, (gx, gy)))
        dev.lookup_table = LookupTable.xor_table(0, 2)
        dev.lookup_gate(b, 0, b, dev.add_witness_to_circuit_description(-1))
        dev.assert_equal_point(pt, pt)
        desc = dev.description()
        values, _ = assign(cid, dev, [xs, [G[0]] * 5, [G[1]] * 5])
        return [t.cpu().numpy().tobytes() for t in list(desc.wires) + [desc.selectors[k] for k in cr.SELECTORS] + list(desc.table_cols)
                + [desc.ins_var, desc.ins_pos, values]]
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
