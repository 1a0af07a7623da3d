"""tests/composer_ref_ext.py -- the sequential restatement of the reference's remaining gadgets (is_zero / is_eq, the conditional
selects, variable-base scalar multiplication, lookup gates and tables) -- against what the repository already trusts: its circuits
pass the circuit check's definition (tests/circuit_check_ref.py, lookup rows with their table) with sigma from tests/compile_ref.py,
the shape table of DESIGN.md 6e holds (and `zk_gadget_shape` returns the same numbers), the closed forms `row_of`
(csrc/gadget_layout.hip) and the kernels gadget_w_select, gadget_w_is_zero, gadget_w_var_bits, gadget_w_var_walk, gadget_w_var_norm and
lookup_table_fill use equal the sequential loops, the table builders equal the reference's own table tests
(lookup/lookup_table.rs:214-326), and the reference's gadget tests (tests/golden/gadget_reference_cases_ext.json, recorded as data)
come out as the reference says.  Exact integers, both curves, no GPU."""
import ctypes
import json
import os
import random

import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from ark_plonk_amd.curves import fr_from_mont
from tests import circuit_check_ref as ck
from tests import compile_ref
from tests import composer_ref as cr
from tests import composer_ref_ext as cx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gadget_reference_cases_ext.json")))
CURVES = ("bls12_381", "bn254")


def masks_of(name, c: cx.RefComposerExt):
    """the circuit check's definition on the padded circuit of a RefComposerExt, lookup rows against its table"""
    n, wires, sel, pi = c.padded()
    omega = fr_from_mont(name, zk.Radix2EvaluationDomain.new(n, name).group_gen().reshape(1, 4))[0]
    sigma = compile_ref.encode(c.p, omega, n, compile_ref.sigma_dict(n, c.ins_var, c.ins_pos(n)))
    table, rows = c.padded_table()
    return ck.masks(c.p, omega, n, wires, sel, pi, sigma, table, rows, c.ca, c.cd)


def setup(name):
    p, ca, cd = cr.EMBEDDED[name]
    return p, ca, cd, cr.te_point(p, ca, cd)


@pytest.mark.parametrize("name", CURVES)
def test_honest_circuits_pass_the_check(name):
    p, ca, cd, G = setup(name)
    rng = random.Random(17)
    c = cx.RefComposerExt(p, ca, cd)
    c.lookup_table.insert_multi_xor(0, 3)
    c.lookup_table.insert_multi_and(2, 3)
    x, y, z = c.add_input(rng.randrange(p)), c.add_input(rng.randrange(p)), c.add_input(0)
    one = c.add_witness_to_circuit_description(1)
    for a, want in ((x, 0), (z, 1), (0, 1)):
        assert c.values[c.is_zero_with_output(a)] == want
    for a, b, want in ((x, y, 0), (x, x, 1), (z, 0, 1)):
        assert c.values[c.is_eq_with_output(a, b)] == want
    assert c.values[c.conditional_select(one, x, y)] == c.values[x] and c.values[c.conditional_select(0, x, y)] == c.values[y]
    P = c.add_affine(G)
    Q = c.add_affine_to_circuit_description(cr.te_mul(p, ca, cd, 9, G))
    s1, s0 = c.conditional_point_select(P, Q, one), c.conditional_point_select(P, Q, z)
    c.assert_equal_point(s1, P)
    c.assert_equal_point(s0, Q)
    n1, n0 = c.conditional_point_neg(one, P), c.conditional_point_neg(z, P)
    c.assert_equal_public_point(n1, ((-G[0]) % p, G[1]))
    c.assert_equal_public_point(n0, G)
    e = c.add_input(rng.randrange(p))
    R = c.variable_base_scalar_mul(e, P)
    c.assert_equal_public_point(R, cr.te_mul(p, ca, cd, c.values[e], G))
    c.assert_equal_point(c.add_public_affine(G), P)
    a3, b3 = c.add_input(5), c.add_input(6)
    c.lookup_gate(a3, b3, c.add_input(5 ^ 6), c.add_input(-1))
    c.lookup_gate(a3, b3, c.add_input(5 & 6), c.add_input(2))
    assert c.values[c.conditional_select_zero(one, x)] == c.values[x] and c.values[c.conditional_select_one(z, x)] == 1
    assert masks_of(name, c) == [0] * c.size()
    # and a dishonest one: the same tuple against the other tag is no row of the table
    c.lookup_gate(a3, b3, c.add_input(5 ^ 6), c.add_input(2))
    assert {i: m for i, m in enumerate(masks_of(name, c)) if m} == {c.n - 1: 1 << ck.BIT["lookup"]}


@pytest.mark.parametrize("name", CURVES)
def test_shape_table_ext(name):
    """rows, new variables and insertions per call: the table of DESIGN.md 6e, the sequential composer, and zk_gadget_shape"""
    p, ca, cd, G = setup(name)
    M = p.bit_length()
    cid = zk.get_curve(name).curve_id

    def lib_shape(kind, calls=1):
        r, v, i, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_size_t()
        assert _lib.lib().zk_gadget_shape(kind, cid, 0, 0, calls, ctypes.byref(r), ctypes.byref(v), ctypes.byref(i), ctypes.byref(w)) == 0
        return (r.value, v.value, i.value), w.value

    def measured(fn):
        c = cx.RefComposerExt(p, ca, cd)
        ins = [c.add_input(1), c.add_input(5), c.add_input(G[0]), c.add_input(G[1]), c.add_input(7)]
        before = (c.n, len(c.values), len(c.ins_var))
        out = fn(c, ins)
        return (c.n - before[0], len(c.values) - before[1], len(c.ins_var) - before[2]), out, before[1]

    table = (
        (_lib.ZK_GADGET_CONST_WITNESS, (1, 1, 4), lambda c, i: (c.add_witness_to_circuit_description(77),), (0,)),
        (_lib.ZK_GADGET_IS_ZERO, (2, 2, 8), lambda c, i: (c.is_zero_with_output(i[1]),), (1,)),
        (_lib.ZK_GADGET_IS_EQ, (3, 3, 12), lambda c, i: (c.is_eq_with_output(i[1], i[4]),), (2,)),
        (_lib.ZK_GADGET_SELECT, (4, 4, 16), lambda c, i: (c.conditional_select(i[0], i[1], i[4]),), (3,)),
        (_lib.ZK_GADGET_POINT_SELECT, (8, 8, 32), lambda c, i: c.conditional_point_select((i[2], i[3]), (i[1], i[4]), i[0]), (3, 7)),
        (_lib.ZK_GADGET_POINT_NEG, (5, 5, 20), lambda c, i: c.conditional_point_neg(i[0], (i[2], i[3]))[:1], (4,)),
        (_lib.ZK_GADGET_VAR_BASE, (8 * M + 2, 9 * M + 257, 32 * M + 8), lambda c, i: c.variable_base_scalar_mul(i[1], (i[2], i[3])),
         (9 * M + 255, 9 * M + 256)),
        (_lib.ZK_GADGET_LOOKUP, (1, 0, 4), lambda c, i: (c.lookup_gate(i[0], i[1], i[4]), ())[1], ()),
    )
    for kind, want, fn, returns in table:
        got, out, var0 = measured(fn)
        shape, work = lib_shape(kind, calls=7)
        assert got == want == shape, kind
        assert tuple(v - var0 for v in out) == returns, kind          # the returned variables, as offsets among the call's new ones
        assert work == 256 + (96 * (2 * M + 1) * 7 if kind == _lib.ZK_GADGET_VAR_BASE else 0)
    if name == "bls12_381":
        assert lib_shape(_lib.ZK_GADGET_VAR_BASE)[0] == (2042, 2552, 8168)
    L = _lib.lib()
    assert L.zk_gadget_shape(_lib.ZK_GADGET_LOOKUP + 1, cid, 0, 0, 1, None, None, None, None) == _lib.ZK_ERR_BAD_ARG


@pytest.mark.parametrize("name", CURVES)
def test_variable_base_closed_forms(name):
    """what the kernels compute per (call, step) without the loops: bit j and accumulator j = e mod 2^(j+1) at variables j and 256 + j,
    the one at 256 + M, iteration i (bit M-1-i) at variables 257 + M + 8 i and rows 2 M + 2 + 6 i, rows 2 j / 2 j + 1 the boolean and
    accumulator rows with q_l = 2^j, four insertions per row in row order; and the output is te_mul(e, P)"""
    p, ca, cd, G = setup(name)
    M = p.bit_length()
    rng = random.Random(23)
    for e in [0, 1, 2, p - 1, 1 << (M - 1)] + [rng.randrange(p) for _ in range(40)]:
        e %= p
        c = cx.RefComposerExt(p, ca, cd)
        s, P = c.add_input(e), c.add_affine(G)
        v0, r0, i0 = len(c.values), c.n, len(c.ins_var)
        out = c.variable_base_scalar_mul(s, P)
        v = c.values
        assert (v[out[0]], v[out[1]]) == cr.te_mul(p, ca, cd, e, G)
        assert out == (v0 + 9 * M + 255, v0 + 9 * M + 256)
        assert v[v0:v0 + 256] == [(e >> j) & 1 for j in range(256)]
        assert v[v0 + 256:v0 + 256 + M] == [e % (1 << (j + 1)) for j in range(M)]
        assert v[v0 + 256 + M] == 1
        acc = (0, 1)
        for i in range(M):
            bit = (e >> (M - 1 - i)) & 1
            dbl = cr.te_add(p, ca, cd, acc, acc)
            sel = (bit * G[0] % p, (1 - bit + bit * G[1]) % p)
            nxt = cr.te_add(p, ca, cd, dbl, sel)
            u = v0 + 257 + M + 8 * i
            assert v[u:u + 8] == [acc[0] * acc[1] % p, dbl[0], dbl[1], sel[0], sel[1], dbl[0] * sel[1] % p, nxt[0], nxt[1]], (e, i)
            acc = nxt
        if e not in (1, p - 1):
            continue
        # rows and insertions, by the closed form of the layout kernel
        one = v0 + 256 + M
        for j in range(M):
            assert [c.w[k][r0 + 2 * j] for k in range(4)] == [v0 + j, v0 + j, v0 + j, 0]
            assert [c.w[k][r0 + 2 * j + 1] for k in range(4)] == [v0 + j, v0 + 255 + j if j else 0, v0 + 256 + j, 0]
            assert (c.q["q_l"][r0 + 2 * j + 1], c.q["q_r"][r0 + 2 * j + 1], c.q["q_o"][r0 + 2 * j + 1]) == (pow(2, j, p), 1, p - 1)
        assert [c.w[k][r0 + 2 * M] for k in range(4)] == [v0 + 255 + M, s, 0, 0]
        assert [c.w[k][r0 + 2 * M + 1] for k in range(4)] == [one, one, one, 0]
        for i in range(M):
            r, u, bit = r0 + 2 * M + 2 + 6 * i, v0 + 257 + M + 8 * i, v0 + M - 1 - i
            rx, ry = (u - 2, u - 1) if i else (0, one)
            want = [[rx, ry, rx, ry], [u + 1, u + 2, 0, u], [bit, P[0], u + 3, 0], [bit, P[1], u + 4, 0], [u + 1, u + 2, u + 3, u + 4],
                    [u + 6, u + 7, 0, u + 5]]
            assert [[c.w[k][r + t] for k in range(4)] for t in range(6)] == want
            assert [c.q["q_variable_group_add"][r + t] for t in range(6)] == [1, 0, 0, 0, 1, 0]
            assert [c.q["q_arith"][r + t] for t in range(6)] == [0, 0, 1, 1, 0, 0]
        R = 8 * M + 2
        assert c.n - r0 == R
        assert c.ins_row[i0:] == [r0 + t // 4 for t in range(4 * R)] and c.ins_wire[i0:] == [t % 4 for t in range(4 * R)]
        assert c.ins_var[i0:] == [c.w[t % 4][r0 + t // 4] for t in range(4 * R)]


def test_table_builders_equal_the_reference_table_tests():
    """lookup/lookup_table.rs:214-326"""
    p = cr.R_BLS
    n = 4
    for build, op in ((cx.LookupTable.add_table, lambda a, b: (a + b) % 16), (cx.LookupTable.xor_table, lambda a, b: a ^ b),
                      (cx.LookupTable.mul_table, lambda a, b: (a * b) % 16)):
        t = build(p, 0, n)
        assert [row[2] for row in t.rows] == [op(a, b) for a in range(16) for b in range(16)] and t.size() == 256
    add = cx.LookupTable.add_table(p, 0, 3)
    assert add.lookup(2, 3, 0) == 5
    assert add.rows[1][0] + add.rows[1][1] == 1 and add.rows[12][0] + add.rows[12][1] == 5
    with pytest.raises(KeyError):
        cx.LookupTable.xor_table(p, 0, 5).lookup(17, 367, 0)
    t = cx.LookupTable(p)
    t.insert_multi_xor(0, 5)
    t.insert_multi_add(4, 7)
    assert t.rows[-1][2] == 126 and t.rows[36][0] ^ t.rows[36][1] == 5
    assert t.size() == 32 * 32 + 124 * 124
    # the device class counts the same rows without building them
    d = zk.composer.LookupTable()
    d.insert_multi_xor(0, 5)
    d.insert_multi_add(4, 7)
    d.insert_row(1, 2, 3, 4)
    assert d.size() == t.size() + 1
    assert zk.composer.LookupTable.mul_table(3, 5).size() == 29 * 29
    with pytest.raises(ValueError):
        zk.composer.LookupTable.xor_table(0, 13)


def test_fixture_is_data_of_the_listed_reference_tests():
    names = [c["name"] for c in CASES["cases"]]
    assert len(names) == len(set(names)) == 12 and CASES["reject_bit"] == "arith"
    for c in CASES["cases"]:
        assert c["expect"] in ("accept", "reject") and (c["expect"] == "reject") == bool(c["rows"])
        assert c["source"].startswith("not the reference's") or c["source"].split(":")[0].endswith(".rs")
        assert (c["expect"] == "reject") == c["source"].startswith("not the reference's")
    assert sum(c["expect"] == "reject" for c in CASES["cases"]) == 3


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("case", CASES["cases"], ids=lambda c: c["name"])
def test_reference_held_cases_ext(name, case):
    """accept: every mask is zero; reject: the expected rows carry the case's bit, and nothing else is set anywhere"""
    p, ca, cd, G = setup(name)
    c = cx.RefComposerExt(p, ca, cd)
    cx.run_program(case["program"], cx.RefApiExt(c), p, ca, cd, G)
    assert c.size() <= case["n"] <= 16384
    got = {i: m for i, m in enumerate(masks_of(name, c)) if m}
    assert got == {c.n + r: 1 << ck.BIT[case.get("bit", CASES["reject_bit"])] for r in case["rows"]}
