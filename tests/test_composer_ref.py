"""tests/composer_ref.py -- the sequential restatement of the reference's composer the device composer is compared with -- against
what the repository already trusts: its circuits pass the circuit check's definition (tests/circuit_check_ref.py) with sigma from
tests/compile_ref.py, the shape table of the gadgets holds (and `zk_gadget_shape` returns the same numbers), the closed forms the
kernels use equal the sequential loops, and the reference's own gadget tests (tests/golden/gadget_reference_cases.json: inputs and the
expected accept / reject, recorded as data) come out as the reference says.  Exact integers, both curves, no GPU."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gadget_reference_cases.json")))
CURVES = ("bls12_381", "bn254")
BITS = (2, 4, 6, 8, 10, 32, 34, 64, 254, 256)


def masks_of(name, c: cr.RefComposer):
    """the circuit check's definition on the padded circuit of a RefComposer"""
    n, wires, sel, pi = c.padded()
    omega = fr_from_mont(name, zk.Radix2EvaluationDomain.new(n, name).group_gen().reshape(1, 4))[0]
    sigma = compile_ref.encode(c.p, omega, n, compile_ref.sigma_dict(n, c.ins_var, c.ins_pos(n)))
    return ck.masks(c.p, omega, n, wires, sel, pi, sigma, [[0]] * 4, 0, c.ca, c.cd)


def setup(name):
    p, ca, cd = cr.EMBEDDED[name]
    return p, ca, cd, cr.te_point(p, ca, cd)


@pytest.mark.parametrize("name", CURVES)
def test_derived_base_point(name):
    p, ca, cd, G = setup(name)
    assert cr.te_on_curve(p, ca, cd, G) and G != (0, 1)
    assert cr.te_on_curve(p, ca, cd, cr.te_mul(p, ca, cd, 12345, G))
    # the group law the expectations are about: (a + b) G = a G + b G
    assert cr.te_mul(p, ca, cd, 300, G) == cr.te_add(p, ca, cd, cr.te_mul(p, ca, cd, 100, G), cr.te_mul(p, ca, cd, 200, G))


@pytest.mark.parametrize("name", CURVES)
def test_honest_circuits_pass_the_check(name):
    p, ca, cd, G = setup(name)
    rng = random.Random(7)
    c = cr.RefComposer(p, ca, cd)
    x, y = c.add_input(rng.randrange(1 << 64)), c.add_input(rng.randrange(1 << 64))
    c.range_gate(x, 64)
    c.range_gate(y, 64)
    z = c.xor_gate(x, y, 64)
    c.constrain_to_constant(z, c.values[x] ^ c.values[y])
    w = c.and_gate(x, y, 10)
    s = c.arithmetic_gate(x, w, None, y, q_m=3, q_l=5, q_r=p - 2, q_c=9, q_4=4, pi=77)
    pt = c.fixed_base_scalar_mul(x, G)
    qx, qy = cr.te_mul(p, ca, cd, 5, G)
    pt2 = c.point_addition_gate(pt, (c.add_input(qx), c.add_input(qy)))
    want = cr.te_mul(p, ca, cd, c.values[x] + 5, G)
    c.constrain_to_constant(pt2[0], 0, -want[0])
    c.constrain_to_constant(pt2[1], 0, -want[1])
    c.boolean_gate(c.add_input(1))
    c.assert_equal(s, s)
    assert masks_of(name, c) == [0] * c.size()


@pytest.mark.parametrize("name", CURVES)
def test_shape_table(name):
    """rows, new variables and insertions per call: the table of DESIGN.md 6e, the sequential composer, and zk_gadget_shape"""
    p, ca, cd, G = setup(name)
    M = p.bit_length()
    cid = zk.get_curve(name).curve_id

    def lib_shape(kind, bits=0, flags=0, calls=1):
        r, v, i, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_size_t()
        assert _lib.lib().zk_gadget_shape(kind, cid, bits, flags, calls, ctypes.byref(r), ctypes.byref(v), ctypes.byref(i), ctypes.byref(w)) == 0
        return (r.value, v.value, i.value), w.value

    def measured(fn):
        c = cr.RefComposer(p, ca, cd)
        ins = [c.add_input(3), c.add_input(5), c.add_input(G[0]), c.add_input(G[1])]
        before = (c.n, len(c.values), len(c.ins_var))
        fn(c, ins)
        return c.n - before[0], len(c.values) - before[1], len(c.ins_var) - before[2]

    for bits in BITS:
        g = -(-bits // 8)
        want = (g + 2, bits // 2, 4 * g + 5)
        assert measured(lambda c, i: c.range_gate(i[0], bits)) == want == lib_shape(_lib.ZK_GADGET_RANGE, bits)[0], bits
        want = (bits // 2 + 1, 2 * bits, 2 * bits + 4)
        for flags, xor in ((_lib.ZK_GADGET_XOR, True), (0, False)):
            assert measured(lambda c, i: c.logic_gate(i[0], i[1], bits, xor)) == want == lib_shape(_lib.ZK_GADGET_LOGIC, bits, flags)[0], bits
    assert [lib_shape(_lib.ZK_GADGET_RANGE, b)[0][0] for b in (32, 34, 64, 254)] == [6, 7, 10, 34]
    assert measured(lambda c, i: c.arithmetic_gate(i[0], i[1], q_m=1)) == (1, 1, 4) == lib_shape(_lib.ZK_GADGET_POLY, 0, _lib.ZK_GADGET_COMPUTE_OUT)[0]
    for fn in (lambda c, i: c.boolean_gate(i[0]), lambda c, i: c.assert_equal(i[0], i[1]), lambda c, i: c.constrain_to_constant(i[0], 3)):
        assert measured(fn) == (1, 0, 4) == lib_shape(_lib.ZK_GADGET_POLY)[0]
    assert measured(lambda c, i: c.point_addition_gate((i[2], i[3]), (i[2], i[3]))) == (2, 3, 8) == lib_shape(_lib.ZK_GADGET_CURVE_ADD)[0]
    want = (M + 5, 4 * M + 3, 4 * (M + 5))
    shape, work = lib_shape(_lib.ZK_GADGET_FIXED_BASE, calls=7)
    assert measured(lambda c, i: c.fixed_base_scalar_mul(i[0], G)) == want == shape and work == 256 + 96 * (M + 1) * 7
    if name == "bls12_381":
        assert want[:2] == (260, 1023)
    # odd or out-of-range widths, unknown kinds and curves are refused
    L = _lib.lib()
    for kind, bits in ((_lib.ZK_GADGET_RANGE, 7), (_lib.ZK_GADGET_RANGE, 0), (_lib.ZK_GADGET_LOGIC, 258), (9, 8), (-1, 8)):
        assert L.zk_gadget_shape(kind, cid, bits, 0, 1, None, None, None, None) == _lib.ZK_ERR_BAD_ARG
    assert L.zk_gadget_shape(_lib.ZK_GADGET_RANGE, 7, 8, 0, 1, None, None, None, None) == _lib.ZK_ERR_BAD_ARG


@pytest.mark.parametrize("name", CURVES)
def test_range_and_logic_prefix_formula(name):
    """accumulator j of a range call, and the input prefixes of a logic call, are (v mod 2^bits) >> (bits - 2 (j + 1)); the output
    prefix is their ^ or & -- reduced, since from 255 bits up the XOR of two field elements can exceed the modulus"""
    p = cr.EMBEDDED[name][0]
    rng = random.Random(3)
    for bits in BITS:
        for v in [0, 1, (1 << bits) - 1, (1 << bits) % p, p - 1] + [rng.randrange(p) for _ in range(4)]:
            c = cr.RefComposer(p)
            x = c.add_input(v)
            first = len(c.values)
            c.range_gate(x, bits)
            got = c.values[first:first + bits // 2]
            assert got == [((v % p) % (1 << bits)) >> (bits - 2 * (j + 1)) for j in range(bits // 2)], (bits, v)
            w = rng.randrange(p)
            y = c.add_input(w)
            for xor in (True, False):
                first = len(c.values)
                c.logic_gate(x, y, bits, xor)
                for i in range(bits // 2):
                    s = bits - 2 * (i + 1)
                    a, b = ((v % p) % (1 << bits)) >> s, (w % (1 << bits)) >> s
                    assert c.values[first + 4 * i:first + 4 * i + 4] == [a, b, (a & 3) * (b & 3), ((a ^ b) if xor else (a & b)) % p]


@pytest.mark.parametrize("name", CURVES)
def test_naf_closed_form(name):
    """digit of weight 2^j of find_wnaf(2) = bit j+1 of 3e - bit j+1 of e; the digits before weight 2^t sum to (3e >> (t+1)) - (e >> (t+1));
    more than M digits iff 3e >= 2^(M+1) -- for BLS12-381's 255-bit field: iff 3e >= 2^256"""
    p = cr.EMBEDDED[name][0]
    M = p.bit_length()
    rng = random.Random(11)
    es = [0, 1, 2, 3, p - 1, (1 << 251), (1 << 256) // 3 % p, ((1 << (M + 1)) - 1) // 3, ((1 << (M + 1)) - 1) // 3 + 1]
    es += [rng.randrange(p) for _ in range(200)] + [rng.randrange(1 << 252) for _ in range(50)]
    long_seen = short_seen = 0
    for e in es:
        if e >= p:
            continue
        naf = cr.find_wnaf2(e)
        assert sum(d << j for j, d in enumerate(naf)) == e and all(d in (-1, 0, 1) for d in naf)
        digits = [((3 * e) >> (j + 1) & 1) - (e >> (j + 1) & 1) for j in range(258)]
        assert digits[:len(naf)] == naf and not any(digits[len(naf):])
        for t in (0, 1, 7, 100, M - 1, M):
            assert sum(d << (j - t) for j, d in enumerate(digits) if j >= t) == ((3 * e) >> (t + 1)) - (e >> (t + 1))
        assert (len(naf) > M) == (3 * e >= 1 << (M + 1))
        long_seen += len(naf) > M
        short_seen += len(naf) <= M
    assert long_seen and short_seen
    if name == "bls12_381":
        assert M + 1 == 256 and len(cr.find_wnaf2(p - 1)) > M
    with pytest.raises(cr.NafTooLong):
        c = cr.RefComposer(p, *cr.EMBEDDED[name][1:])
        c.fixed_base_scalar_mul(c.add_input(p - 1), cr.te_point(*cr.EMBEDDED[name]))


def test_fixture_is_data_of_the_listed_reference_tests():
    names = [c["name"] for c in CASES["cases"]]
    assert len(names) == len(set(names)) == 17 and CASES["reject_bit"] == "arith"
    for c in CASES["cases"]:
        assert c["expect"] in ("accept", "reject") and (c["expect"] == "reject") == bool(c["rows"]) and c["source"].split(":")[0].endswith(".rs")
    assert sum(c["expect"] == "reject" for c in CASES["cases"]) == 8


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("case", CASES["cases"], ids=lambda c: c["name"])
def test_reference_held_cases(name, case):
    """accept: every mask is zero; reject: the expected rows (the closing assert_equal / constant rows) carry `arith`, and nothing else
    is set anywhere"""
    p, ca, cd, G = setup(name)
    c = cr.RefComposer(p, ca, cd)
    cr.run_program(case["program"], cr.RefApi(c), p, ca, cd, G)
    got = {i: m for i, m in enumerate(masks_of(name, c)) if m}
    assert got == {c.n + r: 1 << ck.BIT[CASES["reject_bit"]] for r in case["rows"]}
