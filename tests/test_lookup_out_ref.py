"""CPU suite of the model tests/lookup_out_ref.py and of the host-only entry points behind the lookup output and the benchmark
circuit: the dummy rows satisfy what they must, the benchmark circuit has the size the reference's loop gives, `zk_gadget_shape` knows
the two new kinds and `zk_lookup_map_slots` the capacity of a map."""
import ctypes

import pytest

from ark_plonk_amd import _lib
from tests import composer_ref as cr
from tests import lookup_out_ref as lr

NAMES = {0: "bls12_381", 1: "bn254"}


def new_ref(cid):
    p, ca, cd = cr.EMBEDDED[NAMES[cid]]
    return lr.RefComposerLookupOut(p, ca, cd)


@pytest.mark.parametrize("cid", [0, 1])
def test_dummy_rows_satisfy_the_gate_and_are_table_rows(cid):
    ref = new_ref(cid)
    p, n0 = ref.p, ref.n
    ref.add_dummy_lookup_table()
    ref.add_dummy_constraints()
    ref.add_dummy_constraints()
    assert ref.n == n0 + 4 and ref.lookup_table.size() == 3
    for row in range(n0, ref.n):
        a, b, c, d = (ref.values[ref.w[k][row]] for k in range(4))
        q = {name: ref.q[name][row] for name in cr.SELECTORS}
        assert (q["q_m"] * a * b + q["q_l"] * a + q["q_r"] * b + q["q_o"] * c + q["q_4"] * d + q["q_c"]) % p == 0, row
        assert q["q_arith"] == 1 and q["q_lookup"] == 1
        assert all(q[name] == 0 for name in ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add"))
        assert [a, b, c, d] in ref.lookup_table.rows, row
        assert lr.first_match(ref.lookup_table.rows, a, b, d) == (row - n0) % 2
    assert ref.values[-4:] == [6, 1, 7, p - 20]
    # the eight insertions of a call, in the reference's order (composer.rs:515-546)
    v = len(ref.values) - 4
    assert ref.ins_var[-8:] == [v, v + 2, v + 3, v + 1, v + 3, v, v + 2, 0]
    assert ref.ins_wire[-8:] == [0, 1, 2, 3] * 2 and ref.ins_row[-8:] == [ref.n - 2] * 4 + [ref.n - 1] * 4


@pytest.mark.parametrize("cid", [0, 1])
def test_bench_circuit_gate_counts(cid):
    for k in range(0, 13):
        ref = new_ref(cid)
        ref.bench_circuit(k)
        assert ref.n == ((1 << (k - 1)) + 2 if k >= 3 else 4), k
        assert ref.circuit_bound() == max(1 << k, 4), k
        assert len(ref.values) == 9 + 2 * (ref.n - 4)


def test_computed_lookup_output_is_the_first_match():
    ref = new_ref(0)
    t = ref.lookup_table
    t.insert_row(1, 2, 30, 4)
    t.insert_row(1, 2, 31, 4)                          # the same key, another c: legal, and never returned
    t.insert_row(1, 2, 32, 5)
    a, b, d4, d5 = ref.add_input(1), ref.add_input(2), ref.add_input(4), ref.add_input(5)
    assert ref.values[ref.lookup_gate(a, b, None, d4)] == 30
    assert ref.values[ref.lookup_gate(a, b, None, d5)] == 32
    with pytest.raises(lr.ElementNotIndexed):
        ref.lookup_gate(a, b)                          # d = the zero variable
    with pytest.raises(lr.ElementNotIndexed):
        ref.lookup_gate(b, a, None, d4)


@pytest.mark.parametrize("cid", [0, 1])
def test_gadget_shape_knows_the_new_kinds(cid):
    L = _lib.lib()

    def shape(kind):
        r, v, i, w = _lib.c_u32(), _lib.c_u32(), _lib.c_u32(), _lib.c_size_t()
        rc = L.zk_gadget_shape(kind, cid, 0, 0, 1000, ctypes.byref(r), ctypes.byref(v), ctypes.byref(i), ctypes.byref(w))
        return rc, (r.value, v.value, i.value), w.value
    assert shape(_lib.ZK_GADGET_LOOKUP_OUT) == (0, (1, 1, 4), 256) and _lib.ZK_GADGET_LOOKUP_OUT == 15
    assert shape(_lib.ZK_GADGET_DUMMY) == (0, (2, 4, 8), 256) and _lib.ZK_GADGET_DUMMY == 16
    for kind in (9, 14, -1, 17):                            # 14 = ZK_GADGET_LOOKUP + 1 names no kind, like 9
        assert shape(kind)[0] == _lib.ZK_ERR_BAD_ARG, kind
    assert ctypes.sizeof(_lib.GadgetArgs) == 480            # 424 before; four columns, a row count, the map, its slot count appended
    assert _lib.GadgetArgs.lut.offset == 424 and _lib.GadgetArgs.inputs_ext.offset == 392


def test_map_slot_count():
    L = _lib.lib()
    for rows in (0, 1, 511, 512, 513):
        s = L.zk_lookup_map_slots(rows)
        assert s >= 2 * rows and s >= 64 and s & (s - 1) == 0 and (s == 64 or s < 4 * rows), (rows, s)
    assert [L.zk_lookup_map_slots(r) for r in (511, 512, 513)] == [1024, 1024, 2048]
    assert L.zk_lookup_map_slots(1 << 30) == 1 << 31 and L.zk_lookup_map_slots((1 << 30) + 1) == 0
