"""GPU suite of the two gadget kinds behind lookup outputs and the benchmark circuit (ark_plonk_amd/composer.py: lookup_gate with
c=None, add_dummy_constraints, add_dummy_lookup_table, circuit_bound, bench_circuit; csrc/gadget_layout.hip: row_of; csrc/gadget_witness.hip:
gadget_w_select; csrc/lookup_map.hip for the witness of ZK_GADGET_LOOKUP_OUT): descriptions and values against the sequential model
(tests/lookup_out_ref.py), the reference's test_plookup_xor (constraint_system/lookup.rs:79-144) with computed outputs and the benchmark
circuit end to end (compile -> assign -> check_circuit -> prove -> the oracle's verifier), the refusal of a key the table lacks, a
replay inside an open deferred round and a table that changes between two assignments.  Every comparison is exact equality."""
import random

import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib
from ark_plonk_amd import compile as zc
from ark_plonk_amd.composer import LookupTable, bench_circuit
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont
from ark_plonk_amd.lookup import ElementNotIndexed
from oracle import bigint_oracle as bo
from tests import composer_ref as cr
from tests import composer_ref_ext as cx
from tests import lookup_out_ref as lr
from tests.test_composer_gpu import BLINDING, assert_equal_to_reference, assign, check_of, committer, dev_fr, prove_and_verify, setup

pytestmark = pytest.mark.gpu


def new_pair(cid, ctx):
    p, ca, cd, _ = setup(cid)
    return zk.Composer(cid, ctx, coeffs=(ca, cd)), lr.RefComposerLookupOut(p, ca, cd, BLINDING)


def assert_equal_with_table(cid, dev, ref, values):
    desc = assert_equal_to_reference(cid, dev, ref, values)
    assert len(desc.table_cols) == (4 if ref.lookup_table.size() else 0)
    for got, want in zip(desc.table_cols, ref.lookup_table.columns()):
        assert np.array_equal(got.cpu().numpy().view(np.uint64), fr_to_mont(cid, want))
    return desc


def values_of(cid, values, handle):
    return fr_from_mont(cid, values[handle.long()].cpu().numpy().view(np.uint64))


def idx(handle, picks):
    import torch
    return handle[torch.tensor(picks, device=handle.device)].contiguous()


# ---- 1. both kinds, per batch size: description and values equal the sequential composer's
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_segments_equal_the_reference_composer(cid, B, ctx):
    p, _, _, _ = setup(cid)
    rng = random.Random(10 * B + cid)
    dev, ref = new_pair(cid, ctx)
    for t in (dev.lookup_table, ref.lookup_table):
        t.insert_row(2, 3, 99, 0)                           # before the block's (2, 3, 5, 0): the first match
        t.insert_multi_add(0, 2)
        t.insert_multi_xor(0, 3)
        t.insert_row(7, 7, 1234, -1)                        # behind the block's (7, 7, 0, -1): never the answer
    xs, ys, us = ([rng.randrange(4) for _ in range(B)] for _ in range(3))
    ds = [rng.choice((0, p - 1)) for _ in range(B)]         # the tag of the add block, or of the xor block
    xs[0], ys[0], ds[0] = 2, 3, 0
    if B > 1:
        xs[-1], ys[-1], ds[-1] = 7, 7, p - 1
    x, y, d, u = (dev.inputs(B) for _ in range(4))
    rx, ry, rd, ru = ([ref.add_input(v) for v in col] for col in (xs, ys, ds, us))
    before = (dev.n_gates, dev.num_vars)
    c1 = dev.lookup_gate(x, y, None, d, pi=list(range(B)))
    r1 = [ref.lookup_gate(rx[k], ry[k], None, rd[k], k) for k in range(B)]
    assert c1.cpu().tolist() == r1 and (dev.n_gates, dev.num_vars) == (before[0] + B, before[1] + B)
    assert dev._program[-1][1]["kind"] == _lib.ZK_GADGET_LOOKUP_OUT
    c2 = dev.lookup_gate(u, 0)                              # b a constant handle, d=None: the zero variable, the tag of the add block
    r2 = [ref.lookup_gate(ru[k], 0) for k in range(B)]
    assert c2.cpu().tolist() == r2
    dev.add_dummy_constraints(B)
    for _ in range(B):
        ref.add_dummy_constraints()
    values, _ = assign(cid, dev, [xs, ys, ds, us])
    assert_equal_with_table(cid, dev, ref, values)
    assert values_of(cid, values, c1)[0] == 99 and values_of(cid, values, c2) == us
    if B > 1:
        assert values_of(cid, values, c1)[-1] == 0


# ---- 2. the reference's test_plookup_xor with computed outputs; an operand the table lacks
def plookup_xor(cid, ctx):
    """lookup.rs:79-144 as one segment of three calls: (rand1, rand2), (rand1, rand3), (rand2, rand3) against xor_table(0, 4)"""
    p, ca, cd, _ = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    dev.lookup_table = LookupTable.xor_table(0, 4)
    neg_one, r = dev.inputs(1), dev.inputs(3)
    row0 = dev.n_gates
    out = dev.lookup_gate(idx(r, [0, 0, 1]), idx(r, [1, 2, 2]), None, neg_one)
    dev.arithmetic_gate(idx(r, [0]), idx(r, [1]), q_l=1, q_r=1)
    dev.arithmetic_gate(idx(r, [1]), idx(r, [2]), q_m=1)
    return dev, out, row0


@pytest.mark.parametrize("cid", [0, 1])
def test_plookup_xor_with_computed_outputs(cid, ctx, oracle_cpu):
    import torch
    p, _, _, _ = setup(cid)
    rng = random.Random(79 + cid)
    dev, out, row0 = plookup_xor(cid, ctx)
    desc = dev.description()
    assert desc.size() == 256                               # the table's 256 rows bound the circuit
    ck = committer(ctx, oracle_cpu, cid, desc.size())
    pk, vk, pre = zc.compile(desc, ck, b"plookup xor", cid, ctx)
    for _ in range(2):
        r1, r2, r3 = (rng.randrange(16) for _ in range(3))
        values, pi_limbs = assign(cid, dev, [[p - 1], [r1, r2, r3]])
        assert values_of(cid, values, out) == [r1 ^ r2, r1 ^ r3, r2 ^ r3]
        wires = zc.assign(desc, values, ctx)
        rep = check_of(cid, ctx, pk, wires, pi_limbs)
        assert rep.ok, str(rep)
    ok, _ = prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, dict(dev.public_inputs), b"plookup xor", check=True)
    assert ok
    # one operand outside the table: calls 1 and 2 look up a key no row holds; the first of them is named, with its row
    with pytest.raises(ElementNotIndexed, match=rf"row {row0}: call 1 \(row {row0 + 1}\).*\(2 of 3 calls"):
        assign(cid, dev, [[p - 1], [3, 5, 16]])
    with pytest.raises(ElementNotIndexed, match=r"call 0 .*\(3 of 3 calls"):
        assign(cid, dev, [[0], [3, 5, 6]])                  # the tag of no block of this table
    values, pi_limbs = assign(cid, dev, [[p - 1], [3, 5, 15]])
    assert values_of(cid, values, out) == [6, 12, 10]
    assert check_of(cid, ctx, pk, zc.assign(desc, values, ctx), pi_limbs).ok
    torch.cuda.synchronize()
    ck.close()


# ---- 3. an explicit output: the segment lookup_gate has always produced
@pytest.mark.parametrize("cid", [0, 1])
def test_explicit_output_is_unchanged(cid, ctx):
    p, ca, cd, _ = setup(cid)
    B = 65
    rng = random.Random(3 + cid)
    dev, ref = zk.Composer(cid, ctx, coeffs=(ca, cd)), cx.RefComposerExt(p, ca, cd, BLINDING)
    dev.lookup_table.insert_multi_xor(0, 3)
    ref.lookup_table.insert_multi_xor(0, 3)
    cols = [[rng.randrange(8) for _ in range(B)] for _ in range(2)]
    cols += [[a ^ b for a, b in zip(*cols)], [p - 1] * B]
    h = [dev.inputs(B) for _ in range(4)]
    rh = [[ref.add_input(v) for v in col] for col in cols]
    before = dev.num_vars
    c = dev.lookup_gate(h[0], h[1], h[2], h[3], pi=7)
    assert c.cpu().tolist() == [ref.lookup_gate(rh[0][k], rh[1][k], rh[2][k], rh[3][k], 7) for k in range(B)]
    c = dev.lookup_gate(h[0], h[0], 0)                      # positional, d=None, a constant output
    assert c.cpu().tolist() == [ref.lookup_gate(rh[0][k], rh[0][k], 0) for k in range(B)]
    assert dev.num_vars == before and [s[1]["kind"] for s in dev._program[-2:]] == [_lib.ZK_GADGET_LOOKUP] * 2
    assert [s[1]["V"] for s in dev._program[-2:]] == [0, 0]
    values, _ = assign(cid, dev, cols)
    assert_equal_to_reference(cid, dev, ref, values)


# ---- 4. the benchmark circuit
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("log_n", [5, 10])
def test_bench_circuit(cid, log_n, ctx, oracle_cpu):
    import torch
    p, ca, cd, _ = setup(cid)
    dev = bench_circuit(log_n, cid, ctx, (ca, cd))
    ref = lr.RefComposerLookupOut(p, ca, cd, BLINDING)
    ref.bench_circuit(log_n)
    assert dev.n_gates == (1 << (log_n - 1)) + 2 == ref.n and dev.circuit_bound() == 1 << log_n == ref.circuit_bound()
    assert [w for w, *_ in dev._program] == ["segment"]     # ONE segment of dummy calls
    values, pi_limbs = assign(cid, dev, [])
    desc = assert_equal_with_table(cid, dev, ref, values)
    assert desc.size() == 1 << log_n
    one = fr_to_mont(cid, [1])[0]
    q_lookup = desc.selectors["q_lookup"].cpu().numpy().view(np.uint64)
    assert not q_lookup[:4].any() and (q_lookup[4:] == one).all() and q_lookup.shape[0] == dev.n_gates
    ck = committer(ctx, oracle_cpu, cid, desc.size())
    pk, vk, pre = zc.compile(desc, ck, b"bench circuit", cid, ctx)
    wires = zc.assign(desc, values, ctx)
    rep = check_of(cid, ctx, pk, wires, pi_limbs)
    assert rep.ok, str(rep)
    ok, _ = prove_and_verify(cid, ctx, pk, vk, pre, ck, wires, pi_limbs, {}, b"bench circuit", check=True)
    assert ok
    torch.cuda.synchronize()
    ck.close()


def test_bench_circuit_below_eight_rows(ctx):
    for log_n in (0, 1, 2, 3):
        dev = bench_circuit(log_n, 0, ctx)
        assert dev.n_gates == (6 if log_n == 3 else 4) and dev.lookup_table.size() == 3
    with pytest.raises(ValueError):
        dev.add_dummy_constraints(0)


# ---- 5. inside an open deferred round; a table that changes between two assignments
def test_lookup_out_inside_an_open_deferred_round(ctx, oracle_cpu):
    """a LOOKUP_OUT segment built, its table's map built and its witness replayed while a deferred round is open on the ctx: the same
    bytes as outside, and the round's commitments are what they are without the calls in between"""
    import torch
    cid = 0
    p, ca, cd, _ = setup(cid)
    rng = random.Random(19)
    xs, ys = [rng.randrange(8) for _ in range(70)], [rng.randrange(8) for _ in range(70)]

    def build():
        dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
        dev.lookup_table = LookupTable.xor_table(0, 3)
        x, y = dev.inputs(70), dev.inputs(70)
        out = dev.lookup_gate(x, y, None, dev.add_witness_to_circuit_description(-1))
        dev.lookup_gate(out, x, None, dev.add_witness_to_circuit_description(-1))
        dev.add_dummy_constraints(3)
        desc = dev.description()
        values, _ = assign(cid, dev, [xs, ys])
        assert values_of(cid, values, out) == [a ^ b for a, b in zip(xs, ys)]
        return [t.cpu().numpy().tobytes() for t in list(desc.wires) + [desc.selectors[k] for k in cr.SELECTORS] + [desc.ins_var, desc.ins_pos, values]]
    outside = build()
    ck = committer(ctx, oracle_cpu, cid, 64)
    polys = [dev_fr(cid, bo.seeded_scalars(bo.CURVES[cid], 700 + k, 64)) for k in range(2)]
    want = ck.commit_batch(polys)
    ck.commit_begin(polys)
    assert ck.round_pending() == 2
    inside = build()
    assert ck.round_pending() == 2
    assert ck.round_end(2) == want and inside == outside
    torch.cuda.synchronize()
    ck.close()


@pytest.mark.parametrize("cid", [0, 1])
def test_table_changes_between_assignments(cid, ctx):
    p, ca, cd, _ = setup(cid)
    dev = zk.Composer(cid, ctx, coeffs=(ca, cd))
    dev.lookup_table.insert_multi_add(0, 2)
    x, y = dev.inputs(65), dev.inputs(65)
    out = dev.lookup_gate(x, y)
    xs, ys = [k % 4 for k in range(65)], [(k // 4) % 4 for k in range(65)]
    values, _ = assign(cid, dev, [xs, ys])
    assert values_of(cid, values, out) == [(a + b) % 4 for a, b in zip(xs, ys)]
    kept = dev.lookup_table._dev
    assign(cid, dev, [ys, xs])
    assert dev.lookup_table._dev is kept                    # the columns and the map are reused
    xs[64], ys[64] = 9, 9
    with pytest.raises(ElementNotIndexed, match="call 64 "):
        assign(cid, dev, [xs, ys])
    dev.lookup_table.insert_row(9, 9, 81, 0)
    dev.lookup_table.insert_row(1, 2, 500, 0)               # behind the block's (1, 2, 3, 0): no call sees it
    assert dev.lookup_table._dev is None
    values, _ = assign(cid, dev, [xs, ys])
    assert values_of(cid, values, out) == [(a + b) % 4 for a, b in zip(xs[:64], ys[:64])] + [81]
