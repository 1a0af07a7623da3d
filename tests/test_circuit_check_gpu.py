"""GPU suite of the circuit check: zk_circuit_check_dev through `ark_plonk_amd.circuit_check` against the definition on Python integers
(tests/circuit_check_ref.py).  Every comparison is exact equality: the device mask on ALL rows, the whole summary."""
import numpy as np
import pytest

import ark_plonk_amd as zk
from ark_plonk_amd import _lib, circuit_check, prover, transcript
from ark_plonk_amd import compile as zc
from ark_plonk_amd.curves import fr_from_mont, fr_to_mont
from oracle import bigint_oracle as bo
from tests import circuit_check_ref as ref
from tests.conftest import srs_from_powers, tau_powers

pytestmark = pytest.mark.gpu

CA, CD = 1, 1          # `prover.example_circuit`'s default embedded-curve coefficients


def dev_fr(cid, ints):
    import torch
    return torch.from_numpy(fr_to_mont(cid, ints).view(np.int64)).cuda()


def to_ints(cid, t):
    return fr_from_mont(cid, t.cpu().numpy().view(np.uint64).reshape(-1, 4))


def identity_sigma(cid, log_n):
    cv = bo.CURVES[cid]
    w, n = cv.root_of_unity(log_n), 1 << log_n
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % cv.r
    return [[k * x % cv.r for x in pw] for k in ref.K]


class Circ:
    """A circuit and a witness as integer columns, with their device copies made on demand.  Columns: ("w", k) wires, ("q", name)
    selectors, ("s", k) sigma, ("t", k) table, ("pi",)."""

    def __init__(self, cid, log_n, cols, table_rows, ca=CA, cd=CD, dev=None):
        self.cid, self.log_n, self.n = cid, log_n, 1 << log_n
        self.cols, self.table_rows, self.ca, self.cd = cols, table_rows, ca, cd
        self.dev = dict(dev or {})

    @classmethod
    def blank(cls, cid, log_n, table_rows=0):
        n = 1 << log_n
        cols = {("w", k): [0] * n for k in range(4)}
        cols.update({("q", name): [0] * n for name in ref.SELECTORS})
        cols.update({("s", k): col for k, col in enumerate(identity_sigma(cid, log_n))})
        cols.update({("t", k): [0] * max(table_rows, 1) for k in range(4)})
        cols[("pi",)] = [0] * n
        return cls(cid, log_n, cols, table_rows)

    @classmethod
    def from_example(cls, cid, log_n, ctx):
        """`prover.example_circuit` pulled back to integers (the eleven selector columns the key does not keep: its exact NTT)"""
        pk, wires, pub = prover.example_circuit(log_n, cid, ctx)
        n = 1 << log_n
        dev = {("w", k): wires[k] for k in range(4)}
        dev.update({("q", name): t for name, t in circuit_check.selector_evaluations(pk).items()})
        dev.update({("s", k): pk.sigma_evals[k] for k in range(4)})
        dev.update({("t", k): pk.table_cols[k] for k in range(4)})
        cols = {key: to_ints(cid, t) for key, t in dev.items()}
        pi = [0] * n
        for i, v in pub.items():
            pi[i] = fr_from_mont(cid, np.asarray(v).reshape(1, 4))[0]
        cols[("pi",)] = pi
        c = cls(cid, log_n, cols, n, dev=dev)
        c.pk, c.wires, c.pub = pk, wires, pub
        return c

    def changed(self, *changes):
        """a copy with cells replaced: (column key, row, value) each; the device copies of untouched columns are shared"""
        cols, dev = dict(self.cols), dict(self.dev)
        for key, row, value in changes:
            if cols[key] is self.cols[key]:
                cols[key] = list(cols[key])
            cols[key][row] = value % bo.CURVES[self.cid].r
            dev.pop(key, None)
        return Circ(self.cid, self.log_n, cols, self.table_rows, self.ca, self.cd, dev)

    def tensor(self, key):
        if key not in self.dev:
            self.dev[key] = dev_fr(self.cid, self.cols[key])
        return self.dev[key]

    def reference(self):
        cv = bo.CURVES[self.cid]
        c = self.cols
        ms = ref.masks(cv.r, cv.root_of_unity(self.log_n), self.n, [c[("w", k)] for k in range(4)], {name: c[("q", name)] for name in ref.SELECTORS},
                       c[("pi",)], [c[("s", k)] for k in range(4)], [c[("t", k)] for k in range(4)], self.table_rows, self.ca, self.cd)
        return ms, ref.summary(ms)

    def device(self, ctx, table_rows=None):
        import torch
        mask, s = circuit_check.check_columns(
            zk.get_curve(self.cid), self.log_n, [self.tensor(("w", k)) for k in range(4)], {name: self.tensor(("q", name)) for name in ref.SELECTORS},
            [self.tensor(("s", k)) for k in range(4)], [self.tensor(("t", k)) for k in range(4)], self.table_rows if table_rows is None else table_rows,
            self.tensor(("pi",)), fr_to_mont(self.cid, [self.ca])[0], fr_to_mont(self.cid, [self.cd])[0], ctx)
        torch.cuda.synchronize()
        return mask.cpu().numpy().view(np.uint32).tolist(), (int(s.failing_rows), int(s.first_row), int(s.first_mask), [int(v) for v in s.bit_count])

    def agree(self, ctx):
        """device == definition on all rows and in the summary; returns the masks"""
        want, want_sum = self.reference()
        got, got_sum = self.device(ctx)
        bad = [i for i in range(self.n) if got[i] != want[i]]
        assert not bad, [(i, hex(got[i]), hex(want[i])) for i in bad[:8]]
        assert got_sum == want_sum
        return want


_examples = {}


def example(cid, log_n, ctx):
    """one pull-back of the example circuit per (curve, size) for the whole session; tests work on copies"""
    if (cid, log_n) not in _examples:
        _examples[(cid, log_n)] = Circ.from_example(cid, log_n, ctx)
    return _examples[(cid, log_n)]


def committer(ctx, oracle_cpu, cid, n):
    pw_canon, _ = tau_powers(oracle_cpu, cid, n + 8)
    return zk.CommitterKey(srs_from_powers(ctx, cid, pw_canon), cid, ctx)


def coeffs(cid):
    return fr_to_mont(cid, [CA])[0], fr_to_mont(cid, [CD])[0]


# ---- 1. satisfied circuits
@pytest.mark.parametrize("cid", [0, 1])
def test_satisfied_example_circuit(cid, ctx):
    import torch
    c = example(cid, 7, ctx)
    for name in ("q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup"):
        assert any(c.cols[("q", name)]), name                                 # 128 rows: the smallest size that carries every gate kind
    assert sum(1 for k in range(4) for i in range(c.n) if c.cols[("s", k)][i] != identity_sigma(cid, 7)[k][i]) == 12      # six 2-cycles
    rep = zk.check_circuit(c.pk, c.wires, c.pub, *coeffs(cid), ctx=ctx)
    assert rep.ok and rep.failing_rows == 0 and rep.first_row == c.n and rep.rows() == [] and not any(rep.counts.values())
    assert rep.mask.dtype == torch.int32 and rep.mask.shape == (c.n,) and torch.count_nonzero(rep.mask).item() == 0
    assert "satisfied" in str(rep)
    assert c.agree(ctx) == [0] * c.n                                            # ... and the definition says the same of these columns


def variable_circuit(cid, log_n, seed):
    """Gates by variable ids (the shape of the compile suite's circuit): a, b, d of an arithmetic gate are earlier outputs or variable 0,
    c a fresh variable set to the gate's value; every third row looks a table row up; public inputs on rows 1 and 3."""
    cv = bo.CURVES[cid]
    p, n = cv.r, 1 << log_n
    g = n - 3
    rng = np.random.default_rng(seed)
    rnd = lambda k, s: bo.seeded_scalars(cv, seed * 1000 + s, k)  # noqa: E731
    rows = max(n // 4, 2)
    tcols = [rnd(rows, 10 + k) for k in range(4)]
    qs = {name: rnd(g, 20 + k) for k, name in enumerate(("q_m", "q_l", "q_r", "q_4", "q_c"))}
    fresh = rnd(4 * g, 30)
    sel = {name: [0] * g for name in prover.SELECTORS}
    values, outs = [0], []
    w = [[0] * g for _ in range(4)]
    pub = {1: rnd(1, 40)[0], 3: rnd(1, 41)[0]}

    def new(v):
        values.append(v % p)
        return len(values) - 1
    for i in range(g):
        if i % 3 == 2 and i > 4:
            j = int(rng.integers(0, rows))
            for k in range(4):
                w[k][i] = new(tcols[k][j])
            sel["q_lookup"][i] = 1
            continue
        pick = lambda t: (outs[int(rng.integers(0, len(outs)))] if outs and rng.integers(0, 4) else (0 if outs else new(fresh[4 * i + t])))  # noqa: E731
        a, b, d = pick(0), pick(1), pick(2)
        for name in qs:
            sel[name][i] = qs[name][i]
        sel["q_o"][i], sel["q_arith"][i] = p - 1, 1
        va, vb, vd = values[a], values[b], values[d]
        c = new(qs["q_m"][i] * va * vb + qs["q_l"][i] * va + qs["q_r"][i] * vb + qs["q_4"][i] * vd + qs["q_c"][i] + pub.get(i, 0))
        outs.append(c)
        w[0][i], w[1][i], w[2][i], w[3][i] = a, b, c, d
    desc = zc.CircuitDescription.from_gates({k: dev_fr(cid, v) for k, v in sel.items()}, *w, num_vars=len(values),
                                            table_cols=[dev_fr(cid, t) for t in tcols],
                                            public_inputs={i: fr_to_mont(cid, [v])[0] for i, v in pub.items()}, curve=cid)
    return desc, values, outs[len(outs) // 2]


@pytest.mark.parametrize("cid", [0, 1])
def test_satisfied_through_compile_and_assign(cid, ctx, oracle_cpu):
    log_n = 5
    desc, values, an_output = variable_circuit(cid, log_n, 3)
    pk, _, _ = zc.compile(desc, committer(ctx, oracle_cpu, cid, 1 << log_n), curve=cid, ctx=ctx)
    wires = zc.assign(desc, dev_fr(cid, values), ctx)
    rep = zk.check_circuit(pk, wires, desc.public_inputs, *coeffs(cid), ctx=ctx)
    assert rep.ok and rep.first_row == 1 << log_n, str(rep)
    values[an_output] += 1                                                      # one variable: every cell that holds it moves together
    rep = zk.check_circuit(pk, zc.assign(desc, dev_fr(cid, values), ctx), desc.public_inputs, *coeffs(cid), ctx=ctx)
    assert not rep.ok and rep.counts["arith"] >= 1 and not any(rep.counts[k] for k in ("copy_l", "copy_r", "copy_o", "copy_4")), str(rep)


# ---- 2. single faults at 2^7
def fault_list(c):
    """about 40 single changes of the satisfied example circuit: (label, changes)"""
    cid, n = c.cid, c.n
    p = bo.CURVES[cid].r
    _, _, gadget, _ = prover._gadget_runs(p, n - 5 - 48, np.random.default_rng(99), CA, CD)       # the rows example_circuit placed
    rng = np.random.default_rng(2024)
    kinds = {"range": gadget[0], "range_last": gadget[5], "logic": gadget[8], "curve": gadget[13], "fixed": gadget[18]}
    out = []
    for label, row in kinds.items():
        for k in range(4):
            out.append((f"{label} row {row} wire {k}", [(("w", k), row, c.cols[("w", k)][row] + 1)]))
    ident = identity_sigma(cid, c.log_n)
    tied = [(k, i) for k in range(4) for i in range(n) if c.cols[("s", k)][i] != ident[k][i]]
    live = next(i for i in range(5, n) if c.cols[("q", "q_arith")][i] and all((k, i) not in tied for k in range(4)))
    for k in range(4):
        out.append((f"arithmetic row {live} wire {k}", [(("w", k), live, c.cols[("w", k)][live] + int(rng.integers(1, 1 << 30)))]))
    out.append(("public input 1", [(("pi",), 1, c.cols[("pi",)][1] + 1)]))
    for k, i in (tied[0], tied[-1]):
        out.append((f"tied cell wire {k} row {i}", [(("w", k), i, c.cols[("w", k)][i] + 1)]))
    look = next(i for i in range(n) if c.cols[("q", "q_lookup")][i])
    for k in range(4):
        out.append((f"lookup row {look} wire {k}", [(("w", k), look, c.cols[("w", k)][look] + 1)]))
    # a selector switched on in a padding row: the last row's "next row" is row 0, the one before sees only zeros
    for name in ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup"):
        out.append((f"{name} on in row {n - 1}", [(("q", name), n - 1, 1)]))
    out.append((f"q_lookup on in row {n - 2}", [(("q", "q_lookup"), n - 2, 1)]))
    assert 35 <= len(out) <= 45
    return out, tied


@pytest.mark.parametrize("cid", [0, 1])
def test_single_faults_match_the_definition(cid, ctx):
    c = example(cid, 7, ctx)
    faults, tied = fault_list(c)
    seen = 0
    for label, changes in faults:
        bad = c.changed(*changes)
        want = bad.agree(ctx)
        assert any(want), label                                                 # the case tests something
        seen |= int(np.bitwise_or.reduce(np.array(want, dtype=np.uint32)))
        if label.startswith("tied"):
            (key, row, _), = changes
            k2, r2 = next((k, i) for k, i in tied if c.cols[("s", k)][i] == identity_sigma(cid, 7)[key[1]][row])
            assert want[row] >> (18 + key[1]) & 1 and want[r2] >> (18 + k2) & 1, label      # both cells of the 2-cycle
    for group in (0x1, 0x1E, 0x3E0, 0x3C00, 0x1C000, 0x20000, 0x3C0000):       # arith, range, logic, fixed, curve, lookup, copy
        assert seen & group, (hex(seen), hex(group))


# ---- 3. the last row's next row is row 0
@pytest.mark.parametrize("cid", [0, 1])
def test_wrap_around(cid, ctx):
    p = bo.CURVES[cid].r
    c = Circ.blank(cid, 3)
    d7 = bo.seeded_scalars(bo.CURVES[cid], 77, 1)[0]
    c7 = 4 * d7 + 3
    b7 = 4 * c7 + 0
    a7 = 4 * b7 + 2
    c = c.changed((("q", "q_range"), 7, 1), (("w", 3), 7, d7), (("w", 2), 7, c7), (("w", 1), 7, b7), (("w", 0), 7, a7), (("w", 3), 0, 4 * a7 + 1))
    assert c.agree(ctx) == [0] * 8
    want = c.changed((("w", 3), 0, 4 * a7 + 1 + 4)).agree(ctx)                    # digit 5: out of range whatever it was
    assert want == [0] * 7 + [1 << 4]
    assert (4 * a7 + 5) % p != (4 * a7 + 1) % p


# ---- 4. operands at the edge of the field
@pytest.mark.parametrize("cid", [0, 1])
def test_edge_operands(cid, ctx):
    r = bo.CURVES[cid].r
    rows = [   # (selectors, wires a b c d, pi): each satisfied
        ({"q_m": 1, "q_o": r - 1}, (r - 1, r - 1, 1, 0), 0),
        ({"q_l": r - 1, "q_c": r - 1}, (r - 1, 0, 0, 0), 0),
        ({"q_m": r - 1, "q_c": 2}, (r - 1, r - 2, 0, 0), 0),
        ({"q_4": r - 2, "q_o": r - 1}, (0, 0, 2, r - 1), 0),
        ({}, (0, 0, 0, 0), 0),
        ({"q_r": 1, "q_c": r - 1}, (0, 1, 0, 0), 0),
        ({"q_c": r - 1}, (r - 1, r - 1, r - 1, r - 1), 1),
        ({"q_l": 1, "q_c": r - 1, "q_arith": r - 1}, (1, r - 2, r - 1, 1), 0),
    ]
    changes = []
    for i, (sel, w, pi) in enumerate(rows):
        changes += [(("q", name), i, v) for name, v in dict({"q_arith": 1}, **sel).items()]
        changes += [(("w", k), i, w[k]) for k in range(4)] + [(("pi",), i, pi)]
    c = Circ.blank(cid, 3).changed(*changes)
    assert c.agree(ctx) == [0] * 8
    off = c.changed(*[(("q", "q_c"), i, c.cols[("q", "q_c")][i] + 1) for i in range(8)])
    assert off.agree(ctx) == [1] * 8
    off = c.changed(*[(("pi",), i, c.cols[("pi",)][i] + r - 1) for i in range(8)])
    assert off.agree(ctx) == [1] * 8
    moved = c.changed((("w", 0), 0, r - 2), (("w", 0), 1, 0), (("w", 1), 2, r - 1), (("w", 3), 3, 0), (("w", 1), 5, 2), (("w", 0), 7, 0))
    assert moved.agree(ctx) == [1, 1, 1, 1, 0, 1, 0, 1]


# ---- 5. lookups
def test_lookup_membership(ctx):
    cid, log_n = 0, 10
    n = 1 << log_n
    x, y, z = bo.seeded_scalars(bo.CURVES[cid], 5, 3)
    t3 = bo.seeded_scalars(bo.CURVES[cid], 6, n)
    assert len(set(t3)) == n
    rng = np.random.default_rng(8)
    pick = [int(v) for v in rng.integers(0, n, n)]
    cols = Circ.blank(cid, log_n, n).cols
    cols.update({("t", 0): [x] * n, ("t", 1): [y] * n, ("t", 2): [z] * n, ("t", 3): t3,
                 ("w", 0): [x] * n, ("w", 1): [y] * n, ("w", 2): [z] * n, ("w", 3): [t3[j] for j in pick], ("q", "q_lookup"): [1] * n})
    # rows without a lookup gate may hold anything
    for i in (3, 500, n - 1):
        cols[("q", "q_lookup")][i] = 0
        cols[("w", 3)][i] = 12345
    c = Circ(cid, log_n, cols, n)
    assert c.agree(ctx) == [0] * n                                              # every query present
    near = c.changed((("w", 0), 10, x + 1), (("w", 1), 11, y + 1), (("w", 2), 12, z + 1), (("w", 3), 13, t3[0] + 1 if t3[0] + 1 not in t3 else 1),
                     (("w", 3), 700, 0))
    want = near.agree(ctx)                                                      # equal to a table row in three of four columns
    assert [i for i, m in enumerate(want) if m] == [10, 11, 12, 13, 700] and all(want[i] == 1 << 17 for i in (10, 11, 12, 13, 700))
    # a table padded with repeats of its first row
    rows = n // 4
    padded = dict(c.cols)
    padded[("t", 3)] = t3[:rows] + [t3[0]] * (n - rows)
    padded[("w", 3)] = [t3[j % rows] for j in pick]
    padded[("w", 3)][20] = t3[rows]                                             # a row the padding pushed out
    want = Circ(cid, log_n, padded, n).agree(ctx)
    assert [i for i, m in enumerate(want) if m] == [20]
    # no table at all: every lookup row fails
    empty = Circ(cid, log_n, c.cols, 0, dev=c.dev)
    want = empty.agree(ctx)
    assert want == [(1 << 17) * q for q in c.cols[("q", "q_lookup")]]


# ---- 6. sigma
@pytest.mark.parametrize("cid", [0, 1])
def test_three_cycle_and_a_bad_sigma_entry(cid, ctx):
    ident = identity_sigma(cid, 3)
    cells = [(0, 1), (2, 5), (3, 2)]
    vals = bo.seeded_scalars(bo.CURVES[cid], 31, 33)
    changes = [(("w", k), i, vals[4 * i + k]) for k in range(4) for i in range(8)]
    changes += [(("w", k), i, vals[32]) for k, i in cells]
    changes += [(("s", k), i, ident[k2][i2]) for (k, i), (k2, i2) in zip(cells, cells[1:] + cells[:1])]
    c = Circ.blank(cid, 3).changed(*changes)
    assert c.agree(ctx) == [0] * 8
    want = c.changed((("w", 2), 5, vals[32] + 1)).agree(ctx)
    assert want == [0, 1 << 18, 0, 0, 0, 1 << 20, 0, 0]                         # the cell that points at it, and the cell itself
    bad = c.changed((("s", 1), 4, 5))                                           # 5 = K_w omega^row for no (w, row) of this domain
    with pytest.raises(ref.NotAnEncoding):
        bad.reference()
    with pytest.raises(_lib.ZkError) as e:
        bad.device(ctx)
    assert e.value.code == _lib.ZK_ERR_BAD_ARG
    assert c.agree(ctx) == [0] * 8                                              # the ctx is as usable as before


# ---- 7. many workgroups
def test_many_faults_at_two_to_the_fourteen(ctx):
    cid, log_n = 0, 14
    c = example(cid, log_n, ctx)
    rng = np.random.default_rng(64)
    cells = {(int(k), int(i)) for k, i in zip(rng.integers(0, 4, 64), rng.integers(0, c.n, 64))}
    bad = c.changed(*[(("w", k), i, c.cols[("w", k)][i] + 1) for k, i in sorted(cells)])
    want = bad.agree(ctx)
    assert sum(1 for m in want if m) >= 32
    import torch
    rep = circuit_check.CheckReport(c.n, torch.tensor(np.array(want, dtype=np.uint32).view(np.int32)).cuda(), _summary_struct(ref.summary(want)))
    rows = rep.rows(None)
    assert [r for r, _ in rows] == [i for i, m in enumerate(want) if m]
    assert all(names == [ref.NAMES[b] for b in range(22) if want[r] >> b & 1] for r, names in rows)
    assert f"row {rows[0][0]}: " in str(rep) and "more" in str(rep)


def _summary_struct(s):
    out = _lib.CircuitCheckSummary()
    out.failing_rows, out.first_row, out.first_mask = s[0], s[1], s[2]
    for b in range(32):
        out.bit_count[b] = s[3][b]
    return out


# ---- 8. prove(check=True)
def test_prove_with_check(ctx, oracle_cpu):
    cid, log_n = 0, 7
    c = example(cid, log_n, ctx)
    ck = committer(ctx, oracle_cpu, cid, c.n)
    vk = c.pk.verifier_key(ck)
    pre = transcript.seed_transcript(transcript.Transcript(b"circuit check", cid), vk, c.n)
    ca, cd = coeffs(cid)
    good = prover.prove(c.pk, ck, c.wires, c.pub, pre, ca, cd)
    assert prover.check_identity(c.pk, good, c.pub)
    assert prover.prove(c.pk, ck, c.wires, c.pub, pre, ca, cd, check=True).to_bytes() == good.to_bytes()
    faults, _ = fault_list(c)
    chosen = [f for f in faults if f[0].startswith(("range row", "arithmetic row", "tied cell"))][1::4][:3]
    assert len(chosen) == 3
    for label, changes in chosen:
        bad = c.changed(*changes)
        wires = [bad.tensor(("w", k)) for k in range(4)]
        with pytest.raises(zk.CircuitNotSatisfied) as e:
            prover.prove(c.pk, ck, wires, c.pub, pre, ca, cd, check=True)
        assert not e.value.report.ok and e.value.report.first_row == bad.reference()[1][1], label
        assert ck.round_pending() == 0
        assert not prover.check_identity(c.pk, prover.prove(c.pk, ck, wires, c.pub, pre, ca, cd), c.pub), label   # what the prover enforces


# ---- 9. inside an open deferred round
def test_inside_an_open_round(ctx, oracle_cpu):
    cid, log_n = 0, 7
    c = example(cid, log_n, ctx)
    ck = committer(ctx, oracle_cpu, cid, c.n)
    polys = [c.pk.polys["q_m"], c.pk.sigma_polys[1]]
    ck.commit_begin(polys)
    undisturbed = ck.round_end(2)
    ck.commit_begin(polys)
    try:
        assert ck.round_pending() == 2
        rep = zk.check_circuit(c.pk, c.wires, c.pub, *coeffs(cid), ctx=ctx)
        assert rep.ok and ck.round_pending() == 2
        pts = ck.round_end(2)
    finally:
        if ck.round_pending():
            ck.round_abort()
    assert pts == undisturbed
