"""tests/circuit_check_ref.py -- the definition the device check is compared with -- against what the repository already trusts:
the widget identities of oracle/bigint_oracle.py (which the quotient kernel is pinned to) and the gadget rows `prover._gadget_runs`
builds (which the prover proves).  Exact integers, both curves, no GPU."""
import numpy as np
import pytest

from ark_plonk_amd import circuit_check, prover
from oracle import bigint_oracle as bo
from tests import circuit_check_ref as ref

CA, CD = 5, 7


def _rows(p):
    """the gadget rows of `_gadget_runs` from row 10 as full columns: (n, wires, selectors, gadget rows)"""
    cells, sels, gadget, end = prover._gadget_runs(p, 10, np.random.default_rng(5), CA, CD)
    n = end + 2
    wires = [[0] * n for _ in range(4)]
    for (w, r), v in cells.items():
        wires[w][r] = v
    sel = {name: [0] * n for name in ref.SELECTORS}
    for (name, r), v in sels.items():
        sel[name][r] = v
    return n, wires, sel, gadget


def _gate_masks(p, n, wires, sel):
    out = []
    for i in range(n):
        nx = (i + 1) % n
        q = {name: sel[name][i] for name in ref.SELECTORS}
        out.append(ref.gate_mask(p, wires[0][i], wires[1][i], wires[2][i], wires[3][i], wires[0][nx], wires[1][nx], wires[3][nx], q, 0, CA, CD))
    return out


def test_bit_names_agree():
    assert tuple(circuit_check.BIT_NAMES) == ref.NAMES and len(ref.NAMES) == 22


@pytest.mark.parametrize("cid", [0, 1])
def test_terms_recombine_to_the_oracle_identities(cid):
    """s * sum_j term_j k^j (k = s^2) of the reference's terms is the widget value the oracle -- and through it the quotient -- uses"""
    p = bo.CURVES[cid].r
    for seed in range(8):
        a, b, c, d, a_n, b_n, d_n, q_l, q_r, q_c, s, ca, cd = bo.seeded_scalars(bo.CURVES[cid], 900 + seed, 13)
        k = s * s % p
        comb = lambda ts: s * sum(t * pow(k, j, p) for j, t in enumerate(ts)) % p  # noqa: E731
        assert comb(ref.range_terms(p, a, b, c, d, d_n)) == bo.range_constraint(p, s, a, b, c, d, d_n)
        assert comb(ref.logic_terms(p, a, b, c, d, a_n, b_n, d_n, q_c)) == bo.logic_constraint(p, s, a, b, c, d, a_n, b_n, d_n, q_c)
        assert comb(ref.fixed_terms(p, a, b, c, d, a_n, b_n, d_n, q_l, q_r, q_c, ca, cd)) == \
            bo.fixed_base_constraint(p, s, a, b, c, d, a_n, b_n, d_n, q_l, q_r, q_c, ca, cd)
        assert comb(ref.curve_terms(p, a, b, c, d, a_n, b_n, d_n, ca, cd)) == bo.curve_add_constraint(p, s, a, b, c, d, a_n, b_n, d_n, ca, cd)
        q = dict(zip(ref.SELECTORS, bo.seeded_scalars(bo.CURVES[cid], 950 + seed, 12)))
        pi = q_l
        want = ((a * b * q["q_m"] + a * q["q_l"] + b * q["q_r"] + c * q["q_o"] + d * q["q_4"] + q["q_c"]) * q["q_arith"] + pi) % p   # quotient_at
        assert ref.arith_term(p, a, b, c, d, q, pi) == want


@pytest.mark.parametrize("cid", [0, 1])
def test_every_gadget_row_is_satisfied(cid):
    p = bo.CURVES[cid].r
    n, wires, sel, gadget = _rows(p)
    assert len(gadget) == 6 + 6 + 4 + 5
    assert sum(sel["q_range"]) == 6 and sum(1 for v in sel["q_logic"] if v) == 6
    assert sum(sel["q_variable_group_add"]) == 4 and sum(sel["q_fixed_group_add"]) == 5
    assert _gate_masks(p, n, wires, sel) == [0] * n


@pytest.mark.parametrize("cid", [0, 1])
def test_one_added_to_any_gadget_cell_is_seen(cid):
    p = bo.CURVES[cid].r
    n, wires, sel, gadget = _rows(p)
    for g in gadget:
        for w in range(4):
            bad = [list(col) for col in wires]
            bad[w][g] = (bad[w][g] + 1) % p
            ms = _gate_masks(p, n, bad, sel)
            assert ms[g] | ms[g - 1], (g, w)
            assert all(m == 0 for i, m in enumerate(ms) if i not in (g, g - 1)), (g, w)


def test_summary_of_the_reference():
    assert ref.summary([0, 0, 0]) == (0, 3, 0, [0] * 32)
    assert ref.summary([0, 6, 2, 0]) == (2, 1, 6, [0, 2, 1] + [0] * 29)
