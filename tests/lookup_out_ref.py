"""Helper of tests/test_lookup_out*.py and tests/test_lookup_map_gpu.py (no test): the reference's composer restated sequentially
(tests/composer_ref.py, tests/composer_ref_ext.py) with what the benchmark circuit and a lookup with a computed output need --
composer.rs:493-574 (add_dummy_constraints, add_dummy_lookup_table), constraint_system/lookup.rs:18-65 with
`c = add_input(lookup_table.lookup(a, b, d)?)` (lookup/lookup_table.rs:172-180: a scan for the FIRST matching row), composer.rs:
131-138 (circuit_bound) and benches/plonk.rs:45-68 (BenchCircuit::gadget, with its while loop) -- and the first-match scan over
stored words that the standalone map is compared with.  Independent of ark_plonk_amd/composer.py and csrc/lookup_map.hip."""
from tests import composer_ref_ext as cx


class ElementNotIndexed(KeyError):
    """`Error::ElementNotIndexed`"""


def first_match(rows, a, b, d):
    """index of the first row (a, b, c, d) of `rows` with these a, b, d, or None: `.position(..)` of lookup_table.rs:172-180"""
    for i, row in enumerate(rows):
        if row[0] == a and row[1] == b and row[3] == d:
            return i
    return None


class RefComposerLookupOut(cx.RefComposerExt):
    """`tests/composer_ref.RefComposer` (through its extension, which holds the lookup table) with the dummy rows, a lookup gate
    whose output is computed, and the benchmark circuit"""

    def add_dummy_constraints(self):
        six, one, seven, min_twenty = self.add_input(6), self.add_input(1), self.add_input(7), self.add_input(-20)
        self._row([six, seven, min_twenty, one], {"q_m": 1, "q_l": 2, "q_r": 3, "q_o": 4, "q_c": 4, "q_4": 1, "q_arith": 1, "q_lookup": 1})
        self._map4([six, seven, min_twenty, one])
        self._row([min_twenty, six, seven, 0], {"q_m": 1, "q_l": 1, "q_r": 1, "q_o": 1, "q_c": 127, "q_4": 0, "q_arith": 1, "q_lookup": 1})
        self._map4([min_twenty, six, seven, 0])

    def add_dummy_lookup_table(self):
        self.lookup_table.insert_row(6, 7, -20, 1)
        self.lookup_table.insert_row(-20, 6, 7, 0)
        self.lookup_table.insert_row(3, 1, 4, 9)

    def lookup_gate(self, a, b, c=None, d=None, pi=None):
        if c is None:
            v = self.values
            i = first_match(self.lookup_table.rows, v[a], v[b], v[0 if d is None else d])
            if i is None:
                raise ElementNotIndexed((v[a], v[b], v[0 if d is None else d]))
            c = self.add_input(self.lookup_table.rows[i][2])
        return super().lookup_gate(a, b, c, d, pi)

    def circuit_bound(self):
        return self.size()

    def bench_circuit(self, log_n):
        self.add_dummy_lookup_table()
        while self.circuit_bound() < (1 << log_n) - 1:
            self.add_dummy_constraints()
