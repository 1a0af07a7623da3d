"""Helper of tests/test_composer_ref_ext.py and tests/test_composer_ext_gpu.py (no test): the gadgets of the reference's
`StandardComposer` that tests/composer_ref.py leaves out, restated call by call on Python integers from plonk-core/src/ --
constraint_system/composer.rs:192-196 (add_witness_to_circuit_description), 355-392 (is_zero_with_output, is_eq_with_output), 404-488
(conditional_select, _zero, _one), ecc/mod.rs:58-206 (Point::identity, add_affine ..., conditional_point_select, conditional_point_neg,
conditional_select_identity), ecc/scalar_mul/variable_base.rs:27-95, constraint_system/lookup.rs:18-65 and lookup/lookup_table.rs:
32-204 -- with the loops the reference has: the scalar's accumulators are accumulated, the point is doubled and added bit by bit in
affine coordinates.  Independent of ark_plonk_amd/composer.py, csrc/gadget_layout.hip and csrc/gadget_witness.hip."""
from tests import composer_ref as cr
from tests.composer_ref import te_add


class LookupTable:
    """`LookupTable` (lookup/lookup_table.rs): rows of four integers mod p; the tag -1 is p - 1"""

    def __init__(self, p):
        self.p, self.rows = p, []

    def size(self):
        return len(self.rows)

    def insert_row(self, a, b, c, d):
        self.rows.append([a % self.p, b % self.p, c % self.p, d % self.p])

    def insert_add_row(self, a, b, upper_bound):
        self.insert_row(a, b, (a + b) % upper_bound, 0)

    def insert_mul_row(self, a, b, upper_bound):
        self.insert_row(a, b, (a * b) % upper_bound, 1)

    def insert_xor_row(self, a, b, upper_bound):
        self.insert_row(a, b, (a ^ b) % upper_bound, -1)

    def insert_and_row(self, a, b, upper_bound):
        self.insert_row(a, b, (a & b) % upper_bound, 2)

    def _multi(self, row_fn, lower_bound, n):
        upper_bound = 2 ** n
        for a in range(lower_bound, upper_bound):
            for b in range(lower_bound, upper_bound):
                row_fn(a, b, upper_bound)

    def insert_multi_add(self, lower_bound, n):
        self._multi(self.insert_add_row, lower_bound, n)

    def insert_multi_mul(self, lower_bound, n):
        self._multi(self.insert_mul_row, lower_bound, n)

    def insert_multi_xor(self, lower_bound, n):
        self._multi(self.insert_xor_row, lower_bound, n)

    def insert_multi_and(self, lower_bound, n):
        self._multi(self.insert_and_row, lower_bound, n)

    def lookup(self, a, b, d):
        """the output of the first row with these inputs and tag; KeyError is `Error::ElementNotIndexed`"""
        for row in self.rows:
            if row[0] == a % self.p and row[1] == b % self.p and row[3] == d % self.p:
                return row[2]
        raise KeyError((a, b, d))

    @classmethod
    def add_table(cls, p, lower_bound, n):
        t = cls(p)
        t.insert_multi_add(lower_bound, n)
        return t

    @classmethod
    def xor_table(cls, p, lower_bound, n):
        t = cls(p)
        t.insert_multi_xor(lower_bound, n)
        return t

    @classmethod
    def mul_table(cls, p, lower_bound, n):
        t = cls(p)
        t.insert_multi_mul(lower_bound, n)
        return t

    def columns(self):
        return [[row[w] for row in self.rows] for w in range(4)]


class RefComposerExt(cr.RefComposer):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.lookup_table = LookupTable(self.p)

    def add_witness_to_circuit_description(self, value):
        var = self.add_input(value)
        self.constrain_to_constant(var, value)
        return var

    def is_zero_with_output(self, a):
        a_value = self.values[a]
        y_value = pow(a_value, -1, self.p) if a_value else 1
        b_value = (1 - a_value * y_value) % self.p
        y = self.add_input(y_value)
        b = self.add_input(b_value)
        self.arithmetic_gate(a, b, 0, q_m=1)
        self.arithmetic_gate(a, y, 0, b, q_m=1, q_4=1, q_c=-1)
        return b

    def is_eq_with_output(self, a, b):
        difference = self.arithmetic_gate(a, b, q_l=1, q_r=-1)
        return self.is_zero_with_output(difference)

    def conditional_select(self, bit, choice_a, choice_b):
        bit_times_a = self.arithmetic_gate(bit, choice_a, q_m=1)
        one_min_bit = self.arithmetic_gate(bit, 0, q_l=-1, q_c=1)
        one_min_bit_choice_b = self.arithmetic_gate(one_min_bit, choice_b, q_m=1)
        return self.arithmetic_gate(one_min_bit_choice_b, bit_times_a, q_l=1, q_r=1)

    def conditional_select_zero(self, bit, value):
        return self.arithmetic_gate(bit, value, q_m=1)

    def conditional_select_one(self, bit, value):
        v = self.values
        f_x = self.add_input(1 - v[bit] + v[bit] * v[value])
        self.poly_gate(bit, value, f_x, 1, -1, 0, -1, 1)
        return f_x

    # ---- ecc/mod.rs
    def identity(self):
        return 0, self.add_witness_to_circuit_description(1)

    def add_affine(self, pt):
        return self.add_input(pt[0]), self.add_input(pt[1])

    def add_public_affine(self, pt):
        point = self.add_affine(pt)
        self.constrain_to_constant(point[0], 0, -pt[0])
        self.constrain_to_constant(point[1], 0, -pt[1])
        return point

    def add_affine_to_circuit_description(self, pt):
        return self.add_witness_to_circuit_description(pt[0]), self.add_witness_to_circuit_description(pt[1])

    def assert_equal_public_point(self, point, pt):
        self.constrain_to_constant(point[0], 0, -pt[0])
        self.constrain_to_constant(point[1], 0, -pt[1])

    def assert_equal_point(self, lhs, rhs):
        self.assert_equal(lhs[0], rhs[0])
        self.assert_equal(lhs[1], rhs[1])

    def conditional_point_select(self, point_1, point_0, bit):
        return self.conditional_select(bit, point_1[0], point_0[0]), self.conditional_select(bit, point_1[1], point_0[1])

    def conditional_point_neg(self, bit, point_b):
        x, y = point_b
        x_neg = self.arithmetic_gate(x, 0, q_l=-1)
        return self.conditional_select(bit, x_neg, x), y

    def conditional_select_identity(self, bit, point):
        return self.conditional_select_zero(bit, point[0]), self.conditional_select_one(bit, point[1])

    # ---- ecc/scalar_mul/variable_base.rs
    def scalar_decomposition(self, witness_var, witness_scalar):
        scalar_bits_iter = [(witness_scalar >> i) & 1 for i in range(256)]         # into_repr().to_bits_le(): four 64-bit words
        scalar_bits_var = [self.add_input(bit) for bit in scalar_bits_iter]
        scalar_bits_var = scalar_bits_var[:self.m_bits]
        accumulator_var = 0
        for power, bit in enumerate(scalar_bits_var):
            self.boolean_gate(bit)
            two_pow = pow(2, power, self.p)
            accumulator_var = self.arithmetic_gate(bit, accumulator_var, q_l=two_pow, q_r=1)
        self.assert_equal(accumulator_var, witness_var)
        return scalar_bits_var

    def variable_base_scalar_mul(self, curve_var, point):
        scalar_bits_var = self.scalar_decomposition(curve_var, self.values[curve_var])
        result = self.identity()
        for bit in reversed(scalar_bits_var):
            result = self.point_addition_gate(result, result)
            point_to_add = self.conditional_select_identity(bit, point)
            result = self.point_addition_gate(result, point_to_add)
        return result

    # ---- lookup.rs
    def lookup_gate(self, a, b, c, d=None, pi=None):
        d = 0 if d is None else d
        if pi is not None:
            self.pi[self.n] = pi % self.p
        self._row([a, b, c, d], {"q_lookup": 1})
        self._map4([a, b, c, d])
        return c

    def size(self):
        return 1 << max(max(self.n, self.lookup_table.size(), 1) - 1, 0).bit_length()   # circuit_bound: gates or table rows

    def padded_table(self):
        """(table columns padded to size() with their first row -- lookup/multiset.rs:70-79 --, rows)"""
        n, rows = self.size(), self.lookup_table.size()
        if not rows:
            return [[0]] * 4, 0
        return [col + [col[0]] * (n - rows) for col in self.lookup_table.columns()], rows


# ---- programs of tests/golden/gadget_reference_cases_ext.json: the ops of composer_ref.run_program and the new ones
def run_program(program, api, p, ca, cd, base):
    regs = []
    val = lambda v: cr.resolve(v, p, ca, cd, base)  # noqa: E731
    pt = lambda ix: (regs[ix[0]], regs[ix[1]])  # noqa: E731
    for op in program:
        k = op["op"]
        if k == "input":
            regs.append(api.input(val(op["value"])))
        elif k == "zero":
            regs.append(api.zero())
        elif k == "identity":
            regs.extend(api.identity())
        elif k == "is_zero":
            regs.append(api.is_zero(regs[op["a"]]))
        elif k == "is_eq":
            regs.append(api.is_eq(regs[op["a"]], regs[op["b"]]))
        elif k == "assert_equal":
            api.assert_equal(regs[op["a"]], regs[op["b"]])
        elif k == "select":
            regs.append(api.select(regs[op["bit"]], regs[op["a"]], regs[op["b"]]))
        elif k == "point_select":
            regs.extend(api.point_select(pt(op["p1"]), pt(op["p0"]), regs[op["bit"]]))
        elif k == "point_neg":
            regs.extend(api.point_neg(regs[op["bit"]], pt(op["p"])))
        elif k == "var_base":
            regs.extend(api.var_base(regs[op["scalar"]], pt(op["p"])))
        elif k == "constant":
            api.constant(regs[op["x"]], val(op["value"]), None if op.get("pi") is None else val(op["pi"]))
        elif k == "table":
            api.table(op["kind"], op["lower_bound"], op["n"])
        elif k == "lookup":
            regs.append(api.lookup(regs[op["a"]], regs[op["b"]], regs[op["c"]], None if op.get("d") is None else regs[op["d"]]))
        elif k == "arith":
            regs.append(api.arith(regs[op["a"]], regs[op["b"]], None if op.get("d") is None else regs[op["d"]],
                                  {c: val(op.get(c, "0")) for c in ("q_m", "q_l", "q_r", "q_c", "q_4")},
                                  None if op.get("pi") is None else val(op["pi"])))
        else:
            raise ValueError(k)
    return regs


class RefApiExt(cr.RefApi):
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
