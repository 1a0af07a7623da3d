"""Helper of tests/test_composer*.py (no test): the reference's `StandardComposer` restated sequentially on Python integers, from the
definitions in plonk-core/src/constraint_system/ -- composer.rs:186-350,580-648 (new, poly_gate, constrain_to_constant, assert_equal,
blinding rows), arithmetic.rs:103-168, boolean.rs:25-51, range.rs:27-195, logic.rs:36-345, ecc/curve_addition/variable_base_gate.rs:
24-93, ecc/curve_addition/fixed_base_gate.rs:77-107, ecc/scalar_mul/fixed_base.rs:19-160 -- one call at a time, with the loops the
reference has.  It records rows (four variable ids, twelve selector values), the `add_variable_to_map` calls in call order, the
public inputs and the value of every variable.  Independent of ark_plonk_amd/composer.py, csrc/gadget_layout.hip and
csrc/gadget_witness.hip: no closed form is used here (the accumulators are accumulated, the NAF is `find_wnaf(2)`'s loop, the point accumulator is a running affine sum)."""

SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add", "q_lookup")
L, R, O, F = 0, 1, 2, 3                         # WireData::Left, Right, Output, Fourth

# the embedded curves (a, d): Jubjub over the scalar field of BLS12-381, Baby Jubjub in its published twisted form over BN254's
R_BLS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R_BN = 21888242871839275222246405745257275088548364400416034343698204186575808495617
EMBEDDED = {"bls12_381": (R_BLS, R_BLS - 1, (-10240 * pow(10242, -1, R_BLS)) % R_BLS), "bn254": (R_BN, 168700, 168696)}


class NafTooLong(ValueError):
    """`assert!(wnaf_entries.len() <= num_bits)` (fixed_base.rs:68)"""


def find_wnaf2(e: int) -> list:
    """`BigInteger::find_wnaf(2)` (ark-ff): least significant digit first"""
    res = []
    while e:
        if e & 1:
            z = e % 4
            if z >= 2:
                z -= 4
            e -= z
        else:
            z = 0
        res.append(z)
        e >>= 1
    return res


def te_add(p, ca, cd, p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    t = cd * x1 * x2 * y1 * y2 % p
    return (x1 * y2 + y1 * x2) * pow(1 + t, -1, p) % p, (y1 * y2 - ca * x1 * x2) * pow(1 - t, -1, p) % p


def te_on_curve(p, ca, cd, pt):
    x, y = pt
    return (ca * x * x + y * y - 1 - cd * x * x * y * y) % p == 0


def te_mul(p, ca, cd, k, pt):
    acc = (0, 1)
    while k:
        if k & 1:
            acc = te_add(p, ca, cd, acc, pt)
        pt = te_add(p, ca, cd, pt, pt)
        k >>= 1
    return acc


def _sqrt(p, a):
    """a square root mod p (Tonelli-Shanks), or None"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


def te_point(p, ca, cd, start=2):
    """a point of a x^2 + y^2 = 1 + d x^2 y^2 found by solving the curve equation for x at y = start, start + 1, ...; doubled three
    times so that it lies in the subgroup the cofactor-8 curves' addition law is complete on"""
    y = start
    while True:
        den = (ca - cd * y * y) % p
        if den:
            x = _sqrt(p, (1 - y * y) * pow(den, -1, p))
            if x:
                pt = (x, y)
                for _ in range(3):
                    pt = te_add(p, ca, cd, pt, pt)
                if pt != (0, 1):
                    return pt
        y += 1


class RefComposer:
    def __init__(self, p: int, ca: int = 0, cd: int = 0, blinding=(11, 12, 13, 14, 15, 16, 17, 18)):
        self.p, self.ca, self.cd = p, ca % p, cd % p
        self.m_bits = p.bit_length()
        self.w = [[], [], [], []]
        self.q = {name: [] for name in SELECTORS}
        self.values = []
        self.ins_var, self.ins_wire, self.ins_row = [], [], []
        self.pi = {}
        self.n = 0
        self._multiples = {}
        zero = self.add_input(0)                            # add_witness_to_circuit_description(F::zero())
        self.constrain_to_constant(zero, 0)
        b = [self.add_input(v) for v in blinding]           # add_blinding_factors
        for k in (0, 4):
            self._row(b[k:k + 4], {})
            self._map4(b[k:k + 4])
        self._row([b[4], b[5], 0, 0], {})
        self._map4([b[4], b[5], 0, 0])

    # ---- primitives
    def add_input(self, v: int) -> int:
        self.values.append(v % self.p)
        return len(self.values) - 1

    def _map(self, var, wire, row):
        self.ins_var.append(var)
        self.ins_wire.append(wire)
        self.ins_row.append(row)

    def _row(self, ids, sel):
        """push one row and advance n; the caller maps its cells"""
        for k in range(4):
            self.w[k].append(ids[k])
        for name in SELECTORS:
            self.q[name].append(sel.get(name, 0) % self.p)
        self.n += 1

    def _map4(self, ids):
        for k in range(4):
            self._map(ids[k], k, self.n - 1)

    # ---- arithmetic family
    def poly_gate(self, a, b, c, q_m, q_l, q_r, q_o, q_c, pi=None):
        if pi is not None:
            self.pi[self.n] = pi % self.p
        self._row([a, b, c, 0], {"q_m": q_m, "q_l": q_l, "q_r": q_r, "q_o": q_o, "q_c": q_c, "q_arith": 1})
        self._map4([a, b, c, 0])

    def constrain_to_constant(self, a, constant, pi=None):
        self.poly_gate(a, a, a, 0, 1, 0, 0, -constant, pi)

    def assert_equal(self, a, b):
        self.poly_gate(a, b, 0, 0, 1, -1, 0, 0)

    def boolean_gate(self, a):
        self._row([a, a, a, 0], {"q_m": 1, "q_o": -1, "q_arith": 1})
        self._map4([a, a, a, 0])
        return a

    def arithmetic_gate(self, a, b, c=None, d=None, q_m=0, q_l=0, q_r=0, q_o=-1, q_c=0, q_4=0, pi=None):
        w4 = 0 if d is None else d
        if pi is not None:
            self.pi[self.n] = pi % self.p
        if c is None:
            v = self.values
            c = self.add_input((q_m * v[a] * v[b] + q_l * v[a] + q_r * v[b] + q_c + q_4 * v[w4] + (pi or 0)) * (-q_o))
        self._row([a, b, c, w4], {"q_m": q_m, "q_l": q_l, "q_r": q_r, "q_o": q_o, "q_c": q_c, "q_4": q_4, "q_arith": 1})
        self._map4([a, b, c, w4])
        return c

    # ---- range
    def range_gate(self, witness, num_bits):
        assert num_bits % 2 == 0
        bits = [(self.values[witness] >> i) & 1 for i in range(256)]
        num_gates = num_bits >> 3
        if num_bits % 8:
            num_gates += 1
        num_quads = num_gates * 4
        pad = 1 + (((num_quads << 1) - num_bits) >> 1)
        used_gates = num_gates + 1
        cols = {3: [], 2: [], 1: [], 0: []}

        def add_wire(i, var):
            wire = (F, O, R, L)[i % 4]
            cols[wire].append(var)
            self._map(var, wire, self.n + i // 4)
        accumulators, acc = [], 0
        for i in range(pad):
            add_wire(i, 0)
        for i in range(pad, num_quads + 1):
            bit_index = (num_quads - i) << 1
            acc = (4 * acc + bits[bit_index] + 2 * bits[bit_index + 1]) % self.p
            var = self.add_input(acc)
            accumulators.append(var)
            add_wire(i, var)
        for wire in (L, R, O):                              # pushed without mapping (range.rs:185-187)
            cols[wire].append(0)
        for g in range(used_gates):
            self._row([cols[k][g] for k in range(4)], {"q_range": 1 if g + 1 < used_gates else 0})
        self.assert_equal(accumulators[-1], witness)

    # ---- logic
    def logic_gate(self, a, b, num_bits, is_xor):
        assert num_bits % 2 == 0
        num_quads = num_bits >> 1
        a_bits = [(self.values[a] >> (255 - i)) & 1 for i in range(256)][256 - num_bits:]
        b_bits = [(self.values[b] >> (255 - i)) & 1 for i in range(256)][256 - num_bits:]
        first = self.n
        wl, wr, wo, w4 = [0], [0], [], [0]
        self._map(0, L, first)
        self._map(0, R, first)
        self._map(0, F, first)
        n = first + 1
        la = ra = oa = 0
        for i in range(num_quads):
            lq = (a_bits[2 * i] << 1) + a_bits[2 * i + 1]
            rq = (b_bits[2 * i] << 1) + b_bits[2 * i + 1]
            oq = (lq ^ rq) if is_xor else (lq & rq)
            la, ra, oa = (4 * la + lq) % self.p, (4 * ra + rq) % self.p, (4 * oa + oq) % self.p
            va, vb, vc, v4 = self.add_input(la), self.add_input(ra), self.add_input(lq * rq), self.add_input(oa)
            self._map(va, L, n)
            self._map(vb, R, n)
            self._map(v4, F, n)
            self._map(vc, O, n - 1)
            wl.append(va)
            wr.append(vb)
            wo.append(vc)
            w4.append(v4)
            n += 1
        self._map(0, O, n - 1)
        wo.append(0)
        s = -1 if is_xor else 1
        for g in range(num_quads + 1):
            self._row([wl[g], wr[g], wo[g], w4[g]], {"q_c": s, "q_logic": s} if g < num_quads else {})
        assert self.n == n
        return w4[-1]

    def xor_gate(self, a, b, num_bits):
        return self.logic_gate(a, b, num_bits, True)

    def and_gate(self, a, b, num_bits):
        return self.logic_gate(a, b, num_bits, False)

    # ---- curve
    def point_addition_gate(self, p1, p2):
        (x1, y1), (x2, y2) = p1, p2
        v = self.values
        x3v, y3v = te_add(self.p, self.ca, self.cd, (v[x1], v[y1]), (v[x2], v[y2]))
        x1y2 = self.add_input(v[x1] * v[y2])
        x3, y3 = self.add_input(x3v), self.add_input(y3v)
        self._row([x1, y1, x2, y2], {"q_variable_group_add": 1})
        self._map4([x1, y1, x2, y2])
        self._row([x3, y3, 0, x1y2], {})
        self._map4([x3, y3, 0, x1y2])
        return x3, y3

    def fixed_base_scalar_mul(self, scalar, base):
        p, M = self.p, self.m_bits
        if base not in self._multiples:                     # compute_wnaf_point_multiples, reversed; kept per base point
            mult = [base]
            for _ in range(1, M):
                mult.append(te_add(p, self.ca, self.cd, mult[-1], mult[-1]))
            mult.reverse()
            self._multiples[base] = mult
        mult = self._multiples[base]
        wnaf = find_wnaf2(self.values[scalar])
        if len(wnaf) > M:
            raise NafTooLong(len(wnaf))
        trailing = M - len(wnaf)
        scalar_acc, point_acc, xy_alphas = [0] * (trailing + 1), [(0, 1)] * (trailing + 1), [0] * trailing
        for i, entry in enumerate(reversed(wnaf)):
            index = i + trailing
            if entry == 0:
                s_add, pt = 0, (0, 1)
            elif entry == -1:
                s_add, pt = -1, ((-mult[index][0]) % p, mult[index][1])
            else:
                s_add, pt = 1, mult[index]
            scalar_acc.append((2 * scalar_acc[index] + s_add) % p)
            point_acc.append(te_add(p, self.ca, self.cd, point_acc[index], pt))
            xy_alphas.append(pt[0] * pt[1] % p)
        for i in range(M):
            acc_x, acc_y = self.add_input(point_acc[i][0]), self.add_input(point_acc[i][1])
            bit = self.add_input(scalar_acc[i])
            if i == 0:
                self.constrain_to_constant(acc_x, 0)
                self.constrain_to_constant(acc_y, 1)
                self.constrain_to_constant(bit, 0)
            xb, yb = mult[i]
            xy_alpha = self.add_input(xy_alphas[i])
            self._row([acc_x, acc_y, xy_alpha, bit], {"q_l": xb, "q_r": yb, "q_c": xb * yb, "q_fixed_group_add": 1})
            self._map4([acc_x, acc_y, xy_alpha, bit])
        acc_x, acc_y = self.add_input(point_acc[M][0]), self.add_input(point_acc[M][1])
        last = self.add_input(scalar_acc[M])
        self.arithmetic_gate(acc_x, acc_y, 0, last, q_o=0, q_4=0)
        self.assert_equal(last, scalar)
        return acc_x, acc_y

    # ---- what the device composer is compared with
    def size(self) -> int:
        return 1 << max(self.n - 1, 0).bit_length()

    def ins_pos(self, n=None):
        n = n or self.size()
        return [w * n + r for w, r in zip(self.ins_wire, self.ins_row)]

    def padded(self):
        """(n, wire VALUE columns, selector columns, pi column) padded as preprocess.rs:61-88 pads"""
        n = self.size()
        wires = [[self.values[v] for v in col] + [0] * (n - self.n) for col in self.w]
        sel = {name: col + [0] * (n - self.n) for name, col in self.q.items()}
        pi = [self.pi.get(i, 0) for i in range(n)]
        return n, wires, sel, pi


# ---- programs of tests/golden/gadget_reference_cases.json: the reference's own gadget tests as data
def resolve(v, p, ca, cd, base):
    """a value of the fixture: a decimal string, {"le_bytes": [...]} (`from_le_bytes_mod_order`), or a coordinate of a multiple of the
    base point {"point": value, "of": 1 | 2 (the base or its double), "coord": "x" | "y", "neg": bool}"""
    if isinstance(v, (int, str)):
        return int(v) % p
    if "le_bytes" in v:
        return int.from_bytes(bytes(v["le_bytes"]), "little") % p
    pt = base if v.get("of", 1) == 1 else te_add(p, ca, cd, base, base)
    c = te_mul(p, ca, cd, resolve(v["point"], p, ca, cd, base), pt)[0 if v["coord"] == "x" else 1]
    return (-c) % p if v.get("neg") else c


def run_program(program, api, p, ca, cd, base):
    """Runs one fixture program through `api` (RefApi below, or the device composer's adapter in tests/test_composer_gpu.py): every op
    that yields variables appends them to the register list the later ops index."""
    regs = []
    val = lambda v: resolve(v, p, ca, cd, base)  # noqa: E731
    for op in program:
        k = op["op"]
        if k == "input":
            regs.append(api.input(val(op["value"])))
        elif k == "zero":
            regs.append(api.zero())
        elif k == "range":
            api.range(regs[op["x"]], op["bits"])
        elif k in ("xor", "and"):
            regs.append(api.logic(regs[op["a"]], regs[op["b"]], op["bits"], k == "xor"))
        elif k == "constant":
            api.constant(regs[op["x"]], val(op["value"]), None if op.get("pi") is None else val(op["pi"]))
        elif k == "boolean":
            api.boolean(regs[op["x"]])
        elif k == "fixed_base":
            regs.extend(api.fixed_base(regs[op["scalar"]], base))
        elif k == "point_add":
            regs.extend(api.point_add((regs[op["a"][0]], regs[op["a"][1]]), (regs[op["b"][0]], regs[op["b"][1]])))
        elif k == "arith":
            regs.append(api.arith(regs[op["a"]], regs[op["b"]], None if op.get("d") is None else regs[op["d"]],
                                  {c: val(op.get(c, "0")) for c in ("q_m", "q_l", "q_r", "q_c", "q_4")},
                                  None if op.get("pi") is None else val(op["pi"])))
        else:
            raise ValueError(k)
    return regs


class RefApi:
    def __init__(self, comp: RefComposer):
        self.c = comp

    def input(self, v):
        return self.c.add_input(v)

    def zero(self):
        return 0

    def range(self, x, bits):
        self.c.range_gate(x, bits)

    def logic(self, a, b, bits, is_xor):
        return self.c.logic_gate(a, b, bits, is_xor)

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
