"""`StandardComposer` (plonk-core/src/constraint_system/) for batched gadget calls, on the device: `Composer` produces what
`compile.compile` consumes -- the `CircuitDescription`, built once per circuit (csrc/gadget_layout.hip: zk_gadget_layout_dev) -- and
what `compile.assign` consumes -- the (num_vars, 4) value vector, replayed per proof (csrc/gadget_witness.hip: zk_gadget_witness_dev).

A SEGMENT is B calls of one gadget with the same parameters; by definition it is what the reference's composer holds after that gadget
is called B times in a row, call k with the k-th input variables: rows, new variables in `add_input` order and `add_variable_to_map`
calls in call order, the cells the reference pushes without mapping (range.rs:185-187) and the logic gate's Output(n - 1) after Left(n)
included.  Variable handles are int32 device tensors of shape (B,) (a single id broadcasts), gadgets return the handles the reference
returns, so segments chain without a host copy:

    c = Composer("bls12_381", ctx, coeffs=(a, d))
    x = c.inputs(1024)                          # values arrive at assign time
    c.range_gate(x, 64)
    px, py = c.fixed_base_scalar_mul(x, G)
    desc = c.description()                      # -> compile.compile(desc, ck)
    values = c.assign([x_values])               # -> compile.assign(desc, values)

A new composer starts as `StandardComposer::new()` does (composer.rs:231-235, 580-648): variable 0 constrained to zero on row 0, three
blinding rows over variables 1 .. 8, whose values `assign` takes or draws.

gadget                  rows per call        new variables     insertions
arithmetic family       1                    0 or 1            4
range_gate(bits)        ceil(bits/8) + 2     bits / 2          4 ceil(bits/8) + 5
xor_gate / and_gate     bits / 2 + 1         2 bits            2 bits + 4
point_addition_gate     2                    3                 8
fixed_base_scalar_mul   M + 5                4 M + 3           4 (M + 5)         M = bits of the scalar field (255 / 254)
add_witness_to_circuit_description  1        1                 4
is_zero_with_output     2                    2                 8
is_eq_with_output       3                    3                 12
conditional_select      4                    4                 16
conditional_point_select  8                  8                 32
conditional_point_neg   5                    5                 20
variable_base_scalar_mul  8 M + 2            9 M + 257         32 M + 8
lookup_gate             1                    0 or 1            4                 against `Composer.lookup_table` (a `LookupTable`); with
                                                                                 c=None the output is a new variable: c of the FIRST table row
                                                                                 whose (a, b, d) matches, from the table's map on the device
add_dummy_constraints   2                    4                 8                 the rows of the reference's benchmark circuit (`bench_circuit`)

conditional_select_zero / _one, add_affine, add_public_affine, add_affine_to_circuit_description, assert_equal_point,
assert_equal_public_point and identity are compositions of the rows above with the reference's names."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib
from .compile import CircuitDescription, padded_size
from .context import check_dev_tensor, default_context
from .curves import fr_to_mont, get_curve
from .lookup import ElementNotIndexed
from .prover import SELECTORS

_REC_SHIFT = 30
_TABLE_MAX_BITS = 12                                    # per operand: a block holds at most 2^24 rows
_TABLE_OPS = {"add": 0, "mul": 1, "xor": 2, "and": 3}
_PRELUDE_ROWS, _PRELUDE_VARS = 4, 9


def edwards_add(p: int, ca: int, cd: int, p1, p2):
    """the affine twisted Edwards law a x^2 + y^2 = 1 + d x^2 y^2 on Python integers (ark-ec GroupAffine::add)"""
    (x1, y1), (x2, y2) = p1, p2
    t = cd * x1 * x2 * y1 * y2 % p
    return (x1 * y2 + y1 * x2) * pow(1 + t, -1, p) % p, (y1 * y2 - ca * x1 * x2) * pow(1 - t, -1, p) % p


class LookupTable:
    """`LookupTable` (lookup/lookup_table.rs): rows of four field elements in insertion order.  `insert_row` takes integers;
    the `insert_multi_*(lower_bound, n)` blocks -- every (a, b) with lower_bound <= a, b < 2^n, c = op(a, b) mod 2^n and the tag of the
    operation (add 0, mul 1, xor -1, and 2) -- are recorded and filled on the device when the columns are asked for
    (zk_lookup_table_dev: one lane per row).  `lookup` computes c from (a, b, d) on the device (`LookupTable::lookup`,
    lookup_table.rs:172-180: the first matching row) through a map from (a, b, d) to the smallest row index, built once per table
    (zk_lookup_map_build_dev; 4 bytes per slot, slots = the power of two >= 2 x rows) and kept on the object with the columns until a
    row or block is inserted."""

    def __init__(self):
        self._blocks = []                               # ("rows", [[a, b, c, d], ...]) / ("multi", op, lower_bound, n)
        self._dev = None                                # (curve name, ctx, columns, map, slots): dropped by every insertion

    def insert_row(self, a, b, c, d):
        self._dev = None
        if not self._blocks or self._blocks[-1][0] != "rows":
            self._blocks.append(("rows", []))
        self._blocks[-1][1].append([int(a), int(b), int(c), int(d)])

    # one row of an operation (lookup_table.rs:51-84): c = op(a, b) % upper_bound -- the reference's code takes the remainder by
    # upper_bound itself, whatever its comment says about 2^upper_bound -- and the tag of the operation
    def insert_add_row(self, a, b, upper_bound):
        self.insert_row(a, b, (int(a) + int(b)) % int(upper_bound), 0)

    def insert_mul_row(self, a, b, upper_bound):
        self.insert_row(a, b, (int(a) * int(b)) % int(upper_bound), 1)

    def insert_xor_row(self, a, b, upper_bound):
        self.insert_row(a, b, (int(a) ^ int(b)) % int(upper_bound), -1)

    def insert_and_row(self, a, b, upper_bound):
        self.insert_row(a, b, (int(a) & int(b)) % int(upper_bound), 2)

    def _multi(self, op, lower_bound, n):
        lower_bound, n = int(lower_bound), int(n)
        if not 0 <= n <= _TABLE_MAX_BITS:
            raise ValueError(f"a table block holds operands of at most {_TABLE_MAX_BITS} bits")
        if not 0 <= lower_bound <= 1 << n:
            raise ValueError("lower_bound must lie in 0 .. 2^n")
        if lower_bound < 1 << n:                        # an empty range inserts nothing, as the reference's loops
            self._dev = None
            self._blocks.append(("multi", op, lower_bound, n))

    def insert_multi_add(self, lower_bound, n):
        self._multi("add", lower_bound, n)

    def insert_multi_mul(self, lower_bound, n):
        self._multi("mul", lower_bound, n)

    def insert_multi_xor(self, lower_bound, n):
        self._multi("xor", lower_bound, n)

    def insert_multi_and(self, lower_bound, n):
        self._multi("and", lower_bound, n)

    @classmethod
    def _of(cls, op, lower_bound, n):
        t = cls()
        t._multi(op, lower_bound, n)
        return t

    @classmethod
    def add_table(cls, lower_bound, n):
        return cls._of("add", lower_bound, n)

    @classmethod
    def mul_table(cls, lower_bound, n):
        return cls._of("mul", lower_bound, n)

    @classmethod
    def xor_table(cls, lower_bound, n):
        return cls._of("xor", lower_bound, n)

    def size(self) -> int:
        return sum(len(b[1]) if b[0] == "rows" else ((1 << b[3]) - b[2]) ** 2 for b in self._blocks)

    def columns(self, curve, ctx, device):
        """the four (size, 4) Montgomery columns on the device, blocks concatenated in insertion order"""
        import torch
        curve = get_curve(curve)
        rows = self.size()
        cols = [torch.empty((rows, 4), dtype=torch.int64, device=device) for _ in range(4)]
        at = 0
        ctx.use_torch_stream()
        for b in self._blocks:
            if b[0] == "rows":
                m = len(b[1])
                for w in range(4):
                    cols[w][at:at + m] = torch.from_numpy(fr_to_mont(curve, [r_[w] % curve.r for r_ in b[1]]).view(np.int64)).to(device)
            else:
                _, op, lower, n = b
                m = ((1 << n) - lower) ** 2
                check(lib().zk_lookup_table_dev(ctx.handle, curve.curve_id, _TABLE_OPS[op], lower, n, *[c[at:].data_ptr() for c in cols]),
                      "zk_lookup_table_dev")
            at += m
        return cols

    def device_map(self, curve, ctx, device):
        """(columns, map, slots) of the table on the device: the four columns, the u32 map from (a, b, d) to the first row that holds
        it and its slot count -- built on first use, reused until a row or block is inserted"""
        import torch
        curve = get_curve(curve)
        if self._dev is None or self._dev[0] != curve.name or self._dev[1] is not ctx:
            cols = self.columns(curve, ctx, device)
            rows = self.size()
            slots = int(lib().zk_lookup_map_slots(rows))
            if slots == 0:
                raise ValueError("a lookup table of more than 2^30 rows has no map")
            smap = torch.empty(slots, dtype=torch.int32, device=device)
            ctx.use_torch_stream()
            check(lib().zk_lookup_map_build_dev(ctx.handle, curve.curve_id, cols[0].data_ptr(), cols[1].data_ptr(), cols[3].data_ptr(), rows,
                                                smap.data_ptr(), slots), "zk_lookup_map_build_dev")
            self._dev = (curve.name, ctx, cols, smap, slots)
        return self._dev[2], self._dev[3], self._dev[4]

    def query(self, curve, ctx, n, operands, operand_ids, operand_rows, out, out_ids=None, out_rows=None, pos=None):
        """zk_lookup_map_query_dev over the table's map: -> (return code, misses, first missing query).  operands: three data
        pointers; operand_ids: None or three pointers (0: read directly)"""
        curve = get_curve(curve)
        cols, smap, slots = self.device_map(curve, ctx, out.device)
        misses, first = _lib.c_u64(), _lib.c_u64()
        ids = None if operand_ids is None else (_lib.c_void_p * 3)(*operand_ids)
        ctx.use_torch_stream()
        rc = lib().zk_lookup_map_query_dev(ctx.handle, curve.curve_id, (_lib.c_void_p * 4)(*[c.data_ptr() for c in cols]), self.size(),
                                           smap.data_ptr(), slots, n, (_lib.c_void_p * 3)(*operands), ids, operand_rows, out.data_ptr(),
                                           out_ids, n if out_rows is None else out_rows, None if pos is None else pos.data_ptr(),
                                           ctypes.byref(misses), ctypes.byref(first))
        return rc, misses.value, first.value

    def lookup(self, a, b, d, curve="bls12_381", ctx=None):
        """`LookupTable::lookup` (lookup_table.rs:172-180) for B queries: a, b, d (B, 4) Montgomery device tensors -> the (B, 4) column
        of c, each from the FIRST row whose (a, b, d) matches; raises `lookup.ElementNotIndexed` naming the first query no row holds"""
        import torch
        ctx = ctx or default_context(a.device.index)
        B = check_dev_tensor(a, 4, ctx.device)
        if check_dev_tensor(b, 4, ctx.device) != B or check_dev_tensor(d, 4, ctx.device) != B:
            raise ValueError("a, b and d hold one value per query")
        out = torch.zeros((B, 4), dtype=torch.int64, device=a.device)
        rc, misses, first = self.query(curve, ctx, B, [a.data_ptr(), b.data_ptr(), d.data_ptr()], None, B, out)
        if rc == _lib.ZK_ERR_NOT_INDEXED:
            raise ElementNotIndexed(f"query {first} matches no row of the table ({misses} of {B} queries do not)")
        check(rc, "zk_lookup_map_query_dev")
        return out


class Composer:
    def __init__(self, curve="bls12_381", ctx=None, coeffs=(0, 0), device=None):
        import torch
        self.curve = get_curve(curve)
        self.ctx = ctx or default_context(0 if device is None else device)
        self.device = torch.device("cuda", self.ctx.device)
        self.coeffs = (int(coeffs[0]) % self.curve.r, int(coeffs[1]) % self.curve.r)
        self._coeff_mont = [fr_to_mont(self.curve, [v])[0] for v in self.coeffs]
        self.m_bits = self.curve.r.bit_length()
        self.n_gates, self.num_vars = _PRELUDE_ROWS, _PRELUDE_VARS
        self.public_inputs = {}                         # row -> integer, as given at build time
        self._program = []                              # ("inputs", var0, B) / ("segment", record) in build order
        self._n_inputs = 0
        self.lookup_table = LookupTable()               # `StandardComposer::lookup_table`: assigned by the circuit
        # StandardComposer::new(): constrain_to_constant(zero_var, 0) and add_blinding_factors
        one = fr_to_mont(self.curve, [1])[0].view(np.int64)
        sel = {name: torch.zeros((_PRELUDE_ROWS, 4), dtype=torch.int64) for name in SELECTORS}
        sel["q_l"][0] = torch.from_numpy(one)
        sel["q_arith"][0] = torch.from_numpy(one)
        wires = [[0, 1, 5, 5], [0, 2, 6, 6], [0, 3, 7, 0], [0, 4, 8, 0]]
        self._ids = [[torch.tensor(w, dtype=torch.int32, device=self.device)] for w in wires]
        self._sel = {name: [sel[name].to(self.device)] for name in SELECTORS}
        self._ins_var = [torch.tensor([wires[w][r] for r in range(_PRELUDE_ROWS) for w in range(4)], dtype=torch.int32, device=self.device)]
        self._ins_rec = [torch.tensor([(w << _REC_SHIFT) | r for r in range(_PRELUDE_ROWS) for w in range(4)], dtype=torch.int64)
                         .to(torch.int32).to(self.device)]

    # ------------------------------------------------------------------------------------------------------------ handles
    def zero_var(self) -> int:
        return 0

    def _own(self, t):
        t._composer = self
        return t

    def inputs(self, B: int):
        """B fresh variables whose values arrive at assign time (`add_input`), as a handle"""
        import torch
        B = int(B)
        if B < 1:
            raise ValueError("at least one variable expected")
        v0 = self.num_vars
        self.num_vars += B
        self._program.append(("inputs", v0, B))
        self._n_inputs += 1
        return self._own(torch.arange(v0, v0 + B, dtype=torch.int32, device=self.device))

    def _batch(self, handles, B=None) -> int:
        sizes = {int(h.numel()) for h in handles if hasattr(h, "numel") and int(h.numel()) != 1}
        if B is not None:
            sizes.add(int(B))
        if len(sizes) > 1:
            raise ValueError(f"handles of different batch sizes: {sorted(sizes)}")
        B = sizes.pop() if sizes else 1
        if B < 1:
            raise ValueError("a segment holds at least one call")
        return B

    def _handle(self, h, B: int):
        import torch
        if hasattr(h, "numel"):
            if getattr(h, "_composer", self) is not self:
                raise ValueError("a variable handle of another composer")
            if h.dtype != torch.int32 or h.device != self.device or h.dim() > 1:
                raise ValueError("a variable handle is an int32 device tensor of shape (B,)")
            h = h.reshape(-1)
            return h.contiguous() if h.numel() == B else h.expand(B).contiguous()
        h = int(h)
        if not 0 <= h < self.num_vars:
            raise ValueError(f"variable {h} is not defined")
        return torch.full((B,), h, dtype=torch.int32, device=self.device)

    def _column(self, vals):
        import torch
        return torch.from_numpy(fr_to_mont(self.curve, vals).view(np.int64)).to(self.device)

    # ------------------------------------------------------------------------------------------------------------ segments
    def _shape(self, kind, num_bits=0, flags=0, B=1):
        r, v, i, w = _lib.c_u32(), _lib.c_u32(), _lib.c_u32(), _lib.c_size_t()
        check(lib().zk_gadget_shape(kind, self.curve.curve_id, num_bits, flags, B, ctypes.byref(r), ctypes.byref(v), ctypes.byref(i),
                                    ctypes.byref(w)), "zk_gadget_shape")
        return r.value, v.value, i.value, w.value

    def _args(self, seg) -> _lib.GadgetArgs:
        a = _lib.GadgetArgs()
        a.kind, a.num_bits, a.flags, a.calls, a.row0, a.var0 = seg["kind"], seg["num_bits"], seg["flags"], seg["B"], seg["row0"], seg["var0"]
        for w, h in enumerate(seg["inputs"]):
            if w < 4:
                a.inputs[w] = None if h is None else h.data_ptr()
            else:
                a.inputs_ext[w - 4] = None if h is None else h.data_ptr()
        for j, cf in enumerate(seg["coeff"]):
            if hasattr(cf, "data_ptr"):
                a.coeff[j] = cf.data_ptr()
            else:
                for t, limb in enumerate(fr_to_mont(self.curve, [cf])[0]):
                    a.coeff_const[4 * j + t] = int(limb)
        for t in range(4):
            a.coeff_a[t], a.coeff_d[t] = int(self._coeff_mont[0][t]), int(self._coeff_mont[1][t])
        if seg["table"] is not None:
            a.table = seg["table"].data_ptr()
        return a

    def _lut_args(self, a):
        """the lookup table of a LOOKUP_OUT witness: columns, map and slot count of `self.lookup_table`, built or reused"""
        cols, smap, slots = self.lookup_table.device_map(self.curve, self.ctx, self.device)
        for w in range(4):
            a.lut[w] = cols[w].data_ptr()
        a.lut_rows, a.lut_map, a.lut_slots = self.lookup_table.size(), smap.data_ptr(), slots
        return cols, smap

    def _segment(self, kind, B, inputs, num_bits=0, flags=0, coeff=(0,) * 6, pi=None, table=None) -> dict:
        import torch
        R, V, I, _ = self._shape(kind, num_bits, flags, B)
        cf = []
        for c_ in coeff:
            if hasattr(c_, "data_ptr"):
                if check_dev_tensor(c_, 4, self.ctx.device) != B:
                    raise ValueError(f"a coefficient column holds one Montgomery row per call ({B})")
            elif not isinstance(c_, (int, np.integer)):
                c_ = self._column(list(c_))
                if int(c_.shape[0]) != B:
                    raise ValueError(f"a coefficient column holds one value per call ({B})")
            cf.append(c_)
        if pi is not None:
            pi = [int(v) % self.curve.r for v in (pi if hasattr(pi, "__len__") else [pi] * B)]
            if len(pi) != B:
                raise ValueError(f"one public input per call ({B}) expected")
        seg = {"kind": kind, "num_bits": num_bits, "flags": flags, "B": B, "row0": self.n_gates, "var0": self.num_vars, "R": R, "V": V,
               "inputs": list(inputs) + [None] * max(0, 4 - len(inputs)), "coeff": cf, "pi": pi, "table": table}
        N = B * R
        ids = torch.empty((4, N), dtype=torch.int32, device=self.device)
        sel = [torch.empty((N, 4), dtype=torch.int64, device=self.device) for _ in SELECTORS]
        ins_var = torch.empty(B * I, dtype=torch.int32, device=self.device)
        ins_rec = torch.empty(B * I, dtype=torch.int32, device=self.device)
        a = self._args(seg)
        self.ctx.use_torch_stream()
        check(lib().zk_gadget_layout_dev(self.ctx.handle, self.curve.curve_id, ctypes.addressof(a), ids.data_ptr(),
                                         (ctypes.c_void_p * 12)(*[t.data_ptr() for t in sel]), ins_var.data_ptr(), ins_rec.data_ptr()),
              "zk_gadget_layout_dev")
        for w in range(4):
            self._ids[w].append(ids[w])
        for name, t in zip(SELECTORS, sel):
            self._sel[name].append(t)
        self._ins_var.append(ins_var)
        self._ins_rec.append(ins_rec)
        if pi is not None:
            self.public_inputs.update({seg["row0"] + k: v for k, v in enumerate(pi)})
        self.n_gates += N
        self.num_vars += B * V
        self._program.append(("segment", seg))
        return seg

    def _gadget(self, kind, handles, B=None, **kw):
        """the segment of one gadget over its input handles (None: an input the call does not have), batched to a common B"""
        B = self._batch([h for h in handles if h is not None], B)
        return self._segment(kind, B, [None if h is None else self._handle(h, B) for h in handles], **kw)

    def _new_vars(self, seg, offset: int):
        """the handle of new variable `offset` of every call of the segment"""
        import torch
        return self._own(seg["var0"] + offset + seg["V"] * torch.arange(seg["B"], dtype=torch.int32, device=self.device))

    # ------------------------------------------------------------------------------------------------------------ gadgets
    def arithmetic_gate(self, a, b, c=None, d=None, q_m=0, q_l=0, q_r=0, q_o=-1, q_c=0, q_4=0, pi=None, B=None):
        """`arithmetic_gate` (arithmetic.rs:103-168): one row q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c + pi = 0 per call.  A
        coefficient is an integer (constant for the segment), a sequence of B integers or a (B, 4) Montgomery device column; pi an
        integer or B integers (host values given at build time, replaceable per row at assign time).  With c=None the output is a new
        variable whose value is (q_m a b + q_l a + q_r b + q_c + q_4 d + pi) (-q_o), exactly as arithmetic.rs:144-155 writes it: it
        MULTIPLIES by -q_o, it does not divide -- the row is satisfied for q_o = -1 (the default) and q_o = 1 only.  Returns c."""
        seg = self._gadget(_lib.ZK_GADGET_POLY, [a, b, c, 0 if d is None else d], B, flags=_lib.ZK_GADGET_COMPUTE_OUT if c is None else 0,
                           coeff=(q_m, q_l, q_r, q_o, q_4, q_c), pi=pi)
        return self._new_vars(seg, 0) if c is None else self._own(seg["inputs"][2])

    def poly_gate(self, a, b, c, q_m=0, q_l=0, q_r=0, q_o=0, q_c=0, pi=None, B=None):
        """`poly_gate` (composer.rs:269-312)"""
        self.arithmetic_gate(a, b, c, None, q_m, q_l, q_r, q_o, q_c, 0, pi, B)
        return a, b, c

    def constrain_to_constant(self, a, constant, pi=None):
        """`constrain_to_constant` (composer.rs:318-335): a - constant + pi = 0; constant: an integer or one per call"""
        r = self.curve.r
        neg = (-int(constant)) % r if isinstance(constant, (int, np.integer)) else [(-int(v)) % r for v in constant]
        B = None if isinstance(neg, int) else len(neg)
        self.arithmetic_gate(a, a, a, None, 0, 1, 0, 0, neg, 0, pi, B)

    def assert_equal(self, a, b):
        """`assert_equal` (composer.rs:339-350)"""
        self.arithmetic_gate(a, b, 0, None, 0, 1, -1, 0, 0, 0)

    def boolean_gate(self, a):
        """`boolean_gate` (boolean.rs:25-51): a a - a = 0"""
        return self.arithmetic_gate(a, a, a, None, 1, 0, 0, -1, 0, 0)

    @staticmethod
    def _check_bits(num_bits) -> int:
        num_bits = int(num_bits)
        if num_bits % 2 or not 2 <= num_bits <= 256:
            raise ValueError("num_bits must be even and in 2 .. 256")
        return num_bits

    def range_gate(self, x, num_bits: int):
        """`range_gate` (range.rs:27-195); the closing assert_equal row is satisfied iff the value is below 2^num_bits"""
        self._gadget(_lib.ZK_GADGET_RANGE, [x], num_bits=self._check_bits(num_bits))

    def _logic(self, a, b, num_bits, flags):
        num_bits = self._check_bits(num_bits)
        seg = self._gadget(_lib.ZK_GADGET_LOGIC, [a, b], num_bits=num_bits, flags=flags)
        return self._new_vars(seg, 4 * (num_bits // 2 - 1) + 3)

    def xor_gate(self, a, b, num_bits: int):
        """`xor_gate` (logic.rs:322-329): the variable of the last fourth wire.  As in the reference nothing ties the last input
        prefixes back to a and b."""
        return self._logic(a, b, num_bits, _lib.ZK_GADGET_XOR)

    def and_gate(self, a, b, num_bits: int):
        """`and_gate` (logic.rs:338-345)"""
        return self._logic(a, b, num_bits, 0)

    def point_addition_gate(self, p1, p2):
        """`point_addition_gate` (variable_base_gate.rs:24-93): points are (x, y) pairs of handles; returns (x3, y3)"""
        seg = self._gadget(_lib.ZK_GADGET_CURVE_ADD, [p1[0], p1[1], p2[0], p2[1]])
        return self._new_vars(seg, 1), self._new_vars(seg, 2)

    def fixed_base_table(self, base):
        """(3 M, 4) Montgomery rows: x, y, x y of 2^(M-1-i) G for row i (fixed_base.rs:19-36, 58-60), on Python integers"""
        p, (ca, cd), M = self.curve.r, self.coeffs, self.m_bits
        pts = [(int(base[0]) % p, int(base[1]) % p)]
        for _ in range(M - 1):
            pts.append(edwards_add(p, ca, cd, pts[-1], pts[-1]))
        flat = []
        for x, y in reversed(pts):
            flat += [x, y, x * y % p]
        return self._column(flat)

    def fixed_base_scalar_mul(self, scalar, base):
        """`fixed_base_scalar_mul` (fixed_base.rs:51-160): base an affine point (x, y) of the embedded curve as integers; returns the
        handles (acc_x, acc_y) of the product.  A scalar whose width-2 NAF has more than M digits is refused at assign time."""
        seg = self._gadget(_lib.ZK_GADGET_FIXED_BASE, [scalar], table=self.fixed_base_table(base))
        return self._new_vars(seg, 4 * self.m_bits), self._new_vars(seg, 4 * self.m_bits + 1)

    def add_witness_to_circuit_description(self, value, B=None):
        """`add_witness_to_circuit_description` (composer.rs:192-196): a new variable fixed to `value` -- an integer (B calls of it) or
        one integer per call -- by a row of the circuit description.  Returns the variable."""
        r = self.curve.r
        neg = (-int(value)) % r if isinstance(value, (int, np.integer)) else [(-int(v)) % r for v in value]
        B = (1 if B is None else int(B)) if isinstance(neg, int) else len(neg)
        seg = self._gadget(_lib.ZK_GADGET_CONST_WITNESS, [], B, coeff=(0, 0, 0, 0, 0, neg))
        return self._new_vars(seg, 0)

    def is_zero_with_output(self, a):
        """`is_zero_with_output` (composer.rs:355-383): the variable b = (a == 0), with y = 1 / a (1 when a = 0) beside it"""
        return self._new_vars(self._gadget(_lib.ZK_GADGET_IS_ZERO, [a]), 1)

    def is_eq_with_output(self, a, b):
        """`is_eq_with_output` (composer.rs:387-392): is_zero of the difference a - b"""
        return self._new_vars(self._gadget(_lib.ZK_GADGET_IS_EQ, [a, b]), 2)

    def conditional_select(self, bit, choice_a, choice_b):
        """`conditional_select` (composer.rs:404-433): bit == 1 => choice_a, bit == 0 => choice_b; four rows"""
        return self._new_vars(self._gadget(_lib.ZK_GADGET_SELECT, [bit, choice_a, choice_b]), 3)

    def conditional_point_select(self, point_1, point_0, bit):
        """`conditional_point_select` (ecc/mod.rs:145-155): bit == 1 => point_1, bit == 0 => point_0"""
        seg = self._gadget(_lib.ZK_GADGET_POINT_SELECT, [bit, point_1[0], point_0[0], point_1[1], point_0[1]])
        return self._new_vars(seg, 3), self._new_vars(seg, 7)

    def conditional_point_neg(self, bit, point):
        """`conditional_point_neg` (ecc/mod.rs:165-182): bit == 1 => (-x, y), bit == 0 => (x, y)"""
        seg = self._gadget(_lib.ZK_GADGET_POINT_NEG, [bit, point[0]])
        return self._new_vars(seg, 4), point[1]

    def variable_base_scalar_mul(self, scalar, point):
        """`variable_base_scalar_mul` (ecc/scalar_mul/variable_base.rs:27-95): scalar a variable, point a pair of variables; returns
        the handles of the product.  8 M + 2 rows per call; a zero denominator of the group law on the way is refused at assign time."""
        seg = self._gadget(_lib.ZK_GADGET_VAR_BASE, [scalar, point[0], point[1]])
        return self._new_vars(seg, seg["V"] - 2), self._new_vars(seg, seg["V"] - 1)

    def lookup_gate(self, a, b, c=None, d=None, pi=None, B=None):
        """`lookup_gate` (lookup.rs:18-65): the row (a, b, c, d) must be a row of `self.lookup_table`; d=None is the zero variable.
        With c=None the output is a new variable whose value `assign` takes from the table on the device -- c of the first row whose
        (a, b, d) matches, `c = add_input(table.lookup(a, b, d)?)` in the reference's terms; a key in no row is refused at assign
        time (`lookup.ElementNotIndexed`).  Returns c."""
        if c is None:
            return self._new_vars(self._gadget(_lib.ZK_GADGET_LOOKUP_OUT, [None] * 4 + [a, b, d], B, pi=pi), 0)
        seg = self._gadget(_lib.ZK_GADGET_LOOKUP, [a, b, c, d], B, pi=pi)
        return self._own(seg["inputs"][2])

    def add_dummy_constraints(self, B=1):
        """`add_dummy_constraints` (composer.rs:493-548), B calls: four new variables 6, 1, 7, -20 and two rows that satisfy the
        arithmetic identity and are rows of the dummy table, each with q_arith = q_lookup = 1"""
        self._gadget(_lib.ZK_GADGET_DUMMY, [], B)

    def add_dummy_lookup_table(self):
        """`add_dummy_lookup_table` (composer.rs:553-574): three rows, the first two the rows of `add_dummy_constraints`"""
        for row in ((6, 7, -20, 1), (-20, 6, 7, 0), (3, 1, 4, 9)):
            self.lookup_table.insert_row(*row)

    def circuit_bound(self) -> int:
        """`circuit_bound` (composer.rs:131-138)"""
        return padded_size(self.n_gates, self.lookup_table.size())

    # ---- compositions of the rows above, with the reference's names
    def conditional_select_zero(self, bit, value):
        """`conditional_select_zero` (composer.rs:444-453): bit * value"""
        return self.arithmetic_gate(bit, value, q_m=1)

    def conditional_select_one(self, bit, value):
        """`conditional_select_one` (composer.rs:464-488): 1 - bit + bit * value"""
        return self.arithmetic_gate(bit, value, q_m=1, q_l=-1, q_c=1)

    def identity(self, B=1):
        """`Point::identity` (ecc/mod.rs:58-62): (zero_var, a new variable fixed to one)"""
        return 0, self.add_witness_to_circuit_description(1, B)

    # A call of the point helpers below handles x, then y; B calls in a row therefore interleave the coordinates -- variables
    # x_0 y_0 x_1 y_1 ... and rows likewise -- which is one segment of 2 B calls over interleaved handles.
    def _pair(self, hx, hy, B=None):
        import torch
        B = self._batch([hx, hy], B)
        return self._own(torch.stack([self._handle(hx, B), self._handle(hy, B)], dim=1).reshape(-1)), B

    @staticmethod
    def _pair_ints(vx, vy, B, sign=1):
        one = lambda v: [sign * int(v)] * B if isinstance(v, (int, np.integer)) else [sign * int(t) for t in v]  # noqa: E731
        xs, ys = one(vx), one(vy)
        if len(xs) != B or len(ys) != B:
            raise ValueError(f"one point per call ({B}) expected")
        return [c_ for q in zip(xs, ys) for c_ in q]

    def add_affine(self, B=1):
        """`add_affine` (ecc/mod.rs:82-84): ONE `inputs(2 B)` whose (2 B, 4) values arrive at assign time interleaved, x_0 y_0 x_1 y_1
        ...; returns the handles (x, y)"""
        h = self.inputs(2 * int(B))
        return self._own(h[0::2].contiguous()), self._own(h[1::2].contiguous())

    def add_public_affine(self, point, B=1):
        """`add_public_affine` (ecc/mod.rs:88-93): `add_affine`, both coordinates bound to the public point (integers, or B each)"""
        pt = self.add_affine(B)
        self.assert_equal_public_point(pt, point)
        return pt

    def add_affine_to_circuit_description(self, point, B=1):
        """`add_affine_to_circuit_description` (ecc/mod.rs:97-106): coordinates are integers (B calls of them) or B each"""
        B = B if isinstance(point[0], (int, np.integer)) else len(point[0])
        h = self.add_witness_to_circuit_description(self._pair_ints(point[0], point[1], B))
        return self._own(h[0::2].contiguous()), self._own(h[1::2].contiguous())

    def assert_equal_point(self, lhs, rhs):
        """`assert_equal_point` (ecc/mod.rs:127-130)"""
        B = self._batch([lhs[0], lhs[1], rhs[0], rhs[1]])
        self.assert_equal(self._pair(lhs[0], lhs[1], B)[0], self._pair(rhs[0], rhs[1], B)[0])

    def assert_equal_public_point(self, point, public_point):
        """`assert_equal_public_point` (ecc/mod.rs:110-117): coordinates are integers or one per call"""
        h, B = self._pair(point[0], point[1])
        self.constrain_to_constant(h, 0, pi=self._pair_ints(public_point[0], public_point[1], B, -1))

    # ------------------------------------------------------------------------------------------------------------ results
    def _first_miss(self, seg, values) -> str:
        """the message of a LOOKUP_OUT segment whose witness found a key in no row: the same query again, for the first failing call"""
        ins = seg["inputs"][4:7]
        zero = self._handle(0, seg["B"])
        ids = [(zero if h is None else h).data_ptr() for h in ins]
        out = values[seg["var0"]:seg["var0"] + seg["B"]]
        _, misses, first = self.lookup_table.query(self.curve, self.ctx, seg["B"], [values.data_ptr()] * 3, ids, seg["var0"], out)
        return (f"lookup_gate segment at row {seg['row0']}: call {first} (row {seg['row0'] + first}) looks up a key (a, b, d) that is in no "
                f"row of the lookup table ({misses} of {seg['B']} calls do)")

    def _pi_limbs(self, overrides=None) -> dict:
        pi = dict(self.public_inputs)
        for row, v in (overrides or {}).items():
            if row not in pi:
                raise ValueError(f"row {row} holds no public input")
            pi[row] = int(v) % self.curve.r
        return pi

    def description(self) -> CircuitDescription:
        import torch
        lookup_kinds = (_lib.ZK_GADGET_LOOKUP, _lib.ZK_GADGET_LOOKUP_OUT, _lib.ZK_GADGET_DUMMY)
        has_lookup = any(what == "segment" and rest[0]["kind"] in lookup_kinds for what, *rest in self._program)
        if has_lookup and self.lookup_table.size() == 0:
            raise ValueError("the circuit has lookup gates but `lookup_table` is empty")
        table_cols = self.lookup_table.columns(self.curve, self.ctx, self.device) if self.lookup_table.size() else []
        n = padded_size(self.n_gates, self.lookup_table.size())
        rec = torch.cat(self._ins_rec).to(torch.int64) & 0xFFFFFFFF     # the kernels write the records as unsigned words
        ins_pos = ((rec >> _REC_SHIFT) * n + (rec & ((1 << _REC_SHIFT) - 1))).to(torch.int32).contiguous()
        rows = sorted(self.public_inputs)
        limbs = fr_to_mont(self.curve, [self.public_inputs[r_] for r_ in rows])
        return CircuitDescription(self.n_gates, {name: torch.cat(self._sel[name]).contiguous() for name in SELECTORS},
                                  [torch.cat(w).contiguous() for w in self._ids], self.num_vars, torch.cat(self._ins_var).contiguous(), ins_pos,
                                  table_cols, {r_: limbs[i] for i, r_ in enumerate(rows)}, self.curve.name)

    def assign(self, inputs, blinding=None, public_inputs=None):
        """The (num_vars, 4) values `compile.assign` takes: the witness kernels replayed segment by segment in build order.
        inputs: one (B, 4) Montgomery device tensor per `inputs()` call, in call order; blinding: the (8, 4) values of variables 1 .. 8,
        a `torch.Generator` that draws them, or None (a fresh generator); public_inputs: {row: integer} replacing build-time values.
        With public inputs in the circuit returns (values, {row: 4 Montgomery limbs}) -- the dict `prove` takes."""
        import torch
        if hasattr(inputs, "data_ptr"):
            inputs = [inputs]
        if len(inputs) != self._n_inputs:
            raise ValueError(f"{self._n_inputs} input tensors expected")
        pi = self._pi_limbs(public_inputs)
        values = torch.zeros((self.num_vars, 4), dtype=torch.int64, device=self.device)
        if blinding is None or isinstance(blinding, torch.Generator):
            gen = blinding if blinding is not None else torch.Generator(device=self.device)
            if blinding is None:
                gen.seed()
            blinding = torch.randint(0, 1 << 62, (8, 4), dtype=torch.int64, device=gen.device, generator=gen).to(self.device)
            blinding[:, 3] &= (1 << 60) - 1             # below 2^252: a reduced element of either scalar field
        if check_dev_tensor(blinding, 4, self.ctx.device) != 8:
            raise ValueError("8 blinding values expected")
        values[1:_PRELUDE_VARS] = blinding
        it = iter(inputs)
        self.ctx.use_torch_stream()
        for what, *rest in self._program:
            if what == "inputs":
                v0, B = rest
                t = next(it)
                if check_dev_tensor(t, 4, self.ctx.device) != B:
                    raise ValueError(f"{B} input values expected")
                values[v0:v0 + B] = t
                continue
            seg = rest[0]
            if seg["V"] == 0:
                continue
            a = self._args(seg)
            keep = None
            if seg["pi"] is not None:
                keep = self._column([pi[seg["row0"] + k] for k in range(seg["B"])])
                a.pi = keep.data_ptr()
            lut = self._lut_args(a) if seg["kind"] == _lib.ZK_GADGET_LOOKUP_OUT else None       # kept alive over the call
            rc = lib().zk_gadget_witness_dev(self.ctx.handle, self.curve.curve_id, ctypes.addressof(a), values.data_ptr(), self.num_vars)
            if rc == _lib.ZK_ERR_NOT_INDEXED and lut is not None:
                raise ElementNotIndexed(self._first_miss(seg, values))
            check(rc, "zk_gadget_witness_dev")
        if not pi:
            return values
        rows = sorted(pi)
        limbs = fr_to_mont(self.curve, [pi[r_] for r_ in rows])
        return values, {r_: limbs[i] for i, r_ in enumerate(rows)}


def bench_circuit(log_n: int, curve="bls12_381", ctx=None, coeffs=(0, 0)) -> Composer:
    """`BenchCircuit::gadget` (benches/plonk.rs:45-68), the one circuit the reference benchmarks: `add_dummy_lookup_table`, then
    `add_dummy_constraints` while `circuit_bound() < 2^log_n - 1` -- 2^(log_n - 1) + 2 gates for log_n >= 3 (the composer's first four
    rows included; 4 gates below that), padded to 2^log_n.  The calls are ONE segment: the loop's trip count is known in advance,
    because every call adds two rows and the table stays at three."""
    c = Composer(curve, ctx, coeffs=coeffs)
    c.add_dummy_lookup_table()
    size, n, rows = 1 << int(log_n), c.n_gates, c.lookup_table.size()
    calls = max(0, (size // 2 + 2 - n) // 2)            # the first gate count above size / 2 pads to size
    assert padded_size(n + 2 * calls, rows) >= size - 1 and (calls == 0 or padded_size(n + 2 * (calls - 1), rows) < size - 1)
    if calls:
        c.add_dummy_constraints(calls)
    return c
