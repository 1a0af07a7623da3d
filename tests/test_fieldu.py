"""CPU check of the unsaturated fields (29-bit limbs for the scalar fields: fieldu.cuh; signed 30-bit limbs for the base
fields: fields.cuh) and of the XYZZ group law (ecu.cuh) -- over the signed-limb field as the HIP kernels use it and over the saturated
field (field.cuh) as the host code does -- compiled for the host and compared with big-int arithmetic; and of two device-only pieces: the load conversion of the quotient kernel and the circuit check (to_rp,
zbound.cuh) on boundary and random stored words, and the hash of the device key maps (fr_io.cuh) against its Python restatement
(tests/edge_values.py), on which the crafted collisions of the GPU suite rest.  And of the call sites of the group law (ecu.cuh, ecq.cuh):
instantiated over a field that checks the preconditions of fields.cuh at every call (tests/native/fb_field.h), the law must stay inside
the contract on every branch, from inputs anywhere in its class invariant.  And of the scalar field's lazily normalised operators
(fieldu.cuh: mul_fenced, add_raw, sub_raw3/8/16, sweep, the constants ZB3/8/16) and the numeric rules of zbound.cuh, on raw 29-bit
limb patterns at the ends of the contracts their comments state."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import bigint_oracle as bo
from tests import edge_values as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fu_check.cpp")
SO = os.path.join(ROOT, "tests", "native", "libfu_check.so")


@pytest.fixture(scope="module")
def fu():
    deps = [SRC] + [os.path.join(ROOT, "tests", "native", f) for f in ("fb_field.h", "fb_laws.h")]
    deps += [os.path.join(ROOT, "ark_plonk_amd", "csrc", f) for f in ("field_common.cuh", "fieldu.cuh", "fields.cuh", "ecu.cuh", "ecq.cuh", "curve_params.h", "zk_common.h", "field.cuh", "fr_io.cuh", "domain.cuh", "zbound.cuh")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-x", "c++", SRC, "-o", SO])
    L = ctypes.CDLL(SO)
    L.fb_rule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.fb_op_name.argtypes = [ctypes.c_int]
    L.fb_op_name.restype = ctypes.c_char_p
    L.fb_log_take.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.fb_closure.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    L.fu_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.fu_xyzz_chain.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.fs_raw_op.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.fu_raw_op.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.fu_to_rp.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.fu_to_rp.restype = None
    L.fu_pack_rp.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_uint64]
    L.fu_pack_rp.restype = None
    L.fu_domain_log_ok.argtypes = [ctypes.c_int, ctypes.c_uint32]
    L.fu_domain_root.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    L.fu_domain_root.restype = None
    L.fu_id_consts.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    L.fu_id_consts.restype = None
    L.fu_gate_consts.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 3
    L.fu_gate_consts.restype = None
    L.fu_el_mix.argtypes = [ctypes.c_uint64, ctypes.c_void_p]
    L.fu_el_mix.restype = ctypes.c_uint64
    L.fu_key_hash.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.fu_key_hash.restype = ctypes.c_uint32
    return L


FIELDS = {0: (bo.BLS12_381.q, 12), 1: (bo.BLS12_381.r, 8), 2: (bo.BN254.q, 8), 3: (bo.BN254.r, 8)}   # 0, 2: signed limbs


def words(v, n):
    return np.frombuffer(int(v).to_bytes(4 * n, "little"), dtype="<u4").copy()


def unwords(a):
    return int.from_bytes(np.ascontiguousarray(a, dtype="<u4").tobytes(), "little")


@pytest.mark.parametrize("field", [0, 1, 2, 3])
def test_field_ops(field, fu):
    p, n = FIELDS[field]
    R = 1 << (32 * n)
    Rinv = pow(R, -1, p)
    rng = np.random.default_rng(field)
    specials = [0, 1, p - 1, p - 2, 2, (1 << 29) - 1, 1 << 29, (p - 1) // 2]
    # limb patterns at the edges of the digit ranges: every 29- / 30-bit digit all ones, 2^29 or 2^29 - 1 in every 30-bit digit
    specials += [v % p for v in ((1 << (32 * n)) - 1, sum(1 << (30 * i + 29) for i in range(13)), sum(((1 << 29) - 1) << (30 * i) for i in range(13)),
                                 sum(((1 << 29) + 1) << (30 * i) for i in range(13)), (p + 1) // 2, (1 << (p.bit_length() - 1)) - 1)]
    if field in (0, 2):
        # the edge targets of the curve points (tests/edge_values.py) as field elements: the values whose stored word t * R^-1, and
        # whose internal form t * R'^-1 (R' = 2^(30 NL): strict limbs at the ends of their range), is the target
        cv = bo.CURVES[field // 2]
        ts = [t for t, _ in ev.fq_targets(p)]
        specials += [t * Rinv % p for t in ts]
        specials += [t * pow(ev.form_factor(cv, "internal"), -1, p) % p for t in ts + [ev.limbs_value(l) for l, _ in ev.internal_patterns(cv)]]
    vals = specials + [int.from_bytes(rng.bytes(4 * n + 8), "little") % p for _ in range(40)]
    out = np.zeros(n, dtype="<u4")
    for i, x in enumerate(vals):
        y = vals[(i * 7 + 3) % len(vals)]
        xm, ym = x * R % p, y * R % p   # arkworks Montgomery form in, same form out
        exp = {
            0: x * y % p, 1: (x + y) % p, 2: (x - y) % p, 3: (x - y) % p, 4: x * x % p,
            5: pow(x, -1, p) if x else 0, 6: (-x) % p, 7: 2 * x % p,
            8: pow(((x - y) * (2 * x + y) - x * y) % p, 2, p),
        }
        if field in (0, 2):   # dot2 and the one-step X3 are the base fields'
            exp[9] = (x * y + (x - y) * (2 * x + y)) % p
            exp[10] = (x * y - y * y) % p
            exp[11] = (x * y - 2 * x * x - y * y) % p
        wa, wb = words(xm, n), words(ym, n)   # keep the buffers alive across the call
        for op, e in exp.items():
            fu.fu_op(field, op, wa.ctypes.data, wb.ctypes.data, out.ctypes.data)
            got = unwords(out) * Rinv % p
            assert unwords(out) < p, (field, op)
            assert got == e, (field, op, hex(x), hex(y))


@pytest.mark.parametrize("cid", [0, 1])
def test_xyzz_chain_matches_affine_group_law(cid, fu):
    cv = bo.CURVES[cid]
    W = 2 * cv.fq_limbs
    R = cv.fq_R
    G = (cv.gx, cv.gy)
    pts = [bo.ec_mul(cv, k, G) for k in (1, 2, 3, 5, 7, 1, 11, 7, 13, 5)]
    rng = np.random.default_rng(cid + 10)

    def run(seq, law):
        """seq: list of (point or None, flags); law: the harness's id of the curve and of the field the law is instantiated over"""
        arr = np.zeros((len(seq), 2 * W), dtype="<u4")
        fl = np.zeros(len(seq), dtype=np.uint8)
        for i, (pt, f) in enumerate(seq):
            if pt is not None:
                arr[i, :W] = words(pt[0] * R % cv.q, W)
                arr[i, W:] = words(pt[1] * R % cv.q, W)
            fl[i] = f
        out = np.zeros(2 * W, dtype="<u4")
        inf = fu.fu_xyzz_chain(law, arr.ctypes.data, fl.ctypes.data, len(seq), out.ctypes.data)
        if inf:
            return None
        rinv = pow(R, -1, cv.q)
        return (unwords(out[:W]) * rinv % cv.q, unwords(out[W:]) * rinv % cv.q)

    def expect(seq):
        acc = None
        for pt, f in seq:
            if pt is None:
                continue
            q = bo.ec_neg(cv, pt) if f & 1 else pt
            if f & 4:
                acc = bo.ec_add(cv, acc, acc)
            acc = bo.ec_add(cv, acc, q)
        return acc

    cases = [
        [(pts[0], 0)],
        [(pts[0], 0), (pts[0], 0)],                       # P + P  (madd doubling branch)
        [(pts[0], 0), (pts[0], 1)],                       # P - P  (infinity)
        [(pts[0], 0), (pts[0], 1), (pts[2], 0)],          # back from infinity
        [(pts[1], 0), (pts[2], 0), (pts[3], 2), (pts[3], 2)],   # full add, then full add of same point
        [(pts[1], 2), (pts[1], 2)],                       # add-2008-s doubling branch
        [(pts[1], 2), (pts[1], 3)],                       # add-2008-s cancellation
        [(pts[4], 0), (None, 0), (pts[5], 4), (pts[6], 5), (pts[7], 6)],
        [(p, int(rng.integers(0, 8))) for p in pts] * 3,  # long mixed chain: lazy bounds hold over many ops
    ]
    # the signed-limb field (device), the saturated field (host), and the signed-limb field with the contract of fields.cuh checked
    # at every call and the concrete limbs held against the envelope after every operation (tests/native/fb_field.h)
    log = ctypes.create_string_buffer(1 << 16)
    fu.fb_log_take(log, len(log))
    for law in (cid, cid + 2, cid + 4):
        for seq in cases:
            assert run(seq, law) == expect(seq), (law, seq)
    # the same law on points whose coordinates are base-field edges (tests/edge_values.py): every point alone, so that the output
    # -- to_sat of canon_floor -- is the edge; P + P; P + Q - Q, an edge as the result of real arithmetic; every point against a
    # strided partner under all flag combinations; long mixed chains
    edge = [tuple(e) for e in ev.edge_points(cv)]
    m = len(edge)
    crng = random.Random(0xC4A1 + cid)
    ecases = []
    for i, P in enumerate(edge):
        Q = edge[(7 * i + 3) % m]
        ecases += [[(P, 0)], [(P, 2)], [(P, 0), (P, 0)], [(P, 2), (P, 2)], [(P, 0), (Q, 2 * (i & 1)), (Q, 1 + 2 * (i >> 1 & 1))]]
        ecases += [[(P, f), (Q, g)] for f in range(8) for g in range(8)]
    ecases += [[(edge[crng.randrange(m)], crng.randrange(8)) for _ in range(60)] for _ in range(20)]
    ewant = [expect(seq) for seq in ecases]               # the big-integer reference once, shared by the three laws
    for law in (cid, cid + 2, cid + 4):
        for seq, want in zip(ecases, ewant):
            assert run(seq, law) == want, (law, seq)
    assert fu.fb_log_take(log, len(log)) == 0, log.value.decode()


@pytest.mark.parametrize("field", [0, 1])
def test_signed_limbs_at_the_edge_of_the_column_bound(field, fu):
    """fields.cuh promises: operands with |limb| <= 2^29 + 2 and |value| < 12p go through mul / sqr / dot2 without leaving the signed
    64-bit column, and come out with strict limbs in (-p, p).  Raw limb patterns (no conversion on the way in): every limb at +-(2^29 + 2)
    in all sign combinations that matter (all equal, alternating, one against the other), the top limb at +-12p's, plus random ones."""
    p = bo.BLS12_381.q if field == 0 else bo.BN254.q
    nl = fu.fs_limbs(field)
    Rp = 1 << (30 * nl)
    E = (1 << 29) + 2
    top = (12 * p >> (30 * (nl - 1))) - 1
    rng = np.random.default_rng(field + 77)

    def val(l):
        return sum(int(v) << (30 * i) for i, v in enumerate(l))

    def pat(kind):
        if kind == 0:
            l = [E] * (nl - 1) + [top]
        elif kind == 1:
            l = [-E] * (nl - 1) + [-top]
        elif kind == 2:
            l = [E if i % 2 == 0 else -E for i in range(nl - 1)] + [top]
        elif kind == 3:
            l = [-E if i % 2 == 0 else E for i in range(nl - 1)] + [-top]
        else:
            l = [int(v) for v in rng.integers(-E, E + 1, size=nl - 1)] + [int(rng.integers(-top, top + 1))]
        return np.array(l, dtype=np.int32)

    def strict(l, hi=1):
        return all(-(1 << 29) <= int(v) < (1 << 29) for v in l[:-1]) and abs(val(l)) < hi * p

    out = np.zeros(nl, dtype=np.int32)
    kinds = [0, 1, 2, 3, 4, 4, 4]
    for ka in kinds:
        for kb in kinds:
            a, b, c, d = pat(ka), pat(kb), pat(kb if ka < 4 else 4), pat(ka if kb < 4 else 4)
            A, B, C, D = val(a), val(b), val(c), val(d)
            fu.fs_raw_op(field, 0, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, out.ctypes.data)
            assert strict(out) and (val(out) * Rp - A * B) % p == 0, ("mul", ka, kb)
            fu.fs_raw_op(field, 1, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, out.ctypes.data)
            assert strict(out) and (val(out) * Rp - A * A) % p == 0, ("sqr", ka)
            fu.fs_raw_op(field, 2, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, out.ctypes.data)
            assert strict(out) and (val(out) * Rp - A * B - C * D) % p == 0, ("dot2", ka, kb)
            fu.fs_raw_op(field, 4, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, out.ctypes.data)
            assert val(out) == A + B + C - D and all(abs(int(v)) <= E for v in out[:-1]), ("add3 / sub", ka, kb)
    # the one-step X3: strict operands at the ends of their range
    S = (1 << 29)
    for sa, sb in ((S - 1, -S), (-S, S - 1), (S - 1, S - 1), (-S, -S)):
        a = np.array([sa] * (nl - 1) + [5], dtype=np.int32)
        b = np.array([sb] * (nl - 1) + [-3], dtype=np.int32)
        fu.fs_raw_op(field, 3, a.ctypes.data, b.ctypes.data, b.ctypes.data, b.ctypes.data, out.ctypes.data)
        assert val(out) == val(a) - 3 * val(b) and all(abs(int(v)) <= E for v in out[:-1]), (sa, sb)


# ---- the contract of fields.cuh at every call site of the G1 law (tests/native/fb_field.h, fb_laws.h)
H29 = 1 << 29
STRICT = (-H29, H29 - 1)            # fields.cuh "strict"
ALMOST = (-H29 - 2, H29 + 2)        # fields.cuh "almost"
NEGATED = (-H29 + 1, H29)           # a strict element negated limb-wise
Y_RANGE = (-H29, H29)               # a stored Y: strict or negated
# operation -> its code in fs_raw_op, and operand envelopes (limb range, |value| < V p) AT the extreme of the precondition fields.cuh
# states for it: the rule table must accept each, and the operator must then keep what the table predicts
RULE_CASES = {
    "mul": (0, [[(ALMOST, 12), (ALMOST, 12)], [(ALMOST, 12), (STRICT, 1)]]),
    "sqr": (1, [[(ALMOST, 12)]]),
    "dot2": (2, [[(ALMOST, 12)] * 4, [(ALMOST, 2), (ALMOST, 5), (NEGATED, 1), (STRICT, 1)]]),
    "add": (5, [[((-2 * H29, 2 * H29), 6), ((-H29 + 1, H29 - 1), 6)], [(ALMOST, 4), (ALMOST, 4)]]),
    "sub": (6, [[((-2 * H29, 2 * H29), 6), ((-H29 + 1, H29 - 1), 6)], [(STRICT, 1), (ALMOST, 4)]]),
    "dbl": (7, [[((-3 * H29 // 2 + 1, 3 * H29 // 2 - 1), 6)], [(Y_RANGE, 1)]]),
    "add3": (8, [[((-2 * H29, 2 * H29 - 1), 4), (Y_RANGE, 4), (Y_RANGE, 4)], [(STRICT, 1)] * 3]),
    "sub_sum3": (3, [[(STRICT, 4), (Y_RANGE, 4), (Y_RANGE, 4), (Y_RANGE, 4)], [(STRICT, 1)] * 4]),
    "neg": (9, [[(STRICT, 4)], [(ALMOST, 12)]]),
    "canonical_lt2p": (10, [[(ALMOST, 2)], [(STRICT, 2)]]),
}
# one step past the precondition: the table must refuse each.  (operation, operand envelopes)
RULE_REFUSALS = [
    ("mul", [(ALMOST, 12), ((-H29 - 3, H29 + 2), 12)]), ("mul", [(ALMOST, 12 + 2 ** -16), (ALMOST, 12)]), ("sqr", [((-H29 - 2, H29 + 3), 12)]),
    ("dot2", [(ALMOST, 12), (ALMOST, 12), (ALMOST, 12 + 2 ** -16), (ALMOST, 12)]),
    ("add", [((-2 * H29, 2 * H29), 6), ((-H29 + 1, H29), 6)]), ("sub", [((-2 * H29, 2 * H29), 6), ((-H29, H29 - 1), 6)]),
    ("dbl", [((-3 * H29 // 2, 3 * H29 // 2 - 1), 6)]),
    ("add3", [((-2 * H29, 2 * H29), 4), (Y_RANGE, 4), (Y_RANGE, 4)]), ("add3", [((-2 * H29 - 1, 2 * H29 - 1), 4), (Y_RANGE, 4), (Y_RANGE, 4)]),
    ("sub_sum3", [(Y_RANGE, 4), (Y_RANGE, 4), (Y_RANGE, 4), (Y_RANGE, 4)]), ("sub_sum3", [(STRICT, 4), (ALMOST, 4), (STRICT, 4), (STRICT, 4)]),
    ("is_zero_mod_reduced", [(Y_RANGE, 1)]), ("is_zero_mod_reduced", [(STRICT, 2 + 2 ** -16)]), ("limb0_of_zero_mod", [(ALMOST, 1)]),
    ("canonical_lt2p", [(STRICT, 2 + 2 ** -16)]),
]


def _rule(fu, field, name, envs):
    """the rule table of fb_field.h: (ok, (lo, hi), V as a fraction of 2^-16 p)"""
    ops = {fu.fb_op_name(i).decode(): i for i in range(fu.fb_op_count())}
    unit = fu.fb_units()
    arg = np.array([[lo, hi, round(V * unit)] for (lo, hi), V in envs], dtype=np.int64).reshape(-1)
    res = np.zeros(3, dtype=np.int64)
    ok = fu.fb_rule(field, ops[name], arg.ctypes.data, res.ctypes.data)
    return bool(ok), (int(res[0]), int(res[1])), int(res[2])


@pytest.mark.parametrize("field", [0, 1])
def test_rule_table_is_sound(field, fu):
    """Every rule of the checked field (tests/native/fb_field.h: precondition on the operand envelopes -> envelope of the result) against
    the real operator and big integers.  Operand envelopes at the extreme of each precondition; inside them the limb patterns of the
    column-bound test (every limb at the upper end, at the lower end, alternating both ways, random) with the top limb at +-V p.  The
    result must lie in the predicted envelope and be the exact result: sums as integers, products modulo p after R'.  One step past a
    precondition the table must refuse; for add3 / sub_sum3, whose rule is stated on the raw int32 sum, one step past is shown to be
    wrong as well, so the rule is necessary and not only sufficient.  Prints, per operation, the largest |limb| and |value| / p seen
    against what the rule predicts."""
    p = bo.BLS12_381.q if field == 0 else bo.BN254.q
    nl = fu.fs_limbs(field)
    B, Rp, unit = 1 << (30 * (nl - 1)), 1 << (30 * nl), fu.fb_units()
    rng = random.Random(0xFB + field)

    def val(l):
        return sum(int(v) << (30 * i) for i, v in enumerate(l))

    def operand(env, kind):
        (lo, hi), V = env
        low = {0: [hi] * (nl - 1), 1: [lo] * (nl - 1), 2: [hi if i % 2 == 0 else lo for i in range(nl - 1)],
               3: [lo if i % 2 == 0 else hi for i in range(nl - 1)]}.get(kind) or [rng.randint(lo, hi) for _ in range(nl - 1)]
        lv, edge = val(low), V * p - 1                       # the top limb puts the value at the end of (-V p, V p)
        tmax, tmin = (edge - lv) // B, -((edge + lv) // B)
        top = tmax if kind in (0, 2) else tmin if kind in (1, 3) else rng.randint(tmin, tmax)
        l = np.array(low + [top], dtype=np.int32)
        assert abs(val(l)) < V * p
        return l

    def call(code, ls):
        ls = list(ls) + [ls[-1]] * (4 - len(ls))
        out = np.zeros(nl, dtype=np.int32)
        fu.fs_raw_op(field, code, *[l.ctypes.data for l in ls], out.ctypes.data)
        return out

    exact = {
        "add": lambda v: v[0] + v[1], "sub": lambda v: v[0] - v[1], "dbl": lambda v: 2 * v[0], "add3": lambda v: v[0] + v[1] + v[2],
        "sub_sum3": lambda v: v[0] - v[1] - v[2] - v[3], "neg": lambda v: -v[0],
    }
    modular = {"mul": lambda v: v[0] * v[1], "sqr": lambda v: v[0] * v[0], "dot2": lambda v: v[0] * v[1] + v[2] * v[3]}
    kinds = [0, 1, 2, 3, 4, 4, 4]
    for name, (code, cases) in RULE_CASES.items():
        seen_l, seen_v, pred_l, pred_v = 0, 0, 0, 0
        for envs in cases:
            ok, (lo, hi), V = _rule(fu, field, name, envs)
            assert ok, (name, envs)
            pred_l, pred_v = max(pred_l, -lo, hi), max(pred_v, V / unit)
            for ka in kinds:
                for kb in kinds:
                    ks = [ka, kb, kb if ka < 4 else 4, ka if kb < 4 else 4][:len(envs)]
                    ls = [operand(e, k) for e, k in zip(envs, ks)]
                    vs = [val(l) for l in ls]
                    out = call(code, ls)
                    got = val(out)
                    assert all(lo <= int(x) <= hi for x in out[:-1]), (name, ks)
                    assert abs(got) * unit < V * p, (name, ks, abs(got) / p, V / unit)
                    if name in exact:
                        assert got == exact[name](vs), (name, ks)
                    elif name in modular:
                        assert (got * Rp - modular[name](vs)) % p == 0, (name, ks)
                    else:
                        assert 0 <= got < p and (got - vs[0]) % p == 0, (name, ks)
                    seen_l, seen_v = max([seen_l] + [abs(int(x)) for x in out[:-1]]), max(seen_v, abs(got) / p)
        print(f"field {field} {name}: |limb| seen {seen_l} against {pred_l} predicted, |value|/p seen {seen_v:.6f} against {pred_v:.6f} predicted")
        assert seen_l <= pred_l and seen_v <= pred_v
    # the constants without operands
    assert _rule(fu, field, "zero", []) == (True, (0, 0), 0)
    assert _rule(fu, field, "one", []) == (True, STRICT, unit) and 0 < Rp % p < p
    for name, envs in RULE_REFUSALS:
        assert not _rule(fu, field, name, envs)[0], (name, envs)
    # add3 / sub_sum3 one past int32: the raw sum wraps and the operator is wrong, so their rule cannot be any looser
    big = [np.array([v] * (nl - 1) + [1], dtype=np.int32) for v in (2 * H29, H29, H29, -H29)]
    assert val(call(8, big[:3])) != sum(val(l) for l in big[:3])
    assert val(call(3, [big[3], big[1], big[1], big[1] + 1])) != val(big[3]) - 2 * val(big[1]) - val(big[1] + 1)
    # the zero tests: exact on strict limbs in (-2p, 2p), which their rule demands
    ok, env, V = _rule(fu, field, "is_zero_mod_reduced", [(STRICT, 2)])
    assert ok and env == STRICT and V == 2 * unit and _rule(fu, field, "limb0_of_zero_mod", [(STRICT, 2)])[0]
    for v in [k * p + d for k in (-1, 0, 1) for d in (-1, 0, 1)] + [-2 * p + 1, 2 * p - 1] + [rng.randrange(-2 * p + 1, 2 * p) for _ in range(200)]:
        l = np.array(ev.strict_limbs(v, nl), dtype=np.int32)
        assert val(l) == v and all(STRICT[0] <= int(x) <= STRICT[1] for x in l[:-1])
        assert bool(call(11, [l])[0]) == (v % p == 0), hex(v)
        assert call(12, [l])[0] or v % p != 0, hex(v)


# function / branch outcome: what the closure runs must be exactly this list (ecu.cuh; the issue names every entry)
SINGLE_LANE_CASES = ["setup", "from_affine", "dbl_affine", "dbl/infinity", "dbl/general",
                     "madd/p infinite", "madd/P = Q", "madd/P = -Q", "madd/general",
                     "madd_begin + madd_finish/general", "madd_begin + madd_finish/P = Q", "madd_begin + madd_finish/P = -Q",
                     "add/p infinite", "add/q infinite", "add/P = Q", "add/P = -Q", "add/general", "neg",
                     "to_affine/infinity", "to_affine/general", "to_affine_given"]
# every lane of a quad runs every instruction; the four roles are checked in each case.  "qadd alone" is a wave in which no quad
# has P = +-Q, so the branch around the quad doubling is not taken; in "qadd" all cases share one wave and every lane takes it
QUAD_CASES = ["setup", "qadd/inputs", "qadd/general", "qadd/P = Q", "qadd/P = -Q", "qadd/p infinite", "qadd/q infinite", "qadd/both infinite",
              "qadd alone/inputs", "qadd alone/general", "qdbl/inputs", "qdbl/general", "qdbl/infinity"]
# Violations in lanes whose value nobody reads: "site|role|operation" -> why the value is unread.  Each entry exempts exactly the
# records it names and must occur; an entry may never name a role whose result of that operation is selected into `res`.
# There are none: with inputs inside the class invariant every lane of qadd and qdbl, dead ones included, stays inside the contract
# (the dead lanes multiply and subtract products and stored coordinates like the live ones).
DEAD_LANE_EXEMPTIONS = {}


def _closure(fu, cid, which):
    cv = bo.CURVES[cid]
    W = 2 * cv.fq_limbs
    G = (cv.gx, cv.gy)
    P, Q = bo.ec_mul(cv, 3, G), bo.ec_mul(cv, 5, G)          # Q != +-P; 2P, 2Q, 4P, 2P + Q, 2P + 2Q all finite
    arr = np.concatenate([words(c * cv.fq_R % cv.q, W) for c in P + Q])
    buf = ctypes.create_string_buffer(1 << 18)
    failures = fu.fb_closure(cid, which, arr.ctypes.data, buf, len(buf))
    lines = buf.value.decode().splitlines()
    return failures, lines


@pytest.mark.parametrize("cid", [0, 1])
def test_g1_law_is_closed_under_the_signed_limb_contract(cid, fu):
    """XYZZu (ecu.cuh) over the checked field, every function once per branch outcome on a concrete input that takes the branch, the
    input envelopes widened to the class invariant ("Signed-limb contract of the G1 law"): no precondition of fields.cuh
    is missed at any call site, every output envelope is inside the invariant again, and the result is the group element the branch
    gives.  Envelopes do not depend on values, so this is the induction step for every chain of these functions on every input."""
    failures, lines = _closure(fu, cid, 0)
    assert failures == 0 and all(l.startswith("CASE ") for l in lines), "\n".join(l for l in lines if not l.startswith("CASE "))
    assert [l[5:] for l in lines] == SINGLE_LANE_CASES


@pytest.mark.parametrize("cid", [0, 1])
def test_quad_law_is_closed_under_the_signed_limb_contract(cid, fu):
    """qadd and qdbl of ecq.cuh, the file as the kernels compile it, over the checked field: four host threads per quad in lockstep
    behind host definitions of the wave primitives, the envelope travelling with every limb through the shuffles.  General case, the
    P = +-Q slow path and the infinity paths; per role the result envelope is inside the class invariant, and the gathered point is
    the group element the single-lane law gives.  A violation is tolerated only in a lane listed in DEAD_LANE_EXEMPTIONS."""
    failures, lines = _closure(fu, cid, 1)
    recorded = [l[len("QUADVIOLATION "):] for l in lines if l.startswith("QUADVIOLATION ")]
    rest = [l for l in lines if not l.startswith("QUADVIOLATION ")]
    assert failures == 0 and all(l.startswith("CASE ") for l in rest), "\n".join(l for l in rest if not l.startswith("CASE "))
    assert [l[5:] for l in rest] == QUAD_CASES
    keys = {"|".join(r.split("|")[:3]) for r in recorded}
    assert keys == set(DEAD_LANE_EXEMPTIONS), "\n".join(recorded)


# ---- the scalar field's lazily normalised operators (fieldu.cuh) and the numeric rules of zbound.cuh, on raw 29-bit limbs
U29 = 1 << 29
FU_OPS = {"mul": 0, "mul_fenced": 1, "sqr": 2, "add": 3, "add3": 4, "sub2": 5, "sub8": 6, "sub16": 7, "neg16": 8, "add_raw": 9,
          "sub_raw3": 10, "sub_raw8": 11, "sub_raw16": 12, "sweep": 13, "canonical_lt2p": 14, "is_zero_mod_reduced": 15}
FU_KINDS = [0, 1, 2, 3, 4, 4, 4]


def ntt_units_before(t):
    """ntt_pass.cuh: limb units of a lane's registers before stage t of a pass"""
    b = 1
    for _ in range(t):
        if b > 6:
            b = 1
        b += 2
    return b


class RawFu:
    """Fu<P> of the harness on raw limbs (lists of Python integers in, lists out), for field 1 (Fr of BLS12-381) or 3 (BN254)"""

    def __init__(self, fu, field):
        self.fu, self.field, self.r = fu, field, FIELDS[field][0]
        self.nl = fu.fu_limbs(field)
        self.B, self.Rp = 1 << (29 * (self.nl - 1)), 1 << (29 * self.nl)      # the top limb's weight; the Montgomery radix R'
        self.rng = random.Random(0xF0 + field)
        self.zero = [0] * self.nl

    @staticmethod
    def val(l):
        return sum(int(v) << (29 * i) for i, v in enumerate(l))

    def limbs(self, v):
        """the normalised limbs of v"""
        return [(v >> (29 * i)) & (U29 - 1) for i in range(self.nl - 1)] + [v >> (29 * (self.nl - 1))]

    def swept(self, l):
        return all(0 <= v < U29 for v in l[:-1]) and 0 <= l[-1] < 1 << 32

    def units(self, l):
        return max(l[:-1]) // U29 + 1

    def call(self, name, *ls):
        assert all(0 <= v < 1 << 32 for l in ls for v in l), name
        arrs = [np.array(l, dtype=np.uint32) for l in ls]
        arrs += [arrs[-1]] * (3 - len(arrs))
        out = np.zeros(self.nl, dtype=np.uint32)
        self.fu.fu_raw_op(self.field, FU_OPS[name], *[a.ctypes.data for a in arrs], out.ctypes.data)
        return [int(v) for v in out]

    def operand(self, units, bound, kind):
        """Limbs below the top one in [0, units * 2^29): all at the upper end (kind 0), all zero (1), alternating (2, 3), else random;
        the top limb puts the value just below `bound` (random kinds: anywhere below it)."""
        hi, n = units * U29 - 1, self.nl - 1
        low = {0: [hi] * n, 1: [0] * n, 2: [hi if i % 2 == 0 else 0 for i in range(n)],
               3: [0 if i % 2 == 0 else hi for i in range(n)]}.get(kind) or [self.rng.randint(0, hi) for _ in range(n)]
        tmax = (bound - 1 - self.val(low)) // self.B
        assert 0 <= tmax < 1 << 32
        l = low + [tmax if kind < 4 else self.rng.randint(0, tmax)]
        assert self.val(l) < bound and (kind >= 4 or self.val(l) + self.B >= bound)
        return l

    def product_columns(self, a, b):
        """Fu::mul / mul_fenced restated on integers: (the largest 64-bit column total, the result limbs)"""
        nl, M, mod = self.nl, U29 - 1, self.limbs(self.r)
        pinv = (-pow(self.r, -1, U29)) % U29
        m, out, carry, worst = [], [], 0, 0
        for k in range(nl):
            t = carry + sum(a[i] * b[k - i] for i in range(k + 1)) + sum(m[i] * mod[k - i] for i in range(k))
            m.append((t * pinv) & M)
            t += m[k] * mod[0]
            assert t & M == 0
            worst, carry = max(worst, t), t >> 29
        for k in range(nl, 2 * nl - 1):
            t = carry + sum(a[i] * b[k - i] + m[i] * mod[k - i] for i in range(k - nl + 1, nl))
            out.append(t & M)
            worst, carry = max(worst, t), t >> 29
        return worst, out + [carry]

    def checked_product(self, a, b, what):
        """mul and mul_fenced of a, b: equal limb for limb, every column inside 64 bits, the result swept, below 2r and a b / R'"""
        worst, want = self.product_columns(a, b)
        assert worst < 1 << 64, (what, worst / 2 ** 64)
        got = self.call("mul", a, b)
        assert got == self.call("mul_fenced", a, b) == want, what
        assert self.swept(got) and self.val(got) < 2 * self.r and (self.val(got) * self.Rp - self.val(a) * self.val(b)) % self.r == 0, what
        return got, worst

    def checked_sub_raw(self, name, a, b, what):
        """sub_raw3/8/16: limb-wise a + k r - b computed here without wrap; no limb below zero or past 32 bits, at most units(a) + 2"""
        zb = self.call(name, self.zero, self.zero)
        want = [x + z - y for x, z, y in zip(a, zb, b)]
        assert all(0 <= v < 1 << 32 for v in want), (what, want)
        assert all(v < (self.units(a) + 2) * U29 for v in want[:-1]), what
        got = self.call(name, a, b)
        assert got == want and self.val(got) == self.val(a) + self.val(zb) - self.val(b), what
        return got


@pytest.mark.parametrize("field", [1, 3])
def test_lazy_limbs_at_the_edge_of_the_column_bound(field, fu):
    """The lazily normalised operators of the NTT butterflies (fieldu.cuh) at the ends of the contracts their comments state, on raw
    limb patterns: limbs below the top one all at the upper end of their range, all zero, alternating both ways and random, the top limb
    putting the value just below its bound.
    mul / mul_fenced: a first operand of 6 units just below 47r (the bound of a pass, ntt_pass.cuh) and just below K r, K the largest
    multiple with K r b <= 2^261 r, against a swept second operand just below r: every 64-bit column total (restated here on integers)
    stays below 2^64, the two products agree limb for limb with the restatement, the result is swept, below 2r and a b / 2^261.
    sub_raw3/8/16: a of 1, 3 and 5 units (below 2r, 5r, 13r: a fresh product, after stage 0, after stage 1 of a pass), b swept and just
    below 2r / 7r / 15r: the exact integer a + k r - b, no limb below zero or past 32 bits, at most units(a) + 2; one step past the
    precondition (a b whose top limb exceeds the constant's; an unswept b) the result is wrong, so the bound is necessary.
    add_raw: the exact sum, units add up to the 8 a limb holds.  sweep: 7 units (the most ntt_units_before reaches) below 47r: same
    value, swept, the top limb inside 29 bits.  ZB3/8/16: 3r / 8r / 16r with limbs below the top in [2^29, 2^30) and a top limb that covers
    every swept value below 2r / 7r / 15r.  Then the unit schedule of one radix-9 pass replayed with these operators."""
    F = RawFu(fu, field)
    r, Rp = F.r, F.Rp
    assert F.nl == 9 and 47 * r < Rp
    # ---- the product
    worst = 0
    for kb in [0, 1, 2, 3, 4]:
        b = F.operand(1, r, kb)
        K = Rp // F.val(b) if F.val(b) else Rp // r           # a < K r gives a b < 2^261 r
        assert K >= Rp // r >= 70
        for bound in (47 * r, min(K * r, 6 * U29 * F.B)):       # the top limb counts among the 6 units as well
            for ka in FU_KINDS:
                a = F.operand(6, bound, ka)
                assert F.val(a) * F.val(b) < Rp * r
                worst = max(worst, F.checked_product(a, b, (kb, bound // r, ka))[1])
    # the column argument itself (fieldu.cuh: 9 * 6 * 2^58 + 9 * 2^58 + carry < 2^64, a margin of 1/64) speaks of limbs only: EVERY limb of
    # the first operand at 6 * 2^29 - 1 and of the second at 2^29 - 1, which no value inside the bounds above has in its top limb.  The
    # product is then past 2r, but still a b / 2^261, and no column may wrap
    a, b = [6 * U29 - 1] * F.nl, [U29 - 1] * F.nl
    full, want = F.product_columns(a, b)
    got = F.call("mul", a, b)
    assert got == F.call("mul_fenced", a, b) == want and (F.val(got) * Rp - F.val(a) * F.val(b)) % r == 0
    print(f"field {field}: largest product column {worst / 2 ** 64:.6f} of 2^64 inside the value bounds, {full / 2 ** 64:.6f} with every limb at its end")
    assert 48 << 58 < worst < full < 1 << 64 and full > 54 << 58
    # ---- the constants, and the differences
    for name, k, cover in (("sub_raw3", 3, 2), ("sub_raw8", 8, 7), ("sub_raw16", 16, 15)):
        zb = F.call(name, F.zero, F.zero)
        assert F.val(zb) == k * r and all(U29 <= v < 2 * U29 for v in zb[:-1]), name
        assert zb[-1] >= (cover * r - 1) // F.B, name                                  # the top limb of any swept value below cover * r
        for units, abound in ((1, 2), (3, 5), (5, 13)):
            for ka in FU_KINDS:
                for kb in FU_KINDS:
                    a, b = F.operand(units, abound * r, ka), F.operand(1, cover * r, kb)
                    F.checked_sub_raw(name, a, b, (name, units, ka, kb))
        # one step past: a swept b whose top limb exceeds the constant's (just below 7r / 16r / 32r); a b that is not swept
        a, past = F.operand(1, 2 * r, 0), F.operand(1, {3: 7, 8: 16, 16: 32}[k] * r, 0)
        assert a[-1] + zb[-1] - past[-1] < 0 and F.val(F.call(name, a, past)) != F.val(a) + k * r - F.val(past), name
        wide = F.operand(3, 2 * r, 0)
        assert F.val(F.call(name, F.zero, wide)) != k * r - F.val(wide), name
    # ---- sums without a sweep, and the sweep
    for ua, ub in ((1, 1), (3, 1), (5, 1), (3, 3), (5, 3), (7, 1)):
        for ka in FU_KINDS:
            for kb in FU_KINDS:
                a, b = F.operand(ua, 47 * r, ka), F.operand(ub, 47 * r, kb)
                got = F.call("add_raw", a, b)
                assert got == [x + y for x, y in zip(a, b)] and F.units(got) <= ua + ub <= 8, (ua, ub, ka, kb)
    for ka in FU_KINDS:
        a = F.operand(7, 47 * r, ka)
        got = F.call("sweep", a)
        assert got == F.limbs(F.val(a)) and F.swept(got) and got[-1] < U29, ka
    # ---- one radix-9 pass: three windows of three stages on the eight registers of a lane (dit_window), the sweeps where ntt_sweep_at
    # takes them, the product-free butterflies of the first window; every register's residue followed on integers
    Rinv = pow(Rp, -1, r)
    after = [5, 13, 29, 32, 35, 38, 41, 44, 47]                 # value bound in r after stage t: ntt_pass.cuh "the pass still ends below 47r"
    for run in range(3):
        if run == 0:                                            # the all-high pattern, just below 2r
            x = [F.operand(1, 2 * r - e * F.B, 0) for e in range(8)]
        else:
            x = [F.operand(1, 2 * r, 4) for _ in range(8)]
        exp = [F.val(l) % r for l in x]
        for t in range(9):
            lb, first = t % 3, t < 3
            claimed = ntt_units_before(t)
            assert claimed <= 7 and all(F.units(l) <= claimed for l in x), t
            if claimed > 6:                                     # ntt_sweep_at(t)
                x = [F.call("sweep", l) for l in x]
                assert all(F.swept(l) and F.val(l) % r == v for l, v in zip(x, exp))
                claimed = 1
            for e in range(8):
                if e & (1 << lb):
                    continue
                eo = e | (1 << lb)
                if first and (lb == 0 or e & ((1 << lb) - 1) == 0):       # the twiddle is 1
                    m = x[eo] if lb == 0 else F.call("sweep", x[eo])
                    assert F.swept(m) and F.val(m) < (2, 7, 15)[lb] * r, (t, e)
                    name, tw = ("sub_raw3", "sub_raw8", "sub_raw16")[lb], Rp % r
                else:
                    assert F.units(x[eo]) <= claimed <= 5, (t, e)          # at most 5 units into a product
                    w = F.operand(1, r, (e + t) % 5)
                    m, _ = F.checked_product(x[eo], w, (t, e))
                    name, tw = "sub_raw3", F.val(w)
                te = exp[eo] * tw * Rinv % r
                x[eo], x[e] = F.checked_sub_raw(name, x[e], m, (t, e)), F.call("add_raw", x[e], m)
                exp[eo], exp[e] = (exp[e] - te) % r, (exp[e] + te) % r
            assert all(F.val(l) < after[t] * r and F.val(l) % r == v for l, v in zip(x, exp)), t
        assert ntt_units_before(9) == 7 and all(F.units(l) <= 7 for l in x)        # the sweep in front of the last product
        scale = F.operand(1, r, 0)
        for l, v in zip(x, exp):
            y, _ = F.checked_product(F.call("sweep", l), scale, "scale")
            c = F.call("canonical_lt2p", y)
            assert F.swept(c) and F.val(c) == v * F.val(scale) * Rinv % r


@pytest.mark.parametrize("field", [1, 3])
def test_z_rules_are_sound(field, fu):
    """The numbers of zbound.cuh (Z<F, B>: a value below B / 10 r) against the operators at the extreme each rule admits, on swept
    operands in the limb patterns of the test above.  Products with A B <= 6400: (8r, 8r), (64r, r), (32r, 2r) in both orders and the
    square of 8r come out below 2r and congruent.  Sums up to 640 (kzg.hip: 32 products below 2r): exact, normalised, the top limb inside 29 bits.  Differences through
    sub2 / sub8 / sub16 (SubK: 2r / 8r / 16r): subtrahend just below the multiple, minuend 0 and at the most the sum rule leaves: exact,
    normalised, no negative top limb.  The two tests on values below 2r: exact on 0, r, r +- 1, 2r - 1 and random ones."""
    F = RawFu(fu, field)
    r, Rp = F.r, F.Rp
    text = open(os.path.join(ROOT, "ark_plonk_amd", "csrc", "zbound.cuh")).read()
    prod_max = int(re.search(r"static_assert\(A \* B <= (\d+),", text).group(1))
    sum_max = int(re.search(r"static_assert\(A \+ B <= (\d+),", text).group(1))
    assert re.search(r"K = B <= 20 \? 20 : B <= 80 \? 80 : 160;", text) and "A * A <= %d" % prod_max in text
    assert (prod_max, sum_max) == (6400, 640) and sum_max * r < 10 * Rp

    def below(tenths, kind):
        return F.operand(1, tenths * r // 10, kind)

    for A, B in ((80, 80), (640, 10), (320, 20)):
        assert A * B == prod_max
        for ka in FU_KINDS:
            for kb in FU_KINDS:
                a, b = below(A, ka), below(B, kb)
                F.checked_product(a, b, (A, B, ka, kb))
                F.checked_product(b, a, (B, A, kb, ka))
    for ka in FU_KINDS:
        a = below(80, ka)
        got = F.call("sqr", a)
        assert got == F.call("mul", a, a) and F.swept(got) and F.val(got) < 2 * r and (F.val(got) * Rp - F.val(a) ** 2) % r == 0, ka
    for A, B in ((320, 320), (630, 10), (10, 630), (440, 200)):
        assert A + B == sum_max
        for ka in FU_KINDS:
            for kb in FU_KINDS:
                a, b = below(A, ka), below(B, kb)
                got = F.call("add", a, b)
                assert got == F.limbs(F.val(a) + F.val(b)) and got[-1] < U29, (A, B, ka, kb)
                c = below(B // 2, kb)
                assert F.call("add3", a, c, c) == F.limbs(F.val(a) + 2 * F.val(c)), (A, B, ka, kb)
    for name, k in (("sub2", 2), ("sub8", 8), ("sub16", 16)):
        for kb in FU_KINDS:
            b = F.operand(1, k * r, kb)
            for a in [F.zero] + [below(sum_max - 10 * k, ka) for ka in FU_KINDS]:
                got = F.call(name, a, b)
                assert got == F.limbs(F.val(a) + k * r - F.val(b)) and got[-1] < U29, (name, kb)
            if k == 16:
                assert F.call("neg16", b) == F.limbs(16 * r - F.val(b)), kb
    vs = [0, 1, r - 1, r, r + 1, 2 * r - 1] + [F.rng.randrange(2 * r) for _ in range(300)]
    for v in vs:
        l = F.limbs(v)
        assert bool(F.call("is_zero_mod_reduced", l)[0]) == (v % r == 0), hex(v)
        assert F.call("canonical_lt2p", l) == F.limbs(v % r), hex(v)


# ---- the load conversion of the quotient kernel and the circuit check (zbound.cuh)
def _table_rows():
    """QTAB and CTAB: the multiples of r the two kernels hold"""
    out = []
    for unit, name in (("quotient.hip", "QTAB"), ("check.hip", "CTAB")):
        text = open(os.path.join(ROOT, "ark_plonk_amd", "csrc", unit)).read()
        out.append(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1)))
    return out


@pytest.mark.parametrize("field", [1, 3])
def test_to_rp_is_32v_below_its_bound(field, fu):
    """to_rp(v) for the stored word v: congruent to 32 v, normalised limbs, below RP_B / 10 * r -- the premise of every Z<F, B> rule
    the two kernels compile under -- and never past the multiples of r either kernel holds.  Boundary words (where the true quotient
    and the truncated top the estimate starts from step) and 10^5 random canonical words.  The multiple of r that was taken off,
    (32 v - result) / r, is q2 or q2 + 1: it bounds q2 from above."""
    r = FIELDS[field][0]
    rng = random.Random(0x70 + field)
    vs = ev.to_rp_boundary_words(r) + [rng.randrange(r) for _ in range(100000)]
    nl, bound = fu.fu_rp_limbs(), fu.fu_rp_bound()
    win = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vs), dtype="<u4").copy()
    out = np.zeros(nl * len(vs), dtype="<u4")
    fu.fu_to_rp(field, win.ctypes.data, out.ctypes.data, len(vs))
    assert int(out.max()) < 1 << 29, "limbs not normalised"
    limbs = out.reshape(len(vs), nl).astype(object)
    got = [int(sum(int(l[i]) << (29 * i) for i in range(nl))) for l in limbs]
    worst, worst_q = 0, 0
    for v, g in zip(vs, got):
        assert (g - 32 * v) % r == 0, hex(v)
        worst, worst_q = max(worst, g), max(worst_q, (32 * v - g) // r)
    print(f"to_rp field {field}: largest result {worst / r:.6f} r, largest multiple of r taken off {worst_q}")
    assert 10 * worst < bound * r, f"{worst / r:.4f} r against a bound of {bound / 10} r"
    assert worst_q < min(_table_rows())


@pytest.mark.parametrize("field", [1, 3])
def test_host_rprime_packer(field, fu):
    """The one host conversion behind every kernel-argument multiplier and the NTT's tables (pack_rp / to_rprime, fr_io.cuh): the stored
    word w = x R goes to 32 w mod r = x R', canonical -- against Python integers, against to_rp_host (zbound.cuh: the same value as
    normalised limbs) and against the route the units used to write out, one Montgomery product with R' mod r.  0, 1, r - 1 and the
    edge set, as values and as stored words."""
    r = FIELDS[field][0]
    cv = bo.BLS12_381 if field == 1 else bo.BN254
    edges = [0, 1, r - 1] + list(ev.edge_elements(cv))
    ws = sorted(set(edges + [ev.stored_word(cv, v) for v in edges]))
    nl = fu.fu_rp_limbs()
    win = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in ws), dtype="<u4").copy()
    packed, limbs, prod = np.zeros(8 * len(ws), dtype="<u4"), np.zeros(nl * len(ws), dtype="<u4"), np.zeros(8 * len(ws), dtype="<u4")
    fu.fu_pack_rp(field, win.ctypes.data, packed.ctypes.data, limbs.ctypes.data, prod.ctypes.data, len(ws))
    assert int(limbs.max()) < 1 << 29, "limbs not normalised"
    for k, w in enumerate(ws):
        want = 32 * w % r
        assert unwords(packed[8 * k:8 * k + 8]) == want, hex(w)
        assert unwords(prod[8 * k:8 * k + 8]) == want, hex(w)
        assert sum(int(limbs[nl * k + i]) << (29 * i) for i in range(nl)) == want, hex(w)


# ---- the domain constants and the identity encoding (domain.cuh), the shared host fillers of the gate-argument blocks (zbound.cuh)
@pytest.mark.parametrize("field", [1, 3])
def test_domain_root_has_its_order(field, fu):
    """domain_root(log_n), every log_n up to the two-adicity: its 2^log_n-th power is 1 and (log_n >= 1) its 2^(log_n - 1)-th is -1, so
    its order is 2^log_n exactly; the guard admits the two-adicity and refuses the next size."""
    cv = bo.BLS12_381 if field == 1 else bo.BN254
    r, Rinv = cv.r, pow(1 << 256, -1, cv.r)
    out = np.zeros(8, dtype="<u4")
    for log_n in range(cv.two_adicity + 1):
        assert fu.fu_domain_log_ok(field, log_n)
        fu.fu_domain_root(field, log_n, out.ctypes.data)
        assert unwords(out) < r
        w = unwords(out) * Rinv % r
        assert pow(w, 1 << log_n, r) == 1, log_n
        if log_n >= 1:
            assert pow(w, 1 << (log_n - 1), r) == r - 1, log_n
        assert w == cv.root_of_unity(log_n), log_n
    assert not fu.fu_domain_log_ok(field, cv.two_adicity + 1)


@pytest.mark.parametrize("field,log_n", [(1, 13), (3, 9)])
def test_identity_constants_against_integers(field, log_n, fu):
    """fill_id_consts: K_0..K_3 = 1, 7, 13, 17 (the reference's permutation cosets), then omega^(2^j) for j < 28 -- the squares past
    j = log_n are 1 -- as stored Montgomery words."""
    cv = bo.BLS12_381 if field == 1 else bo.BN254
    r, R = cv.r, 1 << 256
    nc = fu.fu_id_n_consts()
    assert nc == 4 + 28
    out = np.zeros(8 * nc, dtype="<u4")
    fu.fu_id_consts(field, log_n, out.ctypes.data)
    w = cv.root_of_unity(log_n)
    want = [1, 7, 13, 17] + [pow(w, 1 << j, r) for j in range(nc - 4)]
    assert want[4 + log_n - 1] == r - 1 and want[4 + log_n] == 1
    for k, v in enumerate(want):
        assert unwords(out[8 * k:8 * k + 8]) == v * R % r, k


@pytest.mark.parametrize("field", [1, 3])
def test_gate_constants_against_integers(field, fu):
    """fill_gate_consts, which fills the argument blocks of quotient.hip and check.hip: the ten shared constants are x R' mod r
    (R' = 2^261) as normalised 29-bit limbs -- 32 w mod r for the two curve coefficients, which arrive as stored words w --; rtab[q] is
    q r, ratio_fx = floor(2^(BITS + 10) / r) - 1, top_shift = BITS - 29 (NL - 1): what the two units' own fillers wrote."""
    cv = bo.BLS12_381 if field == 1 else bo.BN254
    r, nl = cv.r, fu.fu_rp_limbs()
    rng = random.Random(0x6A + field)

    def limbs(v):
        return [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(nl - 1)] + [v >> (29 * (nl - 1))]

    for rows in sorted(set(_table_rows())) + [64]:
        for wa, wd in ((0, r - 1), (rng.randrange(r), rng.randrange(r))):
            ca, cd = np.frombuffer(wa.to_bytes(32, "little"), dtype="<u8").copy(), np.frombuffer(wd.to_bytes(32, "little"), dtype="<u8").copy()
            lo, rt, sc = np.zeros(10 * nl, dtype="<u4"), np.zeros(rows * nl, dtype="<u4"), np.zeros(2, dtype="<u4")
            fu.fu_gate_consts(field, ca.ctypes.data, cd.ctypes.data, rows, lo.ctypes.data, rt.ctypes.data, sc.ctypes.data)
            want = [32 * wa % r, 32 * wd % r] + [x * (1 << 261) % r for x in (1, 2, 3, 4, 9, 18, 81, 83)]
            for k, v in enumerate(want):
                assert [int(x) for x in lo[nl * k:nl * (k + 1)]] == limbs(v), k
            for q in range(rows):
                assert [int(x) for x in rt[nl * q:nl * (q + 1)]] == limbs(q * r), q
            bits = r.bit_length()
            assert int(sc[0]) == (1 << (bits + 10)) // r - 1 and int(sc[1]) == bits - 29 * (nl - 1)


# ---- the hash of the device key maps (fr_io.cuh) and its restatement
def _w8(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u4").copy()


def test_hash_restatement_and_crafted_collisions(fu):
    """tests/edge_values.py restates el_mix / key_hash; the crafted collisions of the GPU suite collide under the restatement, so it
    has to BE the compiled hash: on random words and chains, on every colliding pair (equal el_mix from any chained state, distinct
    words, both canonical on both curves) and on every member of a slot cluster."""
    rng = random.Random(0xE1)
    for _ in range(2000):
        v, h = rng.getrandbits(256), rng.getrandbits(64)
        assert fu.fu_el_mix(h, _w8(v).ctypes.data) == ev.el_mix(h, v)
        assert fu.fu_el_mix(0, _w8(v).ctypes.data) & 0xFFFFFFFF == ev.el_hash(v)
        key = [rng.getrandbits(256) for _ in range(4)]
        buf = np.concatenate([_w8(k) for k in key])
        assert fu.fu_key_hash(4, buf.ctypes.data) == ev.key_hash(key)
        assert fu.fu_key_hash(1, buf.ctypes.data) == ev.key_hash(key[:1])
    small_r = min(bo.BLS12_381.r, bo.BN254.r)
    for _ in range(500):
        a, b = ev.colliding_pair(rng)
        h = rng.getrandbits(64)
        assert a != b and a < small_r and b < small_r and a >> 252 == 0 and b >> 252 == 0
        assert fu.fu_el_mix(h, _w8(a).ctypes.data) == fu.fu_el_mix(h, _w8(b).ctypes.data) == ev.el_mix(h, a)
        pre = [rng.getrandbits(256) for _ in range(3)]
        ka, kb = np.concatenate([_w8(k) for k in pre + [a]]), np.concatenate([_w8(k) for k in pre + [b]])
        assert fu.fu_key_hash(4, ka.ctypes.data) == fu.fu_key_hash(4, kb.ctypes.data) == ev.key_hash(pre + [a])
    for cv in (bo.BLS12_381, bo.BN254):                    # a partner of a given word (an identity encoding of the copy map)
        v = ev.stored_word(cv, 7 * cv.root_of_unity(3) % cv.r)
        p = ev.colliding_partner(v, rng)
        assert p != v and fu.fu_key_hash(1, _w8(p).ctypes.data) == fu.fu_key_hash(1, _w8(v).ctypes.data)
        assert ev.stored_word(cv, ev.field_value(cv, p % cv.r)) == p % cv.r
    for mask, slot in ((1023, 1023), (1023, 1022), (511, 511)):
        pre = [rng.getrandbits(256) for _ in range(3)]
        for v in ev.slot_cluster(mask, slot, 8, ev.el_hash, seed=1):
            assert fu.fu_el_mix(0, _w8(v).ctypes.data) & mask == slot
        wide = ev.slot_cluster(mask, slot, 8, lambda v: ev.key_hash(pre + [v]), seed=2)
        assert len(set(wide)) == 8
        for v in wide:
            assert fu.fu_key_hash(4, np.concatenate([_w8(k) for k in pre + [v]]).ctypes.data) & mask == slot


@pytest.mark.parametrize("cid", [0, 1])
def test_edge_elements_are_what_they_say(cid):
    cv = bo.CURVES[cid]
    e = ev.edge_elements(cv)
    assert len(set(e)) == len(e) and all(0 <= x < cv.r for x in e)
    for x in (0, 1, 2, 3, cv.r - 1, cv.r - 2, cv.r - 3, (cv.r - 1) // 2, (cv.r + 1) // 2, 1 << 29, (1 << 232) - 1, 1 << 192, (1 << 64) - 1):
        assert x in e
    words = ev.to_rp_boundary_words(cv.r)
    assert all(ev.field_value(cv, v) in e for v in words) and len(words) > 150


# ---- curve points with base-field edges as coordinates (tests/edge_values.py)
@pytest.mark.parametrize("cid", [0, 1])
def test_edge_points_are_what_they_say(cid, fu):
    cv = bo.CURVES[cid]
    q, nl = cv.q, ev.FS_LIMBS[cid]
    assert nl == fu.fs_limbs(cid)
    pts = ev.edge_points(cv)
    assert len(pts) >= 100 and len(set(tuple(e) for e in pts)) == len(pts)
    assert all(0 <= e[0] < q and 0 < e[1] < q and bo.on_curve(cv, tuple(e)) for e in pts)
    worst = max(e.dist for e in pts)
    print(f"{cv.name}: {len(pts)} edge points, largest search distance {worst}")
    assert worst < 32
    patterned = 0
    for e in pts:
        c = e[1] if e.side == "y" else e[0]                     # the coordinate that was aimed
        got = c * ev.form_factor(cv, e.form) % q
        assert abs(got - e.target) == e.dist, (e.form, e.side, hex(e.target))
        if e.pattern is not None:                               # the walk moved limb 0 alone
            limbs = ev.strict_limbs(got, nl)
            assert ev.limbs_value(limbs) == got and limbs[1:nl - 1] == e.pattern[1:nl - 1] and limbs[nl - 1] == e.pattern[nl - 1], e.pattern
            assert abs(limbs[0] - e.pattern[0]) == e.dist
            patterned += 1
    assert patterned >= 10
    for form in ("value", "stored", "internal"):                # the ends of the field, in every form, are in
        have = {e[0] * ev.form_factor(cv, form) % q for e in pts}
        assert any(t in have for t in range(0, 16)) and any(q - t in have for t in range(1, 16)), form
    if cid == 0:
        assert (0, 2) in pts and bo.ec_mul(cv, 3, (0, 2)) is None
    else:
        assert (cv.gx, cv.gy) in pts


@pytest.mark.parametrize("cid", [0, 1])
def test_references_agree_on_edge_points(cid, oracle_cpu):
    """The pure-Python group law and the C++ restatement of the arkworks Pippenger give the same MSM over the whole edge set -- the
    vector of tests/test_edge_points_gpu.py, with its repeated and opposite points, the point of order 3 and the infinities -- so the
    GPU tests may take the restatement alone: scalars in [0, (r - 1) / 2] on both curves and the whole range on BN254, as the MSMs
    of the GPU tests take them (a BLS12-381 edge point is outside the r-torsion subgroup); and the two-point sums L + xi R of the
    key-fold test, where the scalar is an integer on both sides, with xi up to r - 1 on both curves."""
    cv = bo.CURVES[cid]
    for top in ((cv.r - 1) // 2,) + ((cv.r - 1,) if cid == 1 else ()):
        rows = ev.edge_msm_rows(cv, top)
        sc = [s for _, s, _ in rows]
        assert {0, 1, top} <= set(sc) and max(sc) <= top
        assert {tuple(e) for e in ev.edge_points(cv)} <= {p for p, _, _ in rows} and {e for _, _, e in rows} == {0, 1, 2, 3}
        want = bo.msm(cv, [p for p, _, _ in rows], sc)
        bases, scal, _, flags = ev.rows_arrays(cv, rows)
        xy, inf = oracle_cpu.msm_g1(cid, bases, scal, inf=flags)
        assert want is not None and not inf
        assert np.array_equal(xy, ev.points_to_limbs(cv, [want])[0]), hex(top)
    pts = [tuple(e) for e in ev.edge_points(cv)]
    for i in range(0, len(pts), 9):
        pair = [pts[i], pts[(i + 37) % len(pts)]]
        for xi in (0, 1, 2, cv.r - 1):
            want = bo.ec_add(cv, pair[0], bo.ec_mul(cv, xi, pair[1]))
            xy, inf = oracle_cpu.msm_g1(cid, ev.points_to_limbs(cv, pair), oracle_cpu.ints_to_limbs([1, xi], 4), threads=1)
            assert not inf and np.array_equal(xy, ev.points_to_limbs(cv, [want])[0]), (i, hex(xi))
