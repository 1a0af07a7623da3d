"""Inputs that uniform sampling never produces, for the scalar-field kernels, the device hash maps and the G1 kernels.

* `edge_elements`: field values at the ends of the field, at the limb and word boundaries, and the preimages of the stored words at
  which the load conversion of the quotient kernel and the circuit check (`to_rp`, csrc/zbound.cuh) changes its quotient estimate.
* `el_mix` / `el_hash` / `key_hash`: the hash of csrc/fr_io.cuh restated on Python integers (tests/test_fieldu.py holds it equal to
  the compiled functions), and builders of values that collide under it.
* `edge_points`: curve points with a coordinate at a base-field edge -- as a value, as the stored arkworks word, or as the signed
  30-bit limbs of the device's internal form (csrc/fields.cuh) -- for the G1 kernels; `edge_scalars` the scalars that go with them.

A "stored word" is the 256-bit integer a kernel reads from memory: the arkworks Montgomery form v = x * 2^256 mod r of the field
value x.  The maps hash and compare stored words, so the builders work on them; `field_value` takes one back to the x a test passes
through `fr_to_mont`.
"""
import random

import numpy as np

M64 = (1 << 64) - 1
MIX_C = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93)
MIX_F = 0xFF51AFD7ED558CCD
R256 = 1 << 256


# ---------------------------------------------------------------------------------------------------------------- the hash
def el_mix(h, v):
    """fr_io.cuh el_mix: h chained over the elements of a key, v one stored word"""
    for k in range(4):
        h ^= ((v >> (64 * k)) & M64) * MIX_C[k] & M64
    h ^= h >> 33
    h = h * MIX_F & M64
    h ^= h >> 29
    return h


def el_hash(v):
    """lookup.hip's slot hash of one element"""
    return el_mix(0, v) & 0xFFFFFFFF


def key_hash(vs):
    """check.hip's slot hash of a key of 1 or 4 elements"""
    h = 0
    for v in vs:
        h = el_mix(h, v)
    return (h ^ (h >> 32)) & 0xFFFFFFFF


def field_value(cv, v):
    """the field value whose stored word is v (v < r)"""
    assert 0 <= v < cv.r
    return v * pow(R256, -1, cv.r) % cv.r


def stored_word(cv, x):
    return x * R256 % cv.r


# ---------------------------------------------------------------------------------------------------------------- collisions
def colliding_partner(v, rng):
    """A stored word != v with el_mix(h, .) equal to v's for every h: words 2 and 3 kept, word 0 drawn, word 1 solved from
    w0 * C0 ^ w1 * C1 = w0' * C0 ^ w1' * C1 (C1 is odd, so invertible mod 2^64).  The top word is v's, so the partner is below
    2^252 whenever v is."""
    w0, w1 = v & M64, (v >> 64) & M64
    pre = (w0 * MIX_C[0] ^ w1 * MIX_C[1]) & M64
    while True:
        n0 = rng.getrandbits(64)
        if n0 == w0:
            continue
        n1 = ((pre ^ (n0 * MIX_C[0] & M64)) * pow(MIX_C[1], -1, 1 << 64)) & M64
        return (v >> 128 << 128) | (n1 << 64) | n0


def colliding_pair(rng):
    """Two distinct stored words with equal el_mix, the top 64-bit word below 2^60: canonical on both curves."""
    v = rng.getrandbits(252)
    return v, colliding_partner(v, rng)


def slot_cluster(mask, slot, count, hash, seed=0, exclude=()):
    """`count` distinct stored words below 2^252 with hash(v) & mask == slot, by seeded search.  `hash` maps a stored word to the
    32-bit hash of the key it stands in (el_hash for lookup.hip; for a wider key, a closure over the other elements)."""
    rng = random.Random(0x5107 * (seed + 1) + slot)
    out, seen = [], set(exclude)
    while len(out) < count:
        v = rng.getrandbits(252)
        if v not in seen and hash(v) & mask == slot:
            out.append(v)
            seen.add(v)
    return out


# ---------------------------------------------------------------------------------------------------------------- edge values
def to_rp_boundary_words(r):
    """Stored words around which to_rp's arithmetic changes: the ends, the points where floor(32 v / r) steps (the true quotient) and
    the points where floor(32 v / 2^BITS) steps (the truncated top the estimate starts from)."""
    bits = r.bit_length()
    c = [0, 1, r - 1, r - 2]
    for k in range(1, 33):
        c += [-(-k * r // 32) + d for d in (-2, -1, 0, 1)]
    for j in range(32):
        c += [-(-j * (1 << bits) // 32) + d for d in (-1, 0, 1)]
    out = []
    for v in c:
        if 0 <= v < r and v not in out:
            out.append(v)
    return out


def edge_elements(cv):
    """Field values, distinct, in a fixed order."""
    r = cv.r
    bits = r.bit_length()
    xs = [0, 1, 2, 3, r - 1, r - 2, r - 3, (r - 1) // 2, (r + 1) // 2]
    for step in (29, 32, 64):
        for k in range(step, bits, step):
            xs += [1 << k, (1 << k) - 1]
    xs.append(sum(((1 << 29) - 1) << (29 * i) for i in range(9)) % r)
    xs += [field_value(cv, v) for v in to_rp_boundary_words(r)]
    out, seen = [], set()
    for x in xs:
        x %= r
        if x not in seen:
            out.append(x)
            seen.add(x)
    return out


def edge_column(cv, n, stride=1, start=0):
    """n values: the edge set walked with a stride (coprime strides give every column another alignment)"""
    e = edge_elements(cv)
    return [e[(start + stride * i) % len(e)] for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------- edge points
# Curve points one of whose coordinates is a base-field edge, in one of the three forms some piece of code looks at:
#   "value"    the coordinate x itself;
#   "stored"   x * R mod q, R = 2^384 / 2^256: the arkworks word that bases_to_internal, from_sat and to_sat read and write;
#   "internal" x * R' mod q in [0, q), R' = 2^(30 NL): its strict signed limbs (csrc/fields.cuh) are what canonical_lt2p stores and
#              what every madd loads.
# Both curves have a = 0 and q = 3 (mod 4), so y = (x^3 + b)^((q + 1) / 4) lifts about every second x: a point with a chosen
# coordinate is a short walk away from any target.  On BLS12-381 such a point is on the curve but outside the r-torsion subgroup
# (the cofactor is not 1): see tests/test_edge_points_gpu.py for what that allows.
FS_LIMBS = {0: 13, 1: 9}        # NL of csrc/fields.cuh per curve id; tests/test_fieldu.py holds it equal to the compiled value
H29 = 1 << 29
MAX_WALK = 32                   # a walk is a few steps; tests/test_fieldu.py bounds and prints the largest


class EdgePoint(tuple):
    """(x, y) with the record of how it was found: form ("value" / "stored" / "internal"), side ("x" / "y" / "neg": the negation of
    an earlier point), target, dist (steps walked from the target) and, for a limb-pattern target, the pattern's limbs."""
    def __new__(cls, x, y, form, side, target, dist, pattern=None):
        p = super().__new__(cls, (x, y))
        p.form, p.side, p.target, p.dist, p.pattern = form, side, target, dist, pattern
        return p


def strict_limbs(v, nl):
    """fields.cuh's strict form of the integer v: limbs below the top one in [-2^29, 2^29), the top limb takes the rest"""
    out = []
    for _ in range(nl - 1):
        l = ((v + H29) & ((1 << 30) - 1)) - H29
        out.append(l)
        v = (v - l) >> 30
    return out + [v]


def limbs_value(limbs):
    return sum(l << (30 * i) for i, l in enumerate(limbs))


def form_factor(cv, form):
    """the factor f of a form: the form of x is x * f mod q"""
    return {"value": 1, "stored": cv.fq_R % cv.q, "internal": (1 << (30 * FS_LIMBS[cv.curve_id])) % cv.q}[form]


def fq_targets(q):
    """(target, walk direction): the ends of the field, its middle, and the limb (30) and word (32, 64) boundaries.  The walk leaves
    the boundary -- down from q - k and from 2^k - 1, up otherwise -- so that only the lowest limb or word moves."""
    out = [(t, 1) for t in (0, 1, 2, 3)] + [(q - k, -1) for k in (1, 2, 3)] + [((q - 1) // 2, 1), ((q + 1) // 2, 1)]
    for step in (30, 32, 64):
        for k in range(step, q.bit_length(), step):
            out += [(1 << k, 1), ((1 << k) - 1, -1)]
    seen, uniq = set(), []
    for t, d in out:
        if t not in seen:
            uniq.append((t, d))
            seen.add(t)
    return uniq


def internal_patterns(cv):
    """(limbs, walk direction): the low NL - 1 limbs all -2^29, all 2^29 - 1, or alternating in both phases, under a top limb of 0, 1
    or the modulus's top limb less one; the patterns whose value is in [0, q).  Down where limb 0 is at its upper end."""
    nl = FS_LIMBS[cv.curve_id]
    lo, hi = -H29, H29 - 1
    out = []
    for low in ([lo] * (nl - 1), [hi] * (nl - 1), [lo if i % 2 == 0 else hi for i in range(nl - 1)], [hi if i % 2 == 0 else lo for i in range(nl - 1)]):
        for top in (0, 1, (cv.q >> (30 * (nl - 1))) - 1):
            limbs = low + [top]
            if 0 <= limbs_value(limbs) < cv.q:
                out.append((limbs, -1 if low[0] == hi else 1))
    return out


def sqrt_3mod4(a, q):
    """the root the exponentiation returns, or None"""
    y = pow(a, (q + 1) // 4, q)
    return y if y * y % q == a % q else None


def cube_root(a, q):
    """one cube root of a mod q, or None; q = 1 (mod 3) with q - 1 = 3^s t: a^(1/3 mod t) is right up to an element of the 3-Sylow
    subgroup, which is small (s = 2 on both curves) and searched"""
    a %= q
    if a == 0:
        return 0
    if pow(a, (q - 1) // 3, q) != 1:
        return None
    s, t = 0, q - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    g = 2
    while pow(g, (q - 1) // 3, q) == 1:
        g += 1
    z = pow(g, t, q)                     # generates the 3-Sylow subgroup
    c = pow(a, pow(3, -1, t), q)
    for _ in range(3 ** s):
        if pow(c, 3, q) == a:
            return c
        c = c * z % q
    raise AssertionError("cube root search")


def _walk(cv, form, side, target, direction, pattern=None):
    """the first point whose `side` coordinate, in `form`, is target, target + direction, ...: (x, the lifted y) with x^3 + b a
    non-zero square for the x side, (a cube root of y^2 - b, y) with y != 0 for the y side"""
    q = cv.q
    inv = pow(form_factor(cv, form), -1, q)
    for dist in range(MAX_WALK):
        t = target + direction * dist
        if not 0 <= t < q:
            break
        c = t * inv % q
        if side == "x":
            rhs = (c * c * c + cv.b) % q
            y = sqrt_3mod4(rhs, q) if rhs else None
            if y is not None:
                return EdgePoint(c, y, form, side, target, dist, pattern)
        elif c:
            x = cube_root(c * c - cv.b, q)
            if x is not None:
                return EdgePoint(x, c, form, side, target, dist, pattern)
    raise AssertionError(f"no point within {MAX_WALK} steps of {form} {side} target {target:#x}")


_EDGE_POINTS = {}


def edge_points(cv):
    """Distinct affine points (x, y) as integers (EdgePoint: a tuple with its record), in a fixed order: every x target in the three
    forms, the limb patterns of the internal form, the negations (x, q - y) of the first dozen -- in strict limbs -(-2^29) = 2^29
    leaves the strict range -- and a handful of y targets.  y = 2 gives (0, 2) on BLS12-381: x = 0 on a real point (of order 3), next
    to the (0, 0) / (0, 1) encodings of infinity."""
    if cv.curve_id in _EDGE_POINTS:
        return _EDGE_POINTS[cv.curve_id]
    q = cv.q
    pts = []
    for form in ("value", "stored", "internal"):
        pts += [_walk(cv, form, "x", t, d) for t, d in fq_targets(q)]
    pats = internal_patterns(cv)
    pts += [_walk(cv, "internal", "x", limbs_value(l), d, l) for l, d in pats]
    pts += [EdgePoint(p[0], q - p[1], p.form, "neg", p.target, p.dist, p.pattern) for p in pts[:12]]
    for form in ("value", "stored", "internal"):
        pts += [_walk(cv, form, "y", t, d) for t, d in ((1, 1), (2, 1), (q - 1, -1), (q - 2, -1))]
    pts += [_walk(cv, "internal", "y", limbs_value(l), d, l) for l, d in pats if all(v == -H29 for v in l[:-1])]
    out, seen = [], set()
    for p in pts:
        if tuple(p) not in seen:
            out.append(p)
            seen.add(tuple(p))
    _EDGE_POINTS[cv.curve_id] = out
    return out


def points_to_limbs(cv, pts):
    """(n, 2L) uint64: x || y as arkworks Montgomery words; None (infinity) as all zero"""
    L = cv.fq_limbs
    out = np.zeros((len(pts), 2 * L), dtype=np.uint64)
    for i, p in enumerate(pts):
        if p is not None:
            for j, c in enumerate(p):
                out[i, j * L:(j + 1) * L] = np.frombuffer((c * cv.fq_R % cv.q).to_bytes(8 * L, "little"), dtype="<u8")
    return out


def edge_scalars(cv, n, top, stride=1, start=0, seed=0):
    """n scalars in [0, top]: 0, 1, top, then in turn an edge element (walked with a stride, taken mod top + 1: the ends of the
    scalar field land at the end of the range) and a seeded value.  top = r - 1 is the whole field; top = (r - 1) / 2 stays below
    the point at which the MSM folds k to (r - k)(-P), which only a point of order r allows."""
    e = edge_elements(cv)
    rng = random.Random(0xED6E + seed)
    out = [0, 1, top]
    for i in range(n):
        out.append(e[(start + stride * i) % len(e)] % (top + 1) if i % 2 == 0 else rng.randrange(top + 1))
    return out[:n]


def edge_msm_rows(cv, top, seed=0):
    """The MSM vector over the whole edge set, as (point or None, scalar in [0, top], infinity encoding) rows: every edge point
    under an edge_scalars value; mixed in as neighbours, a point next to its negation and a point three times, with equal scalars
    (top and 1 among them); (0, 2), of order 3, on BLS12-381 (G on BN254) with the scalars 1, 2, 3; and infinity in the three
    encodings of the ABI -- 1: the words (0, 0), 2: the words (0, 1), 3: the flag over a finite point's words (0: a finite point)."""
    pts = [tuple(e) for e in edge_points(cv)]
    m = len(pts)
    rng = random.Random(0xE06E + 16 * seed + cv.curve_id)
    rows = [(p, s, 0) for p, s in zip(pts, edge_scalars(cv, m, top, stride=7, start=1, seed=seed))]
    small = (0, 2) if cv.curve_id == 0 else (cv.gx, cv.gy)
    assert small in pts
    groups = [[(small, 1, 0), (small, 2, 0), (small, 3, 0)]]
    for j in range(8):
        p, s = pts[(11 * j + 5) % m], (rng.randrange(top + 1) if j else top)
        groups.append([(p, s, 0), ((p[0], cv.q - p[1]), s, 0)])
        p, s = pts[(13 * j + 2) % m], (rng.randrange(top + 1) if j else 1)
        groups.append([(p, s, 0)] * 3)
    groups += [[(None, rng.randrange(1, top + 1), 1 + j % 3)] for j in range(9)]
    rng.shuffle(groups)
    step = m // len(groups)
    at = 0
    for g in groups:
        rows[at:at] = g
        at += len(g) + step
    return rows


def rows_arrays(cv, rows):
    """-> (bases words (n, 2L), scalar limbs (n, 4), the flags the device is given, the flags an oracle that knows flags only is given)"""
    bases = points_to_limbs(cv, [p for p, _, _ in rows])
    one = points_to_limbs(cv, [(0, 1)])[0]
    filler = points_to_limbs(cv, [tuple(edge_points(cv)[3])])[0]
    for i, (_, _, enc) in enumerate(rows):
        if enc == 2:
            bases[i] = one
        elif enc == 3:
            bases[i] = filler
    scal = np.array([[(s >> (64 * k)) & M64 for k in range(4)] for _, s, _ in rows], dtype=np.uint64)
    return bases, scal, np.array([enc == 3 for _, _, enc in rows], dtype=np.uint8), np.array([enc != 0 for _, _, enc in rows], dtype=np.uint8)
