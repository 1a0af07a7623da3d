"""Inputs that uniform sampling never produces, for the scalar-field kernels and the device hash maps.

* `edge_elements`: field values at the ends of the field, at the limb and word boundaries, and the preimages of the stored words at
  which the load conversion of the quotient kernel and the circuit check (`to_rp`, csrc/zbound.cuh) changes its quotient estimate.
* `el_mix` / `el_hash` / `key_hash`: the hash of csrc/fr_io.cuh restated on Python integers (tests/test_fieldu.py holds it equal to
  the compiled functions), and builders of values that collide under it.

A "stored word" is the 256-bit integer a kernel reads from memory: the arkworks Montgomery form v = x * 2^256 mod r of the field
value x.  The maps hash and compare stored words, so the builders work on them; `field_value` takes one back to the x a test passes
through `fr_to_mont`."""
import random

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
