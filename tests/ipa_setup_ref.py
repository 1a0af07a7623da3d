"""The checker of the IPA key derivation (ark_plonk_amd/ipa.py, csrc/ipa_setup.hip, csrc/h2c.cuh): `ipa_pc::setup`'s rule on Python
integers -- hashlib for the digests, oracle.bigint_oracle's ec_mul / on_curve for the cofactor and the curve.  Of the library it imports
`generator_preimage` alone (the byte layout of what is hashed is an assumption stated there once, like ipa.transcript_hash) and restates
everything else: from_random_bytes, the candidate search, the cofactor, setup's and trim's index arithmetic.  It also counts what the
device's wave-local search is measured against: attempts and square roots per index."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ark_plonk_amd.ipa import generator_preimage  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402

COFACTOR = {0: 0x396c8c005555e1568c00aaab0000aaab, 1: 1}
HASHES = {"blake2s": hashlib.blake2s, "blake2b": hashlib.blake2b}
# statuses of include/ark_plonk_amd.h, restated
OK, BAD_FLAGS, X_NOT_REDUCED, NOT_ON_CURVE, NOT_IN_SUBGROUP, INF_FLAG_X_NONZERO, EXHAUSTED = range(7)
COMBOS = [(c, d) for c in ("bls12_381", "bn254") for d in ("blake2s", "blake2b")]


class NoPoint:
    """from_random_bytes returned None"""
    def __init__(self, status, roots):
        self.status, self.roots = status, roots


def from_random_bytes(curve, data: bytes):
    """(status, point, square roots taken): point (x, y), bo.INF for the infinity encoding, None when there is no point"""
    cv = bo.CURVES[curve]
    g = 8 * cv.fq_limbs
    buf = bytes(data[:g]) + bytes(g - min(len(data), g))
    inf_flag, greatest = (buf[-1] >> 6) & 1, (buf[-1] >> 7) & 1
    x = int.from_bytes(buf, "little") % (1 << cv.q.bit_length())
    if x >= cv.q:
        return X_NOT_REDUCED, None, 0
    if inf_flag and greatest:
        return BAD_FLAGS, None, 0
    if inf_flag:
        return (OK, bo.INF, 0) if x == 0 else (INF_FLAG_X_NONZERO, None, 0)
    a = (pow(x, 3, cv.q) + cv.b) % cv.q
    if pow(a, (cv.q - 1) // 2, cv.q) not in (0, 1):                 # Euler's criterion: one exponentiation on the device, the root itself
        return NOT_ON_CURVE, None, 1
    y = pow(a, (cv.q + 1) // 4, cv.q)
    assert y * y % cv.q == a
    lo, hi = min(y, cv.q - y), max(y, cv.q - y)
    p = (x, hi if greatest else lo)
    assert bo.on_curve(cv, p)
    return OK, p, 1


def clear_cofactor(curve, p):
    cv = bo.CURVES[curve]
    return bo.ec_mul(cv, COFACTOR[cv.curve_id], p)


def generator(curve, digest: str, i: int, max_tries: int = 0):
    """(status, generator | None, attempts, square roots) of index i; a null row (None) with EXHAUSTED after max_tries (0: 1024)"""
    cap = max_tries or 1024
    roots = 0
    for attempt in range(cap):
        st, p, k = from_random_bytes(curve, HASHES[digest](generator_preimage(i, None if attempt == 0 else attempt - 1)).digest())
        roots += k
        if st == OK:
            return OK, clear_cofactor(curve, p), attempt + 1, roots
    return EXHAUSTED, None, cap, roots


_CACHE = {}


def generators(curve, digest: str, first: int, n: int):
    """[(status, point, attempts, roots)] for first <= i < first + n with the default cap, computed once per index and shared"""
    out = []
    for i in range(first, first + n):
        key = (curve, digest, i)
        if key not in _CACHE:
            _CACHE[key] = generator(curve, digest, i)
        out.append(_CACHE[key])
    return out


def attempts_only(curve, digest: str, i: int):
    """(attempts, roots) of index i without the cofactor multiplication: microseconds, for counts over many indices"""
    roots = 0
    for attempt in range(1024):
        st, _, k = from_random_bytes(curve, HASHES[digest](generator_preimage(i, None if attempt == 0 else attempt - 1)).digest())
        roots += k
        if st == OK:
            return attempt + 1, roots
    raise AssertionError("1024 attempts")


def next_power_of_two(k: int) -> int:
    p = 1
    while p < k:
        p *= 2
    return p


def setup_layout(max_degree: int):
    """(d, number of generators, index of h, index of s): gens = sample_generators(d + 3); h = gens.pop(); s = gens.pop()"""
    d = next_power_of_two(max_degree + 1) - 1
    return d, d + 3, d + 2, d + 1


def trim_points(d: int, supported_degree: int):
    """points of the trimmed key, or None where trim is an error"""
    t = next_power_of_two(supported_degree + 1) - 1
    return None if t > d else t + 1


def compress(curve, p) -> str:
    """a point as compressed hex (ark-serialize: x little-endian, bit 7 of the last byte for the larger y, bit 6 for infinity)"""
    cv = bo.CURVES[curve]
    g = 8 * cv.fq_limbs
    if p is bo.INF:
        return (bytes(g - 1) + b"\x40").hex()
    b = bytearray(p[0].to_bytes(g, "little"))
    if p[1] > cv.q - p[1]:
        b[-1] |= 0x80
    return bytes(b).hex()
