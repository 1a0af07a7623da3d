"""Curve ids and limb helpers of the host layer (product code; independent of oracle/)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class CurveInfo:
    name: str
    curve_id: int
    r: int
    q: int
    fq_limbs: int        # 64-bit limbs per Fq element
    two_adicity: int
    scalar_bits: int
    b: int = 0           # G1: y^2 = x^3 + b
    gx: int = 0          # the standard G1 generator (on the curve: tests/test_abi.py)
    gy: int = 0
    g2x: tuple = (0, 0)  # the standard G2 generator on the twist over Fq2 = Fq[u]/(u^2 + 1): (c0, c1) of x and of y
    g2y: tuple = (0, 0)  # (ark-bls12-381 / ark-bn254 g2.rs; on the twist and of order r: tests/test_pairing.py)


BLS12_381 = CurveInfo(
    "bls12_381", 0,
    0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
    6, 32, 255, 4,
    0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
    0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1,
    (0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
     0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
    (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
     0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be),
)
BN254 = CurveInfo(
    "bn254", 1,
    21888242871839275222246405745257275088548364400416034343698204186575808495617,
    21888242871839275222246405745257275088696311157297823662689037894645226208583,
    4, 28, 254, 3, 1, 2,
    (10857046999023057135944570762232829481370756359578518086990519993285655852781,
     11559732032986387107991004021392285783925812861821192530917403151452391805634),
    (8495653923123431417604973247489272438418190587263600148770280649306958101930,
     4082367875863433681332203403145435568316851327593401208105741076214120093531),
)

_BY_KEY = {0: BLS12_381, 1: BN254, "bls12_381": BLS12_381, "bn254": BN254, "bls12-381": BLS12_381}


def get_curve(c) -> CurveInfo:
    if isinstance(c, CurveInfo):
        return c
    try:
        return _BY_KEY[c]
    except KeyError:
        raise ValueError(f"unknown curve {c!r}")


def ints_to_limbs(vals, limbs: int) -> np.ndarray:
    """Python ints -> (len, limbs) little-endian uint64 array."""
    nbytes = limbs * 8
    buf = b"".join(int(v).to_bytes(nbytes, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, limbs).copy()


def limbs_to_ints(arr) -> list:
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    a = a.reshape(-1, a.shape[-1])
    nbytes = a.shape[1] * 8
    raw = a.astype("<u8").tobytes()
    return [int.from_bytes(raw[i * nbytes:(i + 1) * nbytes], "little") for i in range(a.shape[0])]


def fr_to_mont(curve, vals) -> np.ndarray:
    cv = get_curve(curve)
    R = 1 << 256
    return ints_to_limbs([(int(v) % cv.r) * R % cv.r for v in vals], 4)


def fr_from_mont(curve, arr) -> list:
    cv = get_curve(curve)
    rinv = pow(1 << 256, -1, cv.r)
    return [v * rinv % cv.r for v in limbs_to_ints(arr)]


def fq_to_mont(curve, vals) -> np.ndarray:
    cv = get_curve(curve)
    R = 1 << (64 * cv.fq_limbs)
    return ints_to_limbs([(int(v) % cv.q) * R % cv.q for v in vals], cv.fq_limbs)


def fq_from_mont(curve, arr) -> list:
    cv = get_curve(curve)
    rinv = pow(1 << (64 * cv.fq_limbs), -1, cv.q)
    return [v * rinv % cv.q for v in limbs_to_ints(arr)]


def g1_mul(curve, k: int):
    """k * G on y^2 = x^3 + b by affine double-and-add over Python integers: (x, y), or None for the point at infinity.  A few hundred
    modular inversions -- milliseconds; for checks of single results (bench.py's KZG identity), never on a compute path."""
    cv = get_curve(curve)
    q = cv.q
    k %= cv.r
    acc, add = None, (cv.gx, cv.gy)

    def plus(p1, p2):
        if p1 is None:
            return p2
        if p2 is None:
            return p1
        (x1, y1), (x2, y2) = p1, p2
        if x1 == x2:
            if (y1 + y2) % q == 0:
                return None
            lam = 3 * x1 * x1 * pow(2 * y1, -1, q) % q
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, q) % q
        x3 = (lam * lam - x1 - x2) % q
        return x3, (lam * (x1 - x3) - y1) % q

    while k:
        if k & 1:
            acc = plus(acc, add)
        add = plus(add, add)
        k >>= 1
    return acc


def g2_mul(curve, k: int):
    """k * H for the standard G2 generator H, on the twist over Fq2, by affine double-and-add over Python integers: ((x0, x1), (y0, y1)),
    or None for the point at infinity.  Like g1_mul: for keys of tests, tools and examples, never on a compute path."""
    cv = get_curve(curve)
    q = cv.q
    k %= cv.r

    def mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)

    def inv(a):
        d = pow(a[0] * a[0] + a[1] * a[1], -1, q)
        return (a[0] * d % q, -a[1] * d % q)

    def sub(a, b):
        return ((a[0] - b[0]) % q, (a[1] - b[1]) % q)

    def plus(p1, p2):
        if p1 is None:
            return p2
        if p2 is None:
            return p1
        (x1, y1), (x2, y2) = p1, p2
        if x1 == x2:
            if sub(y1, (0, 0)) == sub((0, 0), y2):
                return None
            xx = mul(x1, x1)
            lam = mul((3 * xx[0] % q, 3 * xx[1] % q), inv((2 * y1[0] % q, 2 * y1[1] % q)))
        else:
            lam = mul(sub(y2, y1), inv(sub(x2, x1)))
        x3 = sub(sub(mul(lam, lam), x1), x2)
        return x3, sub(mul(lam, sub(x1, x3)), y1)

    acc, add = None, (cv.g2x, cv.g2y)
    while k:
        if k & 1:
            acc = plus(acc, add)
        add = plus(add, add)
        k >>= 1
    return acc
