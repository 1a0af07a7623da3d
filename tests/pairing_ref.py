"""An independent definition of the reduced ate pairing on Python integers, for tests/test_pairing.py and tests/golden/gen_pairing.py.

It shares nothing with csrc/pairing.cuh but the curve parameters:

* Fq12 is ONE polynomial ring Fq[w]/(w^12 - A w^6 + B): (A, B) = (2, 2) on BLS12-381 and (18, 82) on BN254 (from u = w^6 - xi0,
  u^2 = -1, xi0 = 1 / 9).  No tower, no Karatsuba: schoolbook products, inverses by Gaussian elimination on the multiplication matrix.
* G2 is untwisted into E(Fq12): (x', y') -> (x'/w^2, y'/w^3) on BLS12-381 (M-type twist), (x' w^2, y' w^3) on BN254 (D-type).
* Lines are affine chord-and-tangent lines of E(Fq12), evaluated at the G1 point; vertical lines are left out (they lie in a proper
  subfield).
* The final step is a plain pow(f, (q^12 - 1) // r).

The tower-to-polynomial map the library's outputs go through before they are compared (tower_to_poly): the Fq2 element a0 + a1 u at
tower slot (h, j) -- c_h of Fq12, c_j of Fq6 -- is the coefficient of w^(h + 2j), and u = w^6 - xi0.
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class RefCurve:
    name: str
    q: int
    r: int
    b: int                   # G1: y^2 = x^3 + b
    xi0: int                 # xi = xi0 + u
    m_type: bool             # the twist: y^2 = x^3 + b xi (M) or y^2 = x^3 + b / xi (D)
    loop: int                # Miller loop count: |x| (BLS12), 6x + 2 (BN)
    loop_neg: bool           # x < 0: the loop's value is inverted
    bn_tail: bool            # the two lines through pi(Q) and -pi^2(Q)
    g1: tuple
    g2: tuple                # ((x0, x1), (y0, y1)) on the twist

    @property
    def A(self):
        return 2 * self.xi0

    @property
    def B(self):
        return self.xi0 * self.xi0 + 1


BLS = RefCurve(
    "bls12_381",
    0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
    0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    4, 1, True, 0xd201000000010000, True, False,
    (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
     0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1),
    ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
      0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
     (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
      0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be)),
)
BN = RefCurve(
    "bn254",
    21888242871839275222246405745257275088696311157297823662689037894645226208583,
    21888242871839275222246405745257275088548364400416034343698204186575808495617,
    3, 9, False, 29793968203157093288, False, True,
    (1, 2),
    ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
      11559732032986387107991004021392285783925812861821192530917403151452391805634),
     (8495653923123431417604973247489272438418190587263600148770280649306958101930,
      4082367875863433681332203403145435568316851327593401208105741076214120093531)),
)
CURVES = {0: BLS, 1: BN, "bls12_381": BLS, "bn254": BN}


# ---- Fq12 = Fq[w] / (w^12 - A w^6 + B): a list of 12 integers, coefficient of w^k at index k
def f_one():
    return [1] + [0] * 11


def f_const(c, x):
    return [x % c.q] + [0] * 11


def f_add(c, a, b):
    return [(x + y) % c.q for x, y in zip(a, b)]


def f_sub(c, a, b):
    return [(x - y) % c.q for x, y in zip(a, b)]


def f_mul(c, a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):                # w^k = A w^(k-6) - B w^(k-12)
        v = t[k]
        t[k - 6] += c.A * v
        t[k - 12] -= c.B * v
    return [v % c.q for v in t[:12]]


def f_pow(c, a, e):
    r = f_one()
    for bit in bin(e)[2:]:
        r = f_mul(c, r, r)
        if bit == "1":
            r = f_mul(c, r, a)
    return r


def f_inv(c, a):
    """x with a x = 1: the 12 x 12 system whose column k is a w^k"""
    q = c.q
    wk = f_one()
    w = [0, 1] + [0] * 10
    cols = []
    for _ in range(12):
        cols.append(f_mul(c, a, wk))
        wk = f_mul(c, wk, w)
    m = [[cols[k][i] for k in range(12)] + [1 if i == 0 else 0] for i in range(12)]
    for col in range(12):
        piv = next(i for i in range(col, 12) if m[i][col])
        m[col], m[piv] = m[piv], m[col]
        inv = pow(m[col][col], -1, q)
        m[col] = [v * inv % q for v in m[col]]
        for i in range(12):
            if i != col and m[i][col]:
                k = m[i][col]
                m[i] = [(x - k * y) % q for x, y in zip(m[i], m[col])]
    return [m[i][12] for i in range(12)]


def fq2_to_poly(c, a0, a1, k):
    """(a0 + a1 u) w^k, k < 6"""
    out = [0] * 12
    out[k] = (a0 - c.xi0 * a1) % c.q
    out[k + 6] = a1 % c.q
    return out


def tower_to_poly(c, coeffs):
    """12 integers in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...) -> the polynomial basis"""
    out = [0] * 12
    for h in range(2):
        for j in range(3):
            a0, a1 = coeffs[6 * h + 2 * j], coeffs[6 * h + 2 * j + 1]
            out = f_add(c, out, fq2_to_poly(c, a0, a1, h + 2 * j))
    return out


# ---- Fq2 on integer pairs, for the twist only (g2_mul, on_twist): (a0, a1) = a0 + a1 u
def fq2_mul(c, a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % c.q, (a[0] * b[1] + a[1] * b[0]) % c.q)


def fq2_inv(c, a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, c.q)
    return (a[0] * d % c.q, -a[1] * d % c.q)


def twist_b(c):
    xi = (c.xi0, 1)
    return fq2_mul(c, (c.b, 0), xi if c.m_type else fq2_inv(c, xi))


def on_twist(c, pt):
    x, y = pt
    x3 = fq2_mul(c, fq2_mul(c, x, x), x)
    b = twist_b(c)
    return fq2_mul(c, y, y) == ((x3[0] + b[0]) % c.q, (x3[1] + b[1]) % c.q)


def g2_add(c, p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    q = c.q
    if x1 == x2:
        if ((y1[0] + y2[0]) % q, (y1[1] + y2[1]) % q) == (0, 0):
            return None
        xx = fq2_mul(c, x1, x1)
        lam = fq2_mul(c, (3 * xx[0] % q, 3 * xx[1] % q), fq2_inv(c, (2 * y1[0] % q, 2 * y1[1] % q)))
    else:
        lam = fq2_mul(c, ((y2[0] - y1[0]) % q, (y2[1] - y1[1]) % q), fq2_inv(c, ((x2[0] - x1[0]) % q, (x2[1] - x1[1]) % q)))
    l2 = fq2_mul(c, lam, lam)
    x3 = ((l2[0] - x1[0] - x2[0]) % q, (l2[1] - x1[1] - x2[1]) % q)
    t = fq2_mul(c, lam, ((x1[0] - x3[0]) % q, (x1[1] - x3[1]) % q))
    return x3, ((t[0] - y1[0]) % q, (t[1] - y1[1]) % q)


def g2_mul(c, k, pt=None, reduce=True):
    """k * pt on the twist (pt = the generator by default); reduce=False keeps k as it is (order tests of points outside G2)"""
    pt = c.g2 if pt is None else pt
    if reduce:
        k %= c.r
    acc = None
    while k:
        if k & 1:
            acc = g2_add(c, acc, pt)
        pt = g2_add(c, pt, pt)
        k >>= 1
    return acc


def g1_add(c, p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    q = c.q
    if x1 == x2:
        if (y1 + y2) % q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, q) % q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, q) % q
    x3 = (lam * lam - x1 - x2) % q
    return x3, (lam * (x1 - x3) - y1) % q


def g1_mul(c, k, pt=None, reduce=True):
    """k * pt on the curve (pt = the generator by default); reduce=False keeps k as it is (points of the curve outside G1)"""
    pt = c.g1 if pt is None else pt
    if reduce:
        k %= c.r
    acc = None
    while k:
        if k & 1:
            acc = g1_add(c, acc, pt)
        pt = g1_add(c, pt, pt)
        k >>= 1
    return acc


# ---- E(Fq12): y^2 = x^3 + b
def untwist(c, pt):
    (x0, x1), (y0, y1) = pt
    if c.m_type:            # x'/w^2 = x' w^4 / xi, y'/w^3 = y' w^3 / xi
        xi_inv = fq2_inv(c, (c.xi0, 1))
        xs, ys = fq2_mul(c, (x0, x1), xi_inv), fq2_mul(c, (y0, y1), xi_inv)
        return fq2_to_poly(c, xs[0], xs[1], 4), fq2_to_poly(c, ys[0], ys[1], 3)
    return fq2_to_poly(c, x0, x1, 2), fq2_to_poly(c, y0, y1, 3)


def on_curve12(c, pt):
    x, y = pt
    return f_mul(c, y, y) == f_add(c, f_mul(c, f_mul(c, x, x), x), f_const(c, c.b))


def _step(c, t, s, px, py):
    """(t + s, the line through t and s at (px, py)); t != -s"""
    (x1, y1), (x2, y2) = t, s
    if x1 == x2 and y1 == y2:
        xx = f_mul(c, x1, x1)
        lam = f_mul(c, f_add(c, f_add(c, xx, xx), xx), f_inv(c, f_add(c, y1, y1)))
    else:
        lam = f_mul(c, f_sub(c, y2, y1), f_inv(c, f_sub(c, x2, x1)))
    x3 = f_sub(c, f_sub(c, f_mul(c, lam, lam), x1), x2)
    y3 = f_sub(c, f_mul(c, lam, f_sub(c, x1, x3)), y1)
    line = f_sub(c, f_sub(c, f_const(c, py), y1), f_mul(c, lam, f_sub(c, f_const(c, px), x1)))
    return (x3, y3), line


def miller(c, p, q2):
    """f_{loop, Q}(P) (times the BN tail lines), inverted where x < 0; p in G1 affine, q2 on the twist; 1 if either is infinity"""
    if p is None or q2 is None:
        return f_one()
    px, py = p
    qq = untwist(c, q2)
    assert on_curve12(c, qq)
    t, f = qq, f_one()
    for bit in bin(c.loop)[3:]:
        t, line = _step(c, t, t, px, py)
        f = f_mul(c, f_mul(c, f, f), line)
        if bit == "1":
            t, line = _step(c, t, qq, px, py)
            f = f_mul(c, f, line)
    if c.bn_tail:
        q1 = (f_pow(c, qq[0], c.q), f_pow(c, qq[1], c.q))
        q2p = (f_pow(c, q1[0], c.q), f_pow(c, q1[1], c.q))
        q2n = (q2p[0], f_sub(c, [0] * 12, q2p[1]))
        t, line = _step(c, t, q1, px, py)
        f = f_mul(c, f, line)
        t, line = _step(c, t, q2n, px, py)
        f = f_mul(c, f, line)
    if c.loop_neg:
        f = f_inv(c, f)
    return f


def ref_pairing(c, p, q2):
    """the reduced pairing e(p, q2) = miller ^ ((q^12 - 1) / r), in the polynomial basis"""
    return f_pow(c, miller(c, p, q2), (c.q ** 12 - 1) // c.r)


def first_twist_point_outside_g2(c):
    """the first x = (i, 0), i = 1, 2, ..., with a point of the twist above it (either root): outside the r-torsion but for a
    negligible chance, which the caller asserts away"""
    q = c.q
    b = twist_b(c)
    i = 0
    while True:
        i += 1
        rhs = ((i * i * i + b[0]) % q, b[1])
        y = fq2_sqrt(c, rhs)
        if y is not None:
            return (i, 0), y


def fq2_sqrt(c, a):
    """a root of a in Fq2, or None (q = 3 mod 4: the norm method)"""
    q = c.q
    assert q % 4 == 3
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (q + 1) // 4, q)
        if s * s % q == a0:
            return (s, 0)
        s = pow(-a0 % q, (q + 1) // 4, q)          # a0 a non-residue: sqrt = s u
        return (0, s) if s * s % q == -a0 % q else None
    n = (a0 * a0 + a1 * a1) % q
    s = pow(n, (q + 1) // 4, q)
    if s * s % q != n:
        return None
    for sg in (s, -s):
        h = (a0 + sg) * pow(2, -1, q) % q
        x0 = pow(h, (q + 1) // 4, q)
        if x0 * x0 % q == h and x0:
            x1 = a1 * pow(2 * x0, -1, q) % q
            if fq2_mul(c, (x0, x1), (x0, x1)) == (a0 % q, a1 % q):
                return (x0, x1)
    return None
