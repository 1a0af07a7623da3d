"""Pure-Python restatement of ipa_pc's commit / open / check without hiding and degree bounds (the specification in
ark_plonk_amd/ipa.py), the checker of tests/test_ipa.py and tests/test_ipa_gpu.py.  The transcript is ark_plonk_amd.ipa.transcript_hash
itself: the one place that holds the (unpinned) encodings; everything else here is independent of the library.

Two groups behind the same protocol code:
  * Generic: real points and the big-int group law of oracle.bigint_oracle (for keys of up to a few hundred points);
  * KnownLog: test keys G_i = k_i G and h = k_h G with the k_i known -- a group element is its discrete logarithm, every MSM and fold
    is Fr arithmetic, and a point is computed (one ec_mul) only where the transcript or the proof needs one: C, L_j, R_j, the final key.
Both give byte-identical proofs for the same key (tests/test_ipa.py)."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ark_plonk_amd.ipa import IpaProof, check_poly_eval, transcript_hash  # noqa: E402
from oracle import bigint_oracle as bo  # noqa: E402


class Generic:
    def __init__(self, curve):
        self.cv = curve
        self.zero = None

    def point(self, e):
        return e

    def add(self, p, q):
        return bo.ec_add(self.cv, p, q)

    def mul(self, k, p):
        return bo.ec_mul(self.cv, k % self.cv.r, p)

    def msm(self, elems, scalars):
        acc = None
        for e, s in zip(elems, scalars):
            if s % self.cv.r:
                acc = bo.ec_add(self.cv, acc, bo.ec_mul(self.cv, s % self.cv.r, e))
        return acc

    def fold_key(self, kl, kr, xi):
        return [self.add(a, self.mul(xi, b)) for a, b in zip(kl, kr)]


class KnownLog:
    """A group element is its logarithm to the base G (mod r)."""

    def __init__(self, curve):
        self.cv = curve
        self.zero = 0
        self._pts = {}

    def point(self, e):
        e %= self.cv.r
        if e not in self._pts:
            self._pts[e] = bo.ec_mul(self.cv, e, (self.cv.gx, self.cv.gy))
        return self._pts[e]

    def add(self, p, q):
        return (p + q) % self.cv.r

    def mul(self, k, p):
        return k * p % self.cv.r

    def msm(self, elems, scalars):
        return sum(e * s for e, s in zip(elems, scalars)) % self.cv.r

    def fold_key(self, kl, kr, xi):
        r = self.cv.r
        return [(a + xi * b) % r for a, b in zip(kl, kr)]


def combine(curve, polys, chi, d1):
    r = curve.r
    p = [0] * d1
    for k, poly in enumerate(polys):
        ck = pow(chi, k, r)
        for i, c in enumerate(poly):
            p[i] = (p[i] + ck * c) % r
    return p


def commit(group, key, poly):
    return group.msm(key[:len(poly)], poly)


def open_(group, key, h, polys, comms, z, chi, digest):
    """ipa_pc::open (no hiding, no degree bounds): key / h / comms are group elements, polys canonical coefficient lists.
    Returns an IpaProof with points (affine integer tuples or None) -- whatever the group."""
    cv = group.cv
    r = cv.r
    d1 = len(key)
    a = combine(cv, polys, chi, d1)
    z %= r
    v = bo.horner(a, z, r)
    C = group.msm(comms, [pow(chi, k, r) for k in range(len(comms))])
    xi = transcript_hash(cv.name, digest, [("g1", group.point(C)), ("fr", z), ("fr", v)])
    hp = group.mul(xi, h)
    b = [pow(z, i, r) for i in range(d1)]
    k = list(key)
    proof = IpaProof()
    while len(a) > 1:
        m = len(a) // 2
        al, ar, bl, br, kl, kr = a[:m], a[m:], b[:m], b[m:], k[:m], k[m:]
        ip_l = sum(x * y for x, y in zip(ar, bl)) % r
        ip_r = sum(x * y for x, y in zip(al, br)) % r
        Lp = group.point(group.add(group.msm(kl, ar), group.mul(ip_l, hp)))
        Rp = group.point(group.add(group.msm(kr, al), group.mul(ip_r, hp)))
        proof.l_vec.append(Lp)
        proof.r_vec.append(Rp)
        xi = transcript_hash(cv.name, digest, [("fr", xi), ("g1", Lp), ("g1", Rp)])
        xinv = pow(xi, -1, r)
        a = [(x + xinv * y) % r for x, y in zip(al, ar)]
        b = [(x + xi * y) % r for x, y in zip(bl, br)]
        k = group.fold_key(kl, kr, xi)
    proof.final_comm_key = group.point(k[0])
    proof.c = a[0]
    return proof


def check(group, key, h, comms, z, values, proof, chi, digest):
    """ipa_pc::check of one opening: the succinct check, then final_comm_key == MSM(comm_key, s).  Proof points are affine tuples;
    in the KnownLog group they are compared through their logarithms' points."""
    cv = group.cv
    r = cv.r
    d1 = len(key)
    log_d = d1.bit_length() - 1
    if len(proof.l_vec) != log_d or len(proof.r_vec) != log_d:
        return False
    z %= r
    C = group.msm(comms, [pow(chi, k, r) for k in range(len(comms))])
    v = sum(pow(chi, k, r) * x for k, x in enumerate(values)) % r
    xi = transcript_hash(cv.name, digest, [("g1", group.point(C)), ("fr", z), ("fr", v)])
    hp = group.mul(xi, h)
    xis = []
    for Lp, Rp in zip(proof.l_vec, proof.r_vec):
        xi = transcript_hash(cv.name, digest, [("fr", xi), ("g1", Lp), ("g1", Rp)])
        xis.append(xi)
    # the proof's points are real points: the succinct check runs on them with the big-int group law in either mode
    G = Generic(cv)
    lhs = G.add(group.point(C), G.mul(v, group.point(hp)))
    for x, Lp, Rp in zip(xis, proof.l_vec, proof.r_vec):
        lhs = G.add(lhs, G.add(G.mul(pow(x, -1, r), Lp), G.mul(x, Rp)))
    sz = check_poly_eval(cv.name, log_d, xis, z)
    rhs = G.add(G.mul(proof.c, proof.final_comm_key), G.mul(proof.c * sz % r, group.point(hp)))
    if lhs != rhs:
        return False
    s = check_coeffs(r, log_d, xis)
    return group.point(group.msm(key, s)) == proof.final_comm_key


def check_coeffs(r, log_d, xis):
    """s_k = product of xi_j over the bits (log_d - 1 - j) set in k."""
    s = [1]
    for j in range(log_d - 1, -1, -1):
        s = s + [x * xis[j] % r for x in s]
    return s
