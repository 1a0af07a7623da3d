"""The IPA opening of tests/ipa_oracle.py cut at the seams of the C ABI (zk_ipa_round_dev / zk_ipa_fold_dev / zk_ipa_powers_dev,
include/ark_plonk_amd.h), on Python integers: the checker of tests/test_ipa_steps_gpu.py, itself checked against ipa_oracle.open_ by
tests/test_ipa_steps_ref.py.  A helper, no test.

    st = Steps(io.KnownLog(cv))            # a group element is its logarithm; Steps(io.Generic(cv)) walks real points
    L, R = st.round_(a, b, key, hp)        # one round over vectors of length 2m = len(a): group elements (logarithms)
    a, b, key = st.fold(a, b, key, xi)     # the challenge applied: vectors and key of length m
    b = st.powers(z, n)                    # z^i, i < n, with 0^0 = 1

Unlike open_, b is ANY vector (not only the powers of a point), the key may be longer than the vectors (a first round over the
first 2m points reads key[0 .. 2m) only) and every challenge is the caller's.  `walk` composes the steps under a list of challenges or
under a rule that derives each from the round's (L, R), which is how open_ is reproduced."""
from __future__ import annotations

import ipa_oracle as io


class Steps:
    def __init__(self, group):
        self.g = group
        self.r = group.cv.r

    def powers(self, z, n):
        out, p = [], 1
        for _ in range(n):
            out.append(p)
            p = p * z % self.r
        return out

    def round_(self, a, b, key_logs, hp_log):
        """(L, R) = (MSM(key_l, a_r) + <a_r, b_l> h', MSM(key_r, a_l) + <a_l, b_r> h') over key_logs[0 .. len(a))"""
        g, r = self.g, self.r
        m = len(a) // 2
        assert len(a) == len(b) == 2 * m and len(key_logs) >= 2 * m
        al, ar, bl, br = a[:m], a[m:], b[:m], b[m:2 * m]
        kl, kr = key_logs[:m], key_logs[m:2 * m]
        ip_l = sum(x * y for x, y in zip(ar, bl)) % r
        ip_r = sum(x * y for x, y in zip(al, br)) % r
        return g.add(g.msm(kl, ar), g.mul(ip_l, hp_log)), g.add(g.msm(kr, al), g.mul(ip_r, hp_log))

    def fold(self, a, b, key_logs, xi):
        """(a_l + xi^-1 a_r, b_l + xi b_r, key_l + xi key_r), each of length m = len(a) / 2; xi non-zero mod r"""
        r = self.r
        m = len(a) // 2
        assert len(a) == len(b) == 2 * m and len(key_logs) >= 2 * m and xi % r
        xinv = pow(xi, -1, r)
        a2 = [(x + xinv * y) % r for x, y in zip(a[:m], a[m:])]
        b2 = [(x + xi * y) % r for x, y in zip(b[:m], b[m:])]
        return a2, b2, self.g.fold_key(key_logs[:m], key_logs[m:2 * m], xi)

    def walk(self, a, b, key_logs, hp_log, challenge):
        """Every call of an opening over vectors of length len(a) = 2^k, in ABI order.  challenge(j, Lpoint, Rpoint, state) gives round
        j's xi (state = (a, b, key) before the fold).  Returns a list of per-round records (L, R, xi, a', b', key'), L and R as points
        (affine integer tuples or None), and the last record's key'[0] and a'[0] are the final key (a group element) and c."""
        g = self.g
        a, b, key = list(a), list(b), list(key_logs[:len(a)])
        out = []
        j = 0
        while len(a) > 1:
            L, R = self.round_(a, b, key, hp_log)
            Lp, Rp = g.point(L), g.point(R)
            xi = challenge(j, Lp, Rp, (a, b, key))
            a, b, key = self.fold(a, b, key, xi)
            out.append((Lp, Rp, xi, a, b, key))
            j += 1
        return out


def open_by_steps(group, key, h, polys, comms, z, chi, digest):
    """ipa_oracle.open_ restated as: combine, first challenge, powers, then `walk` under transcript_hash"""
    cv = group.cv
    r = cv.r
    st = Steps(group)
    d1 = len(key)
    a = io.combine(cv, polys, chi, d1)
    z %= r
    v = io.bo.horner(a, z, r)
    C = group.msm(comms, [pow(chi, k, r) for k in range(len(comms))])
    xi0 = io.transcript_hash(cv.name, digest, [("g1", group.point(C)), ("fr", z), ("fr", v)])
    hp = group.mul(xi0, h)
    prev = [xi0]

    def challenge(j, Lp, Rp, state):
        prev[0] = io.transcript_hash(cv.name, digest, [("fr", prev[0]), ("g1", Lp), ("g1", Rp)])
        return prev[0]

    recs = st.walk(a, st.powers(z, d1), key, hp, challenge)
    proof = io.IpaProof()
    proof.l_vec = [rec[0] for rec in recs]
    proof.r_vec = [rec[1] for rec in recs]
    proof.final_comm_key = group.point(recs[-1][5][0] if recs else key[0])
    proof.c = recs[-1][3][0] if recs else a[0]
    return proof


def xi_to_infinity(r, kl, kr):
    """the challenge under which kl + xi kr is the point at infinity (logarithm 0)"""
    return -kl * pow(kr, -1, r) % r


def xi_to_doubling(r, kl, kr):
    """the challenge under which xi kr = kl: the fold's last addition adds a point to itself, the result is 2 kl"""
    return kl * pow(kr, -1, r) % r
