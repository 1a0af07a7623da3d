"""Generates tests/golden/pairing_edges.json: the reduced pairing, by the independent definition of tests/pairing_ref.py, of G1 inputs
whose coordinates are base-field edges, with H and with [TAU]H, and the verdicts of KZG check cases built from them.

    python tests/golden/gen_pairing_edges.py

The library's value is an algebraic function of (x, y) whether or not the point is on the curve or in the r-torsion, and so is
pairing_ref.miller: the fixture pins both sides at points uniform sampling never produces.  Per curve, in a fixed order:

* on-curve edge points: the points of edge_values.edge_points in the forms "value" (the coordinate itself) and "stored" (its
  Montgomery word, x * 2^(64 L) mod q) -- both sides, the negations included -- whose target is an end of the field (0 .. 3,
  q - 1 .. q - 3), its middle, or a 32- or 64-bit word boundary.  The 30-bit targets and the "internal" form belong to the signed
  30-bit limbs of the G1 kernels, which the pairing does not use.  (0, 2) on BLS12-381 is among them: a real point with x = 0.
  Size rule: a GT value is 12 coefficients, so a point costs 2.5 KB on BLS12-381; with every multiple of 32 bits the file would be
  about 350 KB.  Of the word boundaries 2^k, 2^k - 1 it therefore keeps the lowest (k = 32), the highest multiple of 32 below the
  bit length, and a 64-bit boundary in the middle (k = 192 on BLS12-381, 128 on BN254); every form and both sides are kept.
* off-curve extremes: (q-1, q-1), (0, q-1), (q-1, 0), (1, 0), (1/R, 1/R) and ((q-1)/R, (q-1)/R), R = 2^(64 L): the last two are the
  points whose stored words are 1 and q - 1.

Per point: x, y and ref_pairing with H and with [TAU]H (NOT raised to the library's GT_POWER), as in pairing_gt.json.  Per on-curve
point P four check cases (L, R) with the reference's verdict, [ e(L, [TAU]H) e(-R, H) == 1 ]:
  (P, TAU P)            the edge coordinates in L;
  (k P, P)              k = 1 / TAU modulo the order of the curve group (r on BN254, cofactor * r on BLS12-381): the edge
                        coordinates in R, whose y the check negates;
  and both with R.y replaced by q - R.y, which the reference must call invalid -- except where R pairs to one with everything, as
  the points (0, 2), (0, q - 2) of order 3 on BLS12-381 do: there the negated case is as valid as the other, and is recorded so.
On BN254 every curve point is in G1 and the first two must be valid; on BLS12-381 most edge points lie outside G1 and the verdict is
whatever the reference says (the count is printed).
"""
import json
import math
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edge_values as ev  # noqa: E402
import pairing_ref as pr  # noqa: E402

TAU = 0x7A5C0DE                                   # tests/conftest.py
OUT = os.path.join(HERE, "pairing_edges.json")
FQ_LIMBS = {"bls12_381": 6, "bn254": 4}
MIDDLE_BOUNDARY = {"bls12_381": 192, "bn254": 128}


def edge_curve(c):
    """what edge_values needs to know about a curve"""
    L = FQ_LIMBS[c.name]
    return SimpleNamespace(name=c.name, curve_id=0 if c is pr.BLS else 1, q=c.q, r=c.r, b=c.b, fq_limbs=L, fq_R=1 << (64 * L))


def curve_order(c):
    """#E(Fq) = q + 1 - t: t = x + 1 on BLS12 (x < 0 here), cofactor 1 on BN"""
    n = c.q + c.loop if c is pr.BLS else c.r
    assert n % c.r == 0 and pr.g1_mul(c, n, reduce=False) is None
    return n


def kept_targets(c):
    q = c.q
    bits = q.bit_length()
    out = {0, 1, 2, 3, q - 1, q - 2, q - 3, (q - 1) // 2, (q + 1) // 2}
    for k in (32, MIDDLE_BOUNDARY[c.name], (bits - 1) // 32 * 32):
        assert k % 32 == 0 and k < bits
        out |= {1 << k, (1 << k) - 1}
    return out


def point_list(c):
    """[(x, y, label, on_curve)] in the fixture's order"""
    cv = edge_curve(c)
    q = c.q
    keep = kept_targets(c)
    out = []
    for p in ev.edge_points(cv):
        if p.form in ("value", "stored") and p.target in keep:
            assert (p[1] * p[1] - p[0] ** 3 - c.b) % q == 0 and p[1] % q
            out.append((p[0], p[1], f"{p.form} {p.side} {p.target:#x}+{p.dist}", True))
    rinv = pow(cv.fq_R, -1, q)
    for x, y in ((q - 1, q - 1), (0, q - 1), (q - 1, 0), (1, 0), (rinv, rinv), ((q - 1) * rinv % q, (q - 1) * rinv % q)):
        assert (y * y - x ** 3 - c.b) % q != 0
        out.append((x, y, "off the curve", False))
    assert len({(x, y) for x, y, _, _ in out}) == len(out)
    if c is pr.BLS:
        assert (0, 2) in [(x, y) for x, y, _, _ in out]
    return out


_GT = {}


def ref_gt(c, p, which):
    """ref_pairing(p, which ? [TAU]H : H), each distinct input once"""
    key = (c.name, p, which)
    if key not in _GT:
        _GT[key] = pr.ref_pairing(c, p, pr.g2_mul(c, TAU) if which else c.g2)
    return _GT[key]


def ref_verdict(c, L, R):
    """[ e(L, [TAU]H) e(-R, H) == 1 ] as the product of two values of the reference"""
    return pr.f_mul(c, ref_gt(c, L, 1), ref_gt(c, (R[0], -R[1] % c.q), 0)) == pr.f_one()


def check_cases(c, i, p, order):
    """the four check cases of the on-curve point p (the fixture's i-th point)"""
    k = pow(TAU, -1, order)
    tp, kp = pr.g1_mul(c, TAU, p), pr.g1_mul(c, k, p, reduce=False)
    assert pr.g1_mul(c, order, p, reduce=False) is None and tp is not None and kp is not None
    assert pr.g1_mul(c, TAU, kp) == p
    rows = []
    for edge_in, (L, R) in (("L", (p, tp)), ("R", (kp, p))):
        for negated in (False, True):
            if negated:
                R = (R[0], c.q - R[1])
            rows.append({"point": i, "edge_in": edge_in, "r_negated": negated, "L": [hex(v) for v in L], "R": [hex(v) for v in R],
                         "valid": ref_verdict(c, L, R)})
    return rows


def main():
    out = {"tau": TAU, "basis": "coefficients of w^0 .. w^11 in Fq[w]/(w^12 - A w^6 + B)"}
    for c in (pr.BLS, pr.BN):
        order = curve_order(c)
        assert math.gcd(TAU, order) == 1
        pts = point_list(c)
        points, checks = [], []
        for i, (x, y, label, on_curve) in enumerate(pts):
            points.append({"x": hex(x), "y": hex(y), "what": label, "on_curve": on_curve,
                           "gt_h": [hex(v) for v in ref_gt(c, (x, y), 0)], "gt_tau_h": [hex(v) for v in ref_gt(c, (x, y), 1)]})
            if on_curve:
                checks += check_cases(c, i, (x, y), order)
        degenerate = 0
        for row in checks:
            if c is pr.BN:
                assert row["valid"] == (not row["r_negated"]), row
            elif row["r_negated"] and row["valid"]:
                # the reference decides: a negated case can only be valid where R pairs to one with H (e(R, H)^2 = 1 in a group of
                # odd order), which (0, 2) and (0, q - 2), of order 3, do -- every pairing of theirs is one
                R = tuple(int(v, 16) for v in row["R"])
                assert ref_gt(c, R, 0) == pr.f_one() and R[0] == 0, row
                degenerate += 1
        valid = sum(row["valid"] for row in checks if not row["r_negated"])
        print(f"{c.name}: {len(points)} points ({sum(p['on_curve'] for p in points)} on the curve), {len(checks)} check cases, "
              f"{valid} of {len(checks) // 2} unnegated cases valid by the reference, {degenerate} negated cases valid (R of order 3)")
        out[c.name] = {"A": c.A, "B": c.B, "points": points, "checks": checks}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
