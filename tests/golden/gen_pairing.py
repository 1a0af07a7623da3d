"""Generates tests/golden/pairing_gt.json: values of the reduced pairing by the independent definition of tests/pairing_ref.py
(one polynomial ring for Fq12, G2 untwisted into E(Fq12), affine chord-and-tangent lines, a plain pow by (q^12 - 1) / r).

    python tests/golden/gen_pairing.py

For both curves: ref_pairing(a G, b H) for a handful of (a, b) -- (1, 1), (1, TAU) with the trapdoor of tests/conftest.py, a = r - 1,
and two pairs of larger scalars -- each as the 12 coefficients of w^0 .. w^11, hexadecimal.  The reference takes a fraction of a
second per pairing; the fixture exists so that the tests pin the library to values that were written down once, not to whatever the
reference computes on the day.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pairing_ref as pr  # noqa: E402

TAU = 0x7A5C0DE                                   # tests/conftest.py
OUT = os.path.join(HERE, "pairing_gt.json")


def cases(c):
    return [(1, 1), (1, TAU), (c.r - 1, 1), (5, 7), (0x1F2E3D4C5B6A79880123456789ABCDEF, 0xFEDCBA98765432100F1E2D3C4B5A6978 % c.r)]


def main():
    out = {"tau": TAU, "basis": "coefficients of w^0 .. w^11 in Fq[w]/(w^12 - A w^6 + B)"}
    for c in (pr.BLS, pr.BN):
        assert pr.on_twist(c, c.g2) and pr.g2_mul(c, c.r, reduce=False) is None
        rows = []
        for a, b in cases(c):
            e = pr.ref_pairing(c, pr.g1_mul(c, a), pr.g2_mul(c, b))
            assert e != pr.f_one() and pr.f_pow(c, e, c.r) == pr.f_one()
            rows.append({"a": hex(a), "b": hex(b), "gt": [hex(v) for v in e]})
        base = [int(v, 16) for v in rows[0]["gt"]]
        for row, (a, b) in zip(rows, cases(c)):                                      # bilinear in both arguments
            assert [int(v, 16) for v in row["gt"]] == pr.f_pow(c, base, a * b % c.r)
        out[c.name] = {"A": c.A, "B": c.B, "cases": rows}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
