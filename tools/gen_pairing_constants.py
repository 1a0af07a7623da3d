#!/usr/bin/env python3
"""Generate ark_plonk_amd/csrc/pairing_params.h: what the pairing of csrc/pairing.cuh needs beyond curve_params.h.

Every constant is computed here from the moduli, the curve parameter x and the non-residue xi = xi0 + u, never hand-typed (as
tools/gen_constants.py does for curve_params.h):

* FROB1(k): xi^(k (q - 1) / 6) in Fq2, FROB2(k): xi^(k (q^2 - 1) / 6) in Fq, k = 0..5 -- (a w^k)^q = conj(a) FROB1(k) w^k in
  Fq12 = Fq2[w] / (w^6 - xi);
* HARD: the 32-bit words of (q^4 - q^2 + 1) / r, the exponent of the final exponentiation's hard part;
* TWIST_B: the twist's constant, 4 xi (BLS12-381, M-type) and 3 / xi (BN254, D-type);
* the Miller loop count |x| (BLS12) or 6x + 2 (BN), whether x < 0, whether the two Frobenius lines follow.

Run:  python3 tools/gen_pairing_constants.py > ark_plonk_amd/csrc/pairing_params.h
"""

CURVES = [
    dict(name="Bls12_381",
         r=0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
         q=0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
         b=4, xi0=1, m_type=True, x_abs=0xd201000000010000, x_neg=True, bn=False),
    dict(name="Bn254",
         r=21888242871839275222246405745257275088548364400416034343698204186575808495617,
         q=21888242871839275222246405745257275088696311157297823662689037894645226208583,
         b=3, xi0=9, m_type=False, x_abs=4965661367192848881, x_neg=False, bn=True),
]


def limbs32(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def arr(vals):
    return ", ".join("0x%08xu" % v for v in vals)


def fq2_mul(q, a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)


def fq2_pow(q, a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = fq2_mul(q, r, r)
        if bit == "1":
            r = fq2_mul(q, r, a)
    return r


def fq2_inv(q, a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, q)
    return (a[0] * d % q, -a[1] * d % q)


def table(name, rows, width, comment):
    body = ",\n            ".join("{" + arr(r) + "}" for r in rows)
    return (f"    // {comment}\n"
            f"    ZK_HD static constexpr uint32_t {name}(int k, int i) {{\n"
            f"        constexpr uint32_t t[{len(rows)}][{width}] = {{\n            {body}}};\n"
            f"        return t[k][i];\n"
            f"    }}")


def curve_struct(c):
    q, r = c["q"], c["r"]
    n = (q.bit_length() + 31) // 32
    n += n % 2
    R = 1 << (32 * n)
    mont = lambda v: limbs32(v * R % q, n)
    xi = (c["xi0"], 1)
    assert (q - 1) % 6 == 0 and (q ** 4 - q * q + 1) % r == 0
    x = -c["x_abs"] if c["x_neg"] else c["x_abs"]
    if c["bn"]:
        assert q == 36 * x ** 4 + 36 * x ** 3 + 24 * x ** 2 + 6 * x + 1 and r == 36 * x ** 4 + 36 * x ** 3 + 18 * x ** 2 + 6 * x + 1
        loop = 6 * x + 2
    else:
        assert r == x ** 4 - x ** 2 + 1 and q == (x - 1) ** 2 * r // 3 + x
        loop = c["x_abs"]
    assert 0 < loop < 1 << 65
    f1 = [fq2_pow(q, xi, k * (q - 1) // 6) for k in range(6)]
    f2 = [fq2_pow(q, xi, k * (q * q - 1) // 6) for k in range(6)]
    assert all(v[1] == 0 for v in f2)
    hard = (q ** 4 - q * q + 1) // r
    nh = (hard.bit_length() + 31) // 32
    tb = fq2_mul(q, (c["b"], 0), xi if c["m_type"] else fq2_inv(q, xi))
    out = [f"struct Pairing{c['name']}Params {{"]
    out.append(f"    static constexpr bool TWIST_M = {'true' if c['m_type'] else 'false'};      // y^2 = x^3 + b xi (M) or x^3 + b / xi (D)")
    out.append(f"    static constexpr uint32_t XI0 = {c['xi0']};            // xi = XI0 + u")
    out.append(f"    static constexpr uint64_t LOOP_LO = 0x{loop & (2 ** 64 - 1):016x}ull;   // Miller loop count, low 64 bits")
    out.append(f"    static constexpr uint32_t LOOP_HI = {loop >> 64};         // ... and bit 64")
    out.append(f"    static constexpr bool LOOP_NEG = {'true' if c['x_neg'] else 'false'};     // x < 0: the loop's value is conjugated")
    out.append(f"    static constexpr bool BN_TAIL = {'true' if c['bn'] else 'false'};      // the lines through pi(Q) and -pi^2(Q)")
    out.append(f"    static constexpr uint64_t X_ABS = 0x{c['x_abs']:016x}ull;     // |x|")
    out.append(table("FROB1", [mont(v[0]) + mont(v[1]) for v in f1], 2 * n, "xi^(k (q - 1) / 6): c0 then c1, Montgomery"))
    out.append(table("FROB2", [mont(v[0]) for v in f2], n, "xi^(k (q^2 - 1) / 6), in Fq, Montgomery"))
    out.append(f"    static constexpr int HARD_WORDS = {nh};")
    out.append(f"    // (q^4 - q^2 + 1) / r, little-endian 32-bit words\n"
               f"    ZK_HD static constexpr uint32_t HARD(int i) {{\n"
               f"        constexpr uint32_t t[{nh}] = {{{arr(limbs32(hard, nh))}}};\n"
               f"        return t[i];\n    }}")
    out.append(f"    // the twist's constant: c0 then c1, Montgomery\n"
               f"    ZK_HD static constexpr uint32_t TWIST_B(int i) {{\n"
               f"        constexpr uint32_t t[{2 * n}] = {{{arr(mont(tb[0]) + mont(tb[1]))}}};\n"
               f"        return t[i];\n    }}")
    out.append("};")
    return "\n".join(out)


def main():
    print("// GENERATED by tools/gen_pairing_constants.py -- do not edit. All values derived from the moduli, x and xi.")
    print("#pragma once")
    print("#include <stdint.h>")
    print('#include "zk_common.h"')
    for c in CURVES:
        print()
        print(curve_struct(c))


if __name__ == "__main__":
    main()
