// The optimal ate pairing of BLS12-381 and BN254 with the G2 argument prepared: one definition for the host (a single KZG check,
// the latency-bound consumer) and for gfx950 device code (one check per lane, csrc/pairing.hip).
//
// Replaces (behind the C ABI) ark_ec::PairingEngine::product_of_pairings with ark-ec 0.3's G2Prepared, as kzg10::KZG10::check
// uses it (e(L, [tau]H) e(-R, H) = 1 with both G2 points fixed by the verifier key).
//
// Tower (arkworks' layout: c0.c0.c0, c0.c0.c1, c0.c1.c0, ... -- 12 Fq elements):
//   Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v), xi = XI0 + u (pairing_params.h).
// The Fq2 coefficient at slot (h, j) -- c[h] of Fq12, c[j] of Fq6 -- multiplies w^(h + 2j).
//
// A prepared G2 point is its Miller-loop line table: no G2 arithmetic runs where the pairing is evaluated.  With the affine step
// T + S of slope m on the twist, the line through the untwisted points, evaluated at P = (xP, yP) and scaled by a factor the final
// exponentiation removes, is
//   M-type twist (BLS12-381):  yP w^3 + (-m xP) w^2 + (m xT - yT)          slots (1,1), (0,1), (0,0)
//   D-type twist (BN254):      yP       + (-m xP) w   + (m xT - yT) w^3    slots (0,0), (1,0), (1,1)
// so a table entry is two Fq2 values (m xT - yT, -m), the same for both twists; which slots they land in is PP::TWIST_M, a
// constant of the curve.  The step kinds (bit 0: square and doubling line, bit 1: addition line) are data too: the loop below
// does not know the curve.
//
// Field type: the canonical Fp<FqP> of field.cuh on both sides, so every zero and equality test is exact.
//
// Device code size: an Fq12 value is 144 VGPRs on BLS12-381.  The tower's loops stay rolled and the Fq2 / Fq6 / Fq12 products are
// real calls on the device (ZK_PAIR_FN), with the Fq12 operands behind references (scratch memory); only Fq2 values travel in
// registers.
#pragma once
#include "field.cuh"
#include "pairing_params.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define ZK_PAIR_FN __host__ __device__ __noinline__
#elif defined(__HIPCC__)
#define ZK_PAIR_FN __host__ __device__ inline
#else
#define ZK_PAIR_FN inline
#endif

// the power c of the reference pairing (exponent (q^12 - 1) / r exactly) that final_exp computes: c is coprime to r
#define ZK_PAIRING_GT_POWER_BLS12_381 3      // the x-chain: (x - 1)^2 (x + q) (x^2 + q^2 - 1) + 3 = 3 (q^4 - q^2 + 1) / r
#define ZK_PAIRING_GT_POWER_BN254 1          // square-and-multiply over the digits of (q^4 - q^2 + 1) / r

template <class PP, class F>
struct Pairing {
    static constexpr int N = F::N;                    // 32-bit words of an Fq element
    static constexpr int LINE_WORDS = 4 * N;          // a table entry: two Fq2 values
    static constexpr int GT_POWER = PP::BN_TAIL ? ZK_PAIRING_GT_POWER_BN254 : ZK_PAIRING_GT_POWER_BLS12_381;

    struct Fq2 {
        F c0, c1;
    };
    struct Fq6 {
        Fq2 c[3];
    };
    struct Fq12 {
        Fq6 c[2];
    };

    ZK_HD static F load_fq(const uint32_t* p) {
        F r;
#pragma unroll
        for (int i = 0; i < N; ++i) r.v[i] = p[i];
        return r;
    }
    ZK_HD static void store_fq(uint32_t* p, const F& a) {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = a.v[i];
    }

    // ---- Fq2
    ZK_HD static Fq2 zero2() { return Fq2{F::zero(), F::zero()}; }
    ZK_HD static Fq2 one2() { return Fq2{F::one(), F::zero()}; }
    ZK_HD static Fq2 load2(const uint32_t* p) { return Fq2{load_fq(p), load_fq(p + N)}; }
    ZK_HD static bool is_zero2(const Fq2& a) { return a.c0.is_zero() && a.c1.is_zero(); }
    ZK_HD static bool eq2(const Fq2& a, const Fq2& b) { return a.c0 == b.c0 && a.c1 == b.c1; }
    ZK_HD static Fq2 add2(const Fq2& a, const Fq2& b) { return Fq2{F::add(a.c0, b.c0), F::add(a.c1, b.c1)}; }
    ZK_HD static Fq2 sub2(const Fq2& a, const Fq2& b) { return Fq2{F::sub(a.c0, b.c0), F::sub(a.c1, b.c1)}; }
    ZK_HD static Fq2 dbl2(const Fq2& a) { return Fq2{F::dbl(a.c0), F::dbl(a.c1)}; }
    ZK_HD static Fq2 neg2(const Fq2& a) { return Fq2{F::neg(a.c0), F::neg(a.c1)}; }
    ZK_HD static Fq2 conj2(const Fq2& a) { return Fq2{a.c0, F::neg(a.c1)}; }
    ZK_PAIR_FN static Fq2 mul2(const Fq2& a, const Fq2& b) {
        const F t0 = F::mul(a.c0, b.c0), t1 = F::mul(a.c1, b.c1);
        const F m = F::mul(F::add(a.c0, a.c1), F::add(b.c0, b.c1));
        return Fq2{F::sub(t0, t1), F::sub(F::sub(m, t0), t1)};
    }
    ZK_PAIR_FN static Fq2 sqr2(const Fq2& a) {
        const F p = F::mul(a.c0, a.c1);
        return Fq2{F::mul(F::add(a.c0, a.c1), F::sub(a.c0, a.c1)), F::dbl(p)};
    }
    ZK_PAIR_FN static Fq2 mul2_fq(const Fq2& a, const F& s) { return Fq2{F::mul(a.c0, s), F::mul(a.c1, s)}; }
    // a xi = (XI0 a0 - a1) + (XI0 a1 + a0) u
    ZK_HD static Fq2 mul2_xi(const Fq2& a) {
        static_assert(PP::XI0 == 1 || PP::XI0 == 9, "xi = 1 + u or 9 + u");
        if constexpr (PP::XI0 == 1) {
            return Fq2{F::sub(a.c0, a.c1), F::add(a.c0, a.c1)};
        } else {
            const Fq2 n = add2(dbl2(dbl2(dbl2(a))), a);              // 9 a
            return Fq2{F::sub(n.c0, a.c1), F::add(n.c1, a.c0)};
        }
    }
    // 1 / a = conj(a) / (a0^2 + a1^2); inv2(0) = 0
    ZK_PAIR_FN static Fq2 inv2(const Fq2& a) {
        const F d = F::inverse(F::add(F::sqr(a.c0), F::sqr(a.c1)));
        return Fq2{F::mul(a.c0, d), F::neg(F::mul(a.c1, d))};
    }

    // ---- Fq6.  Every function may be called with r aliasing an operand.
    ZK_HD static void add6(Fq6& r, const Fq6& a, const Fq6& b) {
#pragma unroll 1
        for (int i = 0; i < 3; ++i) r.c[i] = add2(a.c[i], b.c[i]);
    }
    ZK_HD static void sub6(Fq6& r, const Fq6& a, const Fq6& b) {
#pragma unroll 1
        for (int i = 0; i < 3; ++i) r.c[i] = sub2(a.c[i], b.c[i]);
    }
    ZK_HD static void neg6(Fq6& r, const Fq6& a) {
#pragma unroll 1
        for (int i = 0; i < 3; ++i) r.c[i] = neg2(a.c[i]);
    }
    // a v = (xi a2, a0, a1)
    ZK_HD static void mul6_v(Fq6& r, const Fq6& a) {
        const Fq2 t = mul2_xi(a.c[2]);
        r.c[2] = a.c[1];
        r.c[1] = a.c[0];
        r.c[0] = t;
    }
    ZK_PAIR_FN static void mul6(Fq6& r, const Fq6& a, const Fq6& b) {
        const Fq2 v0 = mul2(a.c[0], b.c[0]), v1 = mul2(a.c[1], b.c[1]), v2 = mul2(a.c[2], b.c[2]);
        const Fq2 m12 = mul2(add2(a.c[1], a.c[2]), add2(b.c[1], b.c[2]));
        const Fq2 m01 = mul2(add2(a.c[0], a.c[1]), add2(b.c[0], b.c[1]));
        const Fq2 m02 = mul2(add2(a.c[0], a.c[2]), add2(b.c[0], b.c[2]));
        r.c[0] = add2(v0, mul2_xi(sub2(sub2(m12, v1), v2)));
        r.c[1] = add2(sub2(sub2(m01, v0), v1), mul2_xi(v2));
        r.c[2] = add2(sub2(sub2(m02, v0), v2), v1);
    }
    // a (b0 + b1 v)
    ZK_PAIR_FN static void mul6_by_01(Fq6& r, const Fq6& a, const Fq2& b0, const Fq2& b1) {
        const Fq2 v0 = mul2(a.c[0], b0), v1 = mul2(a.c[1], b1);
        const Fq2 m12 = mul2(add2(a.c[1], a.c[2]), b1);
        const Fq2 m01 = mul2(add2(a.c[0], a.c[1]), add2(b0, b1));
        const Fq2 m02 = mul2(add2(a.c[0], a.c[2]), b0);
        r.c[0] = add2(v0, mul2_xi(sub2(m12, v1)));
        r.c[1] = sub2(sub2(m01, v0), v1);
        r.c[2] = add2(sub2(m02, v0), v1);
    }
    // a (b1 v)
    ZK_PAIR_FN static void mul6_by_1(Fq6& r, const Fq6& a, const Fq2& b1) {
        const Fq2 t = mul2_xi(mul2(a.c[2], b1));
        r.c[2] = mul2(a.c[1], b1);
        r.c[1] = mul2(a.c[0], b1);
        r.c[0] = t;
    }
    // a b0
    ZK_PAIR_FN static void mul6_by_0(Fq6& r, const Fq6& a, const Fq2& b0) {
#pragma unroll 1
        for (int i = 0; i < 3; ++i) r.c[i] = mul2(a.c[i], b0);
    }
    ZK_PAIR_FN static void inv6(Fq6& r, const Fq6& a) {
        const Fq2 t0 = sub2(sqr2(a.c[0]), mul2_xi(mul2(a.c[1], a.c[2])));
        const Fq2 t1 = sub2(mul2_xi(sqr2(a.c[2])), mul2(a.c[0], a.c[1]));
        const Fq2 t2 = sub2(sqr2(a.c[1]), mul2(a.c[0], a.c[2]));
        const Fq2 d = inv2(add2(mul2(a.c[0], t0), mul2_xi(add2(mul2(a.c[2], t1), mul2(a.c[1], t2)))));
        r.c[0] = mul2(t0, d);
        r.c[1] = mul2(t1, d);
        r.c[2] = mul2(t2, d);
    }

    // ---- Fq12.  r may alias an operand.
    ZK_HD static void one12(Fq12& r) {
#pragma unroll 1
        for (int h = 0; h < 2; ++h)
#pragma unroll 1
            for (int j = 0; j < 3; ++j) r.c[h].c[j] = zero2();
        r.c[0].c[0] = one2();
    }
    ZK_HD static bool is_one12(const Fq12& a) {
        bool ok = eq2(a.c[0].c[0], one2());
#pragma unroll 1
        for (int k = 1; k < 6; ++k) ok = ok && is_zero2(a.c[k / 3].c[k % 3]);
        return ok;
    }
    ZK_HD static void conj12(Fq12& r, const Fq12& a) {
        r.c[0] = a.c[0];
        neg6(r.c[1], a.c[1]);
    }
    ZK_PAIR_FN static void mul12(Fq12& r, const Fq12& a, const Fq12& b) {
        Fq6 v0, v1, s, t;
        mul6(v0, a.c[0], b.c[0]);
        mul6(v1, a.c[1], b.c[1]);
        add6(s, a.c[0], a.c[1]);
        add6(t, b.c[0], b.c[1]);
        mul6(s, s, t);
        sub6(s, s, v0);
        sub6(r.c[1], s, v1);
        mul6_v(v1, v1);
        add6(r.c[0], v0, v1);
    }
    // (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - p - v p + 2 p w,  p = a0 a1
    ZK_PAIR_FN static void sqr12(Fq12& r, const Fq12& a) {
        Fq6 p, s, t;
        mul6(p, a.c[0], a.c[1]);
        add6(s, a.c[0], a.c[1]);
        mul6_v(t, a.c[1]);
        add6(t, t, a.c[0]);
        mul6(s, s, t);
        sub6(s, s, p);
        add6(r.c[1], p, p);
        mul6_v(p, p);
        sub6(r.c[0], s, p);
    }
    // 1 / (a0 + a1 w) = (a0 - a1 w) / (a0^2 - v a1^2); inv12(0) = 0
    ZK_PAIR_FN static void inv12(Fq12& r, const Fq12& a) {
        Fq6 d, t;
        mul6(d, a.c[0], a.c[0]);
        mul6(t, a.c[1], a.c[1]);
        mul6_v(t, t);
        sub6(d, d, t);
        inv6(d, d);
        mul6(r.c[0], a.c[0], d);
        mul6(t, a.c[1], d);
        neg6(r.c[1], t);
    }
    // a^(q^POW), POW = 1 or 2: the coefficient c of w^k becomes conj^POW(c) xi^(k (q^POW - 1) / 6)
    template <int POW>
    ZK_PAIR_FN static void frobenius12(Fq12& r, const Fq12& a) {
        static_assert(POW == 1 || POW == 2, "Frobenius by q or q^2");
#pragma unroll 1
        for (int h = 0; h < 2; ++h)
#pragma unroll 1
            for (int j = 0; j < 3; ++j) {
                const int k = h + 2 * j;
                if constexpr (POW == 1) {
                    Fq2 g;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        g.c0.v[i] = PP::FROB1(k, i);
                        g.c1.v[i] = PP::FROB1(k, N + i);
                    }
                    r.c[h].c[j] = mul2(conj2(a.c[h].c[j]), g);
                } else {
                    F g;
#pragma unroll
                    for (int i = 0; i < N; ++i) g.v[i] = PP::FROB2(k, i);
                    r.c[h].c[j] = mul2_fq(a.c[h].c[j], g);
                }
            }
    }
    // a^2 for a in the cyclotomic subgroup (a^(q^4 - q^2 + 1) = 1), Granger-Scott: three Fq4 squarings
    ZK_PAIR_FN static void cyclotomic_sqr12(Fq12& r, const Fq12& a) {
        // the pairs (z0, z1), (z2, z3), (z4, z5) of Fq4 = Fq2[y]/(y^2 - xi): slots (0,0),(1,1) | (1,0),(0,2) | (0,1),(1,2)
        const Fq2 z0 = a.c[0].c[0], z4 = a.c[0].c[1], z3 = a.c[0].c[2], z2 = a.c[1].c[0], z1 = a.c[1].c[1], z5 = a.c[1].c[2];
        Fq2 tmp = mul2(z0, z1);
        const Fq2 t0 = sub2(sub2(mul2(add2(z0, z1), add2(mul2_xi(z1), z0)), tmp), mul2_xi(tmp));
        const Fq2 t1 = dbl2(tmp);
        tmp = mul2(z2, z3);
        const Fq2 t2 = sub2(sub2(mul2(add2(z2, z3), add2(mul2_xi(z3), z2)), tmp), mul2_xi(tmp));
        const Fq2 t3 = dbl2(tmp);
        tmp = mul2(z4, z5);
        const Fq2 t4 = sub2(sub2(mul2(add2(z4, z5), add2(mul2_xi(z5), z4)), tmp), mul2_xi(tmp));
        const Fq2 t5 = dbl2(tmp);
        r.c[0].c[0] = add2(dbl2(sub2(t0, z0)), t0);                 // 3 t0 - 2 z0
        r.c[1].c[1] = add2(dbl2(add2(t1, z1)), t1);                 // 3 t1 + 2 z1
        tmp = mul2_xi(t5);
        r.c[1].c[0] = add2(dbl2(add2(tmp, z2)), tmp);               // 3 xi t5 + 2 z2
        r.c[0].c[2] = add2(dbl2(sub2(t4, z3)), t4);                 // 3 t4 - 2 z3
        r.c[0].c[1] = add2(dbl2(sub2(t2, z4)), t2);                 // 3 t2 - 2 z4
        r.c[1].c[2] = add2(dbl2(add2(t3, z5)), t3);                 // 3 t3 + 2 z5
    }
    // a^e for a in the cyclotomic subgroup, e given as n little-endian 32-bit words (top word non-zero)
    ZK_PAIR_FN static void cyclotomic_pow12(Fq12& r, const Fq12& a, const uint32_t* e, int n) {
        Fq12 acc;
        one12(acc);
        bool started = false;
#pragma unroll 1
        for (int i = n - 1; i >= 0; --i)
#pragma unroll 1
            for (int b = 31; b >= 0; --b) {
                if (started) cyclotomic_sqr12(acc, acc);
                if ((e[i] >> b) & 1u) {
                    if (started) mul12(acc, acc, a);
                    else acc = a;
                    started = true;
                }
            }
        r = acc;
    }

    // ---- lines
    // f *= the line of one table entry at P = (px, py)
    ZK_PAIR_FN static void mul12_by_line(Fq12& f, const uint32_t* entry, const F& px, const F& py) {
        const Fq2 k = load2(entry);                                  // m xT - yT
        const Fq2 cx = mul2_fq(load2(entry + 2 * N), px);            // -m xP
        const Fq2 cy = Fq2{py, F::zero()};
        Fq6 t0, t1, s;
        add6(s, f.c[0], f.c[1]);
        if constexpr (PP::TWIST_M) {                                 // (k, cx, 0) + (0, cy, 0) w
            mul6_by_01(t0, f.c[0], k, cx);
            mul6_by_1(t1, f.c[1], cy);
            mul6_by_01(s, s, k, add2(cx, cy));
        } else {                                                     // (cy, 0, 0) + (cx, k, 0) w
            mul6_by_0(t0, f.c[0], cy);
            mul6_by_01(t1, f.c[1], cx, k);
            mul6_by_01(s, s, add2(cy, cx), k);
        }
        sub6(s, s, t0);
        sub6(f.c[1], s, t1);
        mul6_v(t1, t1);
        add6(f.c[0], t0, t1);
    }

    // One squaring chain for two pairs: f <- f^2 l_a(P_a) l_b(P_b) per step.  steps[s] bit 0: square, then one entry of each
    // table (the doubling line); bit 1: one more entry of each (the addition line).  A pair that is skipped (its G1 point is
    // infinity, or there is no second pair) contributes 1.
    ZK_PAIR_FN static void miller2(Fq12& f, const uint8_t* steps, int n_steps, const uint32_t* lines_a, const uint32_t* lines_b,
                                   const F& ax, const F& ay, bool skip_a, const F& bx, const F& by, bool skip_b) {
        one12(f);
        size_t at = 0;
#pragma unroll 1
        for (int s = 0; s < n_steps; ++s) {
            const uint32_t kind = steps[s];
#pragma unroll 1
            for (uint32_t bit = 1; bit <= 2; ++bit) {
                if (!(kind & bit)) continue;
                if (bit == 1) sqr12(f, f);
                if (!skip_a) mul12_by_line(f, lines_a + at, ax, ay);
                if (!skip_b) mul12_by_line(f, lines_b + at, bx, by);
                at += LINE_WORDS;
            }
        }
        if constexpr (PP::LOOP_NEG) conj12(f, f);
    }

    // a^|x|, conjugated where x < 0 (a in the cyclotomic subgroup, where the conjugate is the inverse): a^x
    ZK_HD static void exp_x(Fq12& r, const Fq12& a) {
        const uint32_t e[2] = {(uint32_t)PP::X_ABS, (uint32_t)(PP::X_ABS >> 32)};
        cyclotomic_pow12(r, a, e, 2);
        if constexpr (PP::LOOP_NEG) conj12(r, r);
    }
    // The hard part f^((q^4 - q^2 + 1) / r) by its digits (GENERIC: the power c = 1), or f^(3 (q^4 - q^2 + 1) / r) by the BLS12
    // chain (x - 1)^2 (x + q) (x^2 + q^2 - 1) + 3.  f is in the cyclotomic subgroup.
    template <bool GENERIC>
    ZK_PAIR_FN static void hard_part(Fq12& r, const Fq12& f) {
        if constexpr (GENERIC) {
            uint32_t e[PP::HARD_WORDS];
#pragma unroll 1
            for (int i = 0; i < PP::HARD_WORDS; ++i) e[i] = PP::HARD(i);
            cyclotomic_pow12(r, f, e, PP::HARD_WORDS);
        } else {
            Fq12 y, t, u;
            conj12(u, f);
            exp_x(y, f);
            mul12(y, y, u);                       // f^(x - 1)
            conj12(u, y);
            exp_x(t, y);
            mul12(y, t, u);                       // f^((x - 1)^2)
            exp_x(t, y);
            frobenius12<1>(u, y);
            mul12(y, t, u);                       // ... ^(x + q)
            exp_x(t, y);
            exp_x(t, t);
            frobenius12<2>(u, y);
            mul12(t, t, u);
            conj12(u, y);
            mul12(y, t, u);                       // ... ^(x^2 + q^2 - 1)
            cyclotomic_sqr12(t, f);
            mul12(t, t, f);
            mul12(r, y, t);                       // ... f^3
        }
    }
    // f^((q^6 - 1)(q^2 + 1)), then the hard part: ref^GT_POWER for ref the reduced pairing with the exponent (q^12 - 1) / r
    template <bool GENERIC = PP::BN_TAIL>
    ZK_PAIR_FN static void final_exp(Fq12& r, const Fq12& f) {
        Fq12 a, b;
        inv12(a, f);
        conj12(b, f);
        mul12(a, a, b);                           // f^(q^6 - 1)
        frobenius12<2>(b, a);
        mul12(a, a, b);                           // ... ^(q^2 + 1)
        hard_part<GENERIC>(r, a);
    }

    // A G1 point as the library writes it: infinity by flag, or as (0, 1) / (0, 0)
    ZK_HD static bool g1_is_inf(const F& x, const F& y, bool flag) {
        return flag || (x.is_zero() && (y.is_zero() || y == F::one()));
    }
    ZK_HD static void store12(uint32_t* out, const Fq12& a) {
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
            store_fq(out + (2 * k) * N, a.c[k / 3].c[k % 3].c0);
            store_fq(out + (2 * k + 1) * N, a.c[k / 3].c[k % 3].c1);
        }
    }
};
