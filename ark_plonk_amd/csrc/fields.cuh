// Signed 30-bit-limb Montgomery arithmetic for the MSM base field (the XYZZ group law of ecu.cuh / ecq.cuh).
//
// Why a second unsaturated form next to fieldu.cuh: msm_accumulate is bound by the issue rate of the 64-bit
// multiply-add, so the only way to make a mixed addition cheaper is fewer limb products.  With SIGNED limbs in
// [-2^29, 2^29) a product is below 2^58 in magnitude, a product-scanning column of 2*NL products (3*NL in dot2)
// still fits a signed 64-bit accumulator (checked per modulus by tools/gen_constants.py), and a limb carries 30
// bits instead of 29: BLS12-381 Fq takes 13 limbs instead of 14 (338 v_mad_i64_i32 per product instead of 392),
// BN254 Fq 9 instead of 10 (162 instead of 200).  Signed limbs also make subtraction limb-wise with no multiple
// of p added, and the Montgomery quotient digits balanced, so a product of operands below 12p in magnitude
// comes out in (-p, p): |a||b|/R' + p/2 with R' >= 512 p.
//
// Representation: value = sum v[i] * 2^(30 i), v[i] two's-complement in a uint32_t, Montgomery radix R' = 2^(30 NL).
//   "strict"  : v[i] in [-2^29, 2^29) for i < NL-1 (the top limb takes the rest) -- unique for a given integer;
//               what mul / sqr / dot2 / from_sat / canonical_lt2p return;
//   "almost"  : |v[i]| <= 2^29 + 2 -- what add / sub / dbl / add3 return (one carry step, no ripple).
// Inputs of mul / sqr / dot2: almost-balanced limbs, |value| < 12p.
// These preconditions, and the ones stated at each operator below, are restated once as a rule table in tests/native/fb_field.h (a
// field that checks them at every call); tests/test_fieldu.py holds each rule against big integers at the extreme of its precondition
// and runs the group law over that field, so a call site that leaves the contract fails there.
// A difference is a plain limb-wise difference and a negation a limb-wise negation: no multiple of p is added, so `sub` and `neg` are
// the only names.  The group law of ecu.cuh is written against this interface; the host instantiates it over the saturated Fp of
// field.cuh, which carries the same names with canonical values.
//
// Stands behind ark-ff 0.3 Fp384 / Fp256 arithmetic inside VariableBaseMSM (commitment.rs:45); arkworks-format
// values cross in / out through from_sat / to_sat.
#pragma once
#include "field_common.cuh"

// Fs<P> is the field every kernel and the host use.  Fs<P, true> is the same field, limb for limb and value for value, whose mul / sqr /
// dot2 are the chained products (mul_chain ...): the bucket accumulation (msm_accumulate.hip) instantiates its two kernels over it and
// nothing else does.  In the kernels that run the general doubling and addition in a loop (g1_fixed_base, ipa_fold_key, g1_decompress,
// msm_win_finish) the chained products spill registers; the plain ones do not (profiles/field_chains/notes.md section 4).
template <class P, bool CHAIN = false>
struct Fs {
    typedef P Params;
    static constexpr int NL = P::NL;
    static constexpr int SAT = P::SAT_WORDS;
    static constexpr uint32_t M = (1u << 30) - 1u;
    static constexpr int32_t H = 1 << 29;
    uint32_t v[NL];

    ZK_HD static int32_t sx(uint32_t x) { return (int32_t)(x << 2) >> 2; }   // low 30 bits, sign-extended
    // link(): one step of a column's chain in the chained products (see mul_chain).  On the device the partial sum is handed to an empty asm as an INPUT, which gives
    // it a second use: the optimiser re-associates a sum only through values used once, so every column stays ONE v_mad_i64_i32 chain
    // that starts from the carry of the column below.  Left alone, the optimiser forms the a*b products of a column as a chain of
    // their own and merges it with the carry and the m*p chain afterwards: two v_lshl_add_u64 per column.  The asm defines no
    // register on purpose: the partial sum passed through an asm OUTPUT (the form of Fu::mul_fenced) costs an s_nop in front of its
    // consumer, because the compiler's hazard rules assume that an asm's result is forwarded (profiles/field_chains/notes.md §2).
    ZK_HD static int64_t link(int64_t t) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : : "v"(t));
#endif
        return t;
    }
    // a value the optimiser knows nothing about (no known bits): an empty asm, no instruction
    ZK_HD static uint32_t opaque(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm("" : "+v"(x));
#endif
        return x;
    }
    // The bias 2^29 of the high-half columns, once per product.  On the device it is hidden from the optimiser in a scalar register
    // pair (an empty asm).  Plain products: it starts the column, and as a variable it can be the addend of the column's first
    // multiply-add (as a visible constant it is moved to the end of the sum and costs a 64-bit add per column).  Chained products: it
    // is added last, and as a visible constant it would be folded with the column's shift and mask at the price of multiply-adds
    // (profiles/field_chains/notes.md section 2).
    ZK_HD static int64_t column_bias() {
        int64_t h = H;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(h));
#endif
        return h;
    }
    // the end of a low-half column: the balanced quotient digit m_k makes the column a multiple of 2^30; returns the carry (exact shift)
    ZK_HD static int64_t finish_low(int64_t t, int32_t& mk) {
        mk = (int32_t)((uint32_t)t * (P::PINV << 2)) >> 2;      // (t * PINV mod 2^30), sign-extended: the shift rides in the constant
        return (t + (int64_t)mk * P::MOD(0)) >> 30;
    }
    // the end of a high-half column, three instructions: the balanced digit is the sign-extended low 30 bits of the column sum t (one
    // v_bfe_i32), and its carry (t - digit) / 2^30 is the floor shift of t + 2^29.  The digit is made opaque: a consumer that knows
    // it to be a sign extension is compiled to unsigned multiply-adds with corrections.
    ZK_HD static int64_t finish_high(int64_t t, int64_t hb, uint32_t& digit) {
        digit = opaque((uint32_t)sx((uint32_t)t));
        return (t + hb) >> 30;
    }

    ZK_HD static Fs zero() {
        Fs r;
#pragma unroll
        for (int i = 0; i < NL; ++i) r.v[i] = 0;
        return r;
    }
    ZK_HD static Fs one() {
        Fs r;
#pragma unroll
        for (int i = 0; i < NL; ++i) r.v[i] = (uint32_t)P::ONE(i);
        return r;
    }
    ZK_HD bool limbs_zero() const {
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < NL; ++i) o |= v[i];
        return o == 0;
    }

    // one carry step, every limb at once: a limb keeps its balanced low 30 bits and takes the carry of the limb
    // below (computed from that limb's value BEFORE the step).  |in| < 2^31 - 2^29 (sums and differences of TWO operands)
    // ->  |out| <= 2^29 + 2.
    ZK_HD static void normalize(Fs& t) {
        int32_t c = 0;
#pragma unroll
        for (int i = 0; i < NL - 1; ++i) {
            const int32_t x = (int32_t)t.v[i];
            const int32_t r = sx((uint32_t)x);
            t.v[i] = (uint32_t)(r + c);
            c = (x - r) >> 30;
        }
        t.v[NL - 1] += (uint32_t)c;
    }
    // the same step for limbs anywhere in int32 (sums of three or four operands): x - sx(x) can leave 32 bits there, so the
    // carry is taken as floor(x / 2^30) + bit 29 of x -- one instruction more per limb
    ZK_HD static void normalize_wide(Fs& t) {
        int32_t c = 0;
#pragma unroll
        for (int i = 0; i < NL - 1; ++i) {
            const int32_t x = (int32_t)t.v[i];
            t.v[i] = (uint32_t)(sx((uint32_t)x) + c);
            c = (x >> 30) + (int32_t)(((uint32_t)x >> 29) & 1u);
        }
        t.v[NL - 1] += (uint32_t)c;
    }
    // full ripple: strict limbs (unique representation)
    ZK_HD static void normalize_strict(Fs& t) {
#pragma unroll
        for (int i = 0; i < NL - 1; ++i) {
            const int32_t x = (int32_t)t.v[i];
            const int32_t r = sx((uint32_t)x);
            t.v[i] = (uint32_t)r;
            t.v[i + 1] += (uint32_t)((x - r) >> 30);
        }
    }

    ZK_HD static Fs add(const Fs& a, const Fs& b) {
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) t.v[i] = a.v[i] + b.v[i];
        normalize(t);
        return t;
    }
    ZK_HD static Fs dbl(const Fs& a) {
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) t.v[i] = a.v[i] << 1;
        normalize(t);
        return t;
    }
    ZK_HD static Fs add3(const Fs& a, const Fs& b, const Fs& c) {
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) t.v[i] = a.v[i] + b.v[i] + c.v[i];
        normalize_wide(t);
        return t;
    }
    ZK_HD static Fs sub(const Fs& a, const Fs& b) {
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) t.v[i] = a.v[i] - b.v[i];
        normalize(t);
        return t;
    }
    // a - (b + c + d) with one carry step.  Strict operands: a limb of the raw result is in [-2^31 + 3, 2^31 - 1].  What it needs, like
    // add3, is the raw limb sum inside int32 (one past it wraps: tests/test_fieldu.py shows both); negated strict operands still fit.
    ZK_HD static Fs sub_sum3(const Fs& a, const Fs& b, const Fs& c, const Fs& d) {
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) t.v[i] = a.v[i] - b.v[i] - c.v[i] - d.v[i];
        normalize_wide(t);
        return t;
    }
    ZK_HD static Fs neg(const Fs& a) {                    // limb-wise: stays almost balanced
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) t.v[i] = 0u - a.v[i];
        return t;
    }

    // Montgomery product a*b/R': interleaved product scanning, one signed 64-bit accumulator per column (the
    // compiler merges the three partial sums below into one v_mad_i64_i32 chain per column, two columns interleaved).
    // Low half: the balanced quotient digit m_k makes the column a multiple of 2^30 (exact shift).
    // High half: the column starts from the bias 2^29, so the floor shift is the carry of the BALANCED digit
    // (t + 2^29) mod 2^30 - 2^29.
    ZK_HD static Fs mul(const Fs& a, const Fs& b) {
        if constexpr (CHAIN) return mul_chain(a, b);
        int32_t m[NL];
        Fs r;
        int64_t carry = 0;
        const int64_t hb = column_bias();
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            int64_t a0 = 0, a1 = 0, am = 0;
#pragma unroll
            for (int i = 0; i <= k; ++i) {
                if (i & 1) a1 += (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i];
                else a0 += (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i];
            }
#pragma unroll
            for (int i = 0; i < k; ++i) am += (int64_t)m[i] * P::MOD(k - i);
            int64_t t = a0 + a1 + am + carry;
            m[k] = (int32_t)((uint32_t)t * (P::PINV << 2)) >> 2;      // (t * PINV mod 2^30), sign-extended: the shift rides in the constant
            t += (int64_t)m[k] * P::MOD(0);
            carry = t >> 30;
        }
#pragma unroll
        for (int k = NL; k < 2 * NL - 1; ++k) {
            int64_t a0 = hb, a1 = 0, am = 0;
#pragma unroll
            for (int i = k - NL + 1; i < NL; ++i) {
                if (i & 1) a1 += (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i];
                else a0 += (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i];
                am += (int64_t)m[i] * P::MOD(k - i);
            }
            const int64_t t = a0 + a1 + am + carry;
            r.v[k - NL] = ((uint32_t)t & M) - (uint32_t)H;
            carry = t >> 30;
        }
        r.v[NL - 1] = (uint32_t)carry;
        return r;
    }
    // The chained product (what mul is in Fs<P, true>): ONE signed 64-bit accumulator per column, no partial sums to merge.  A column's chain starts from
    // the carry of the column below plus the column's first product and takes every further a*b product and every m*p product in
    // turn (link); column 0 has no carry.  The sum of a column is the integer it always was -- the same terms of one 64-bit sum in
    // another order -- so the column bounds that tools/gen_constants.py and tests/test_fieldu.py check hold unchanged, and the host
    // compile (link, opaque and column_bias do nothing there) computes the same values as the device.
    // Low half: finish_low.  High half: finish_high.
    ZK_HD static Fs mul_chain(const Fs& a, const Fs& b) {
        int32_t m[NL];
        Fs r;
        int64_t carry = 0;
        const int64_t hb = column_bias();
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            int64_t t = (int64_t)(int32_t)a.v[0] * (int32_t)b.v[k];
            if (k) t = link(carry + t);
#pragma unroll
            for (int i = 1; i <= k; ++i) t = link(t + (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i]);
#pragma unroll
            for (int i = 0; i < k; ++i) t = link(t + (int64_t)m[i] * P::MOD(k - i));
            carry = finish_low(t, m[k]);
        }
#pragma unroll
        for (int k = NL; k < 2 * NL - 1; ++k) {
            int64_t t = link(carry + (int64_t)(int32_t)a.v[k - NL + 1] * (int32_t)b.v[NL - 1]);
#pragma unroll
            for (int i = k - NL + 2; i < NL; ++i) t = link(t + (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i]);
#pragma unroll
            for (int i = k - NL + 1; i < NL; ++i) t = link(t + (int64_t)m[i] * P::MOD(k - i));
            carry = finish_high(t, hb, r.v[k - NL]);
        }
        r.v[NL - 1] = (uint32_t)carry;
        return r;
    }
    // (a*b + c*d)/R' with ONE Montgomery reduction, for |a||b| + |c||d| < 288 p^2 (all that four operands below 12p can give).  The
    // result is below (|a||b| + |c||d|)/R' + p/2 in magnitude: inside (-p, p) up to 256 p^2 at the R' >= 512 p every modulus has, and
    // up to the whole 288 p^2 at R' >= 576 p, which both moduli in use have (gen_constants.py asserts either); always in (-2p, 2p).
    ZK_HD static Fs dot2(const Fs& a, const Fs& b, const Fs& c, const Fs& d) {
        if constexpr (CHAIN) return dot2_chain(a, b, c, d);
        int32_t m[NL];
        Fs r;
        int64_t carry = 0;
        const int64_t hb = column_bias();
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            int64_t a0 = 0, a1 = 0, am = 0;
#pragma unroll
            for (int i = 0; i <= k; ++i) {
                a0 += (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i];
                a1 += (int64_t)(int32_t)c.v[i] * (int32_t)d.v[k - i];
            }
#pragma unroll
            for (int i = 0; i < k; ++i) am += (int64_t)m[i] * P::MOD(k - i);
            int64_t t = a0 + a1 + am + carry;
            m[k] = (int32_t)((uint32_t)t * (P::PINV << 2)) >> 2;      // (t * PINV mod 2^30), sign-extended: the shift rides in the constant
            t += (int64_t)m[k] * P::MOD(0);
            carry = t >> 30;
        }
#pragma unroll
        for (int k = NL; k < 2 * NL - 1; ++k) {
            int64_t a0 = hb, a1 = 0, am = 0;
#pragma unroll
            for (int i = k - NL + 1; i < NL; ++i) {
                a0 += (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i];
                a1 += (int64_t)(int32_t)c.v[i] * (int32_t)d.v[k - i];
                am += (int64_t)m[i] * P::MOD(k - i);
            }
            const int64_t t = a0 + a1 + am + carry;
            r.v[k - NL] = ((uint32_t)t & M) - (uint32_t)H;
            carry = t >> 30;
        }
        r.v[NL - 1] = (uint32_t)carry;
        return r;
    }
    // chained: both products of a column's first index open its chain
    ZK_HD static Fs dot2_chain(const Fs& a, const Fs& b, const Fs& c, const Fs& d) {
        int32_t m[NL];
        Fs r;
        int64_t carry = 0;
        const int64_t hb = column_bias();
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            int64_t t = (int64_t)(int32_t)a.v[0] * (int32_t)b.v[k] + (int64_t)(int32_t)c.v[0] * (int32_t)d.v[k];
            if (k) t = link(carry + t);
#pragma unroll
            for (int i = 1; i <= k; ++i) {
                t = link(t + (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i]);
                t = link(t + (int64_t)(int32_t)c.v[i] * (int32_t)d.v[k - i]);
            }
#pragma unroll
            for (int i = 0; i < k; ++i) t = link(t + (int64_t)m[i] * P::MOD(k - i));
            carry = finish_low(t, m[k]);
        }
#pragma unroll
        for (int k = NL; k < 2 * NL - 1; ++k) {
            int64_t t = link(carry + (int64_t)(int32_t)a.v[k - NL + 1] * (int32_t)b.v[NL - 1]
                                      + (int64_t)(int32_t)c.v[k - NL + 1] * (int32_t)d.v[NL - 1]);
#pragma unroll
            for (int i = k - NL + 2; i < NL; ++i) {
                t = link(t + (int64_t)(int32_t)a.v[i] * (int32_t)b.v[k - i]);
                t = link(t + (int64_t)(int32_t)c.v[i] * (int32_t)d.v[k - i]);
            }
#pragma unroll
            for (int i = k - NL + 1; i < NL; ++i) t = link(t + (int64_t)m[i] * P::MOD(k - i));
            carry = finish_high(t, hb, r.v[k - NL]);
        }
        r.v[NL - 1] = (uint32_t)carry;
        return r;
    }
    // a*a/R': cross products once, against doubled limbs (|2 a_i| <= 2^30 + 4: the column bound is the one of mul)
    ZK_HD static Fs sqr(const Fs& a) {
        if constexpr (CHAIN) return sqr_chain(a);
        int32_t m[NL], a2[NL];
        Fs r;
#pragma unroll
        for (int i = 0; i < NL; ++i) a2[i] = (int32_t)(a.v[i] << 1);
        int64_t carry = 0;
        const int64_t hb = column_bias();
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            int64_t aa = 0, am = 0;
#pragma unroll
            for (int i = 0; 2 * i < k; ++i) aa += (int64_t)a2[i] * (int32_t)a.v[k - i];
            if ((k & 1) == 0) aa += (int64_t)(int32_t)a.v[k / 2] * (int32_t)a.v[k / 2];
#pragma unroll
            for (int i = 0; i < k; ++i) am += (int64_t)m[i] * P::MOD(k - i);
            int64_t t = aa + am + carry;
            m[k] = (int32_t)((uint32_t)t * (P::PINV << 2)) >> 2;      // (t * PINV mod 2^30), sign-extended: the shift rides in the constant
            t += (int64_t)m[k] * P::MOD(0);
            carry = t >> 30;
        }
#pragma unroll
        for (int k = NL; k < 2 * NL - 1; ++k) {
            int64_t aa = hb, am = 0;
#pragma unroll
            for (int i = k - NL + 1; 2 * i < k; ++i) aa += (int64_t)a2[i] * (int32_t)a.v[k - i];
            if ((k & 1) == 0) aa += (int64_t)(int32_t)a.v[k / 2] * (int32_t)a.v[k / 2];
#pragma unroll
            for (int i = k - NL + 1; i < NL; ++i) am += (int64_t)m[i] * P::MOD(k - i);
            const int64_t t = aa + am + carry;
            r.v[k - NL] = ((uint32_t)t & M) - (uint32_t)H;
            carry = t >> 30;
        }
        r.v[NL - 1] = (uint32_t)carry;
        return r;
    }
    // chained: a column's chain opens with its first cross product, or with the square term where it has no cross product (columns 0
    // and 2 NL - 2)
    ZK_HD static Fs sqr_chain(const Fs& a) {
        int32_t m[NL], a2[NL];
        Fs r;
#pragma unroll
        for (int i = 0; i < NL; ++i) a2[i] = (int32_t)(a.v[i] << 1);
        int64_t carry = 0;
        const int64_t hb = column_bias();
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            int64_t t = k ? link(carry + (int64_t)a2[0] * (int32_t)a.v[k]) : (int64_t)(int32_t)a.v[0] * (int32_t)a.v[0];
#pragma unroll
            for (int i = 1; 2 * i < k; ++i) t = link(t + (int64_t)a2[i] * (int32_t)a.v[k - i]);
            if (k && (k & 1) == 0) t = link(t + (int64_t)(int32_t)a.v[k / 2] * (int32_t)a.v[k / 2]);
#pragma unroll
            for (int i = 0; i < k; ++i) t = link(t + (int64_t)m[i] * P::MOD(k - i));
            carry = finish_low(t, m[k]);
        }
#pragma unroll
        for (int k = NL; k < 2 * NL - 1; ++k) {
            const int lo = k - NL + 1;
            int64_t t = link(carry + (2 * lo < k ? (int64_t)a2[lo] * (int32_t)a.v[k - lo] : (int64_t)(int32_t)a.v[lo] * (int32_t)a.v[lo]));
#pragma unroll
            for (int i = lo + 1; 2 * i < k; ++i) t = link(t + (int64_t)a2[i] * (int32_t)a.v[k - i]);
            if (2 * lo < k && (k & 1) == 0) t = link(t + (int64_t)(int32_t)a.v[k / 2] * (int32_t)a.v[k / 2]);
#pragma unroll
            for (int i = lo; i < NL; ++i) t = link(t + (int64_t)m[i] * P::MOD(k - i));
            carry = finish_high(t, hb, r.v[k - NL]);
        }
        r.v[NL - 1] = (uint32_t)carry;
        return r;
    }

    // necessary for is_zero_mod_reduced(): limb 0 is that of 0, p or -p (one in 2^30 values that are not zero pass it too)
    ZK_HD bool limb0_of_zero_mod() const { return v[0] == 0 || v[0] == (uint32_t)P::MOD(0) || v[0] == (uint32_t)P::NMOD(0); }
    // exact "== 0 mod p" for a mul / sqr / dot2 output: strict limbs, value in (-2p, 2p), so it is 0, p or -p
    ZK_HD bool is_zero_mod_reduced() const {
        if (v[0] != 0 && v[0] != (uint32_t)P::MOD(0) && v[0] != (uint32_t)P::NMOD(0)) return false;
        uint32_t dz = 0, dp = 0, dn = 0;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            dz |= v[i];
            dp |= v[i] ^ (uint32_t)P::MOD(i);
            dn |= v[i] ^ (uint32_t)P::NMOD(i);
        }
        return dz == 0 || dp == 0 || dn == 0;
    }
    // exact zero test for any lazily reduced value
    ZK_HD bool is_zero_mod() const { return mul(*this, one()).is_zero_mod_reduced(); }

    // limbs in [0, 2^30) below the top one (floor carries, full ripple): the sign of the value is the sign of the top limb
    ZK_HD static void floor_sweep(Fs& t) {
#pragma unroll
        for (int i = 0; i < NL - 1; ++i) {
            const int32_t x = (int32_t)t.v[i];
            t.v[i] = (uint32_t)x & M;
            t.v[i + 1] += (uint32_t)(x >> 30);
        }
    }
    // the representative in [0, p) of a value in (-2p, 2p), floor limbs
    ZK_HD static Fs canon_floor(const Fs& a) {
        Fs x = a;
        floor_sweep(x);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            Fs y;
#pragma unroll
            for (int i = 0; i < NL; ++i) y.v[i] = x.v[i] + (uint32_t)P::MOD(i);
            floor_sweep(y);
            const bool neg = (int32_t)x.v[NL - 1] < 0;
#pragma unroll
            for (int i = 0; i < NL; ++i) x.v[i] = neg ? y.v[i] : x.v[i];
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            Fs y;
#pragma unroll
            for (int i = 0; i < NL; ++i) y.v[i] = x.v[i] - (uint32_t)P::MOD(i);
            floor_sweep(y);
            const bool ge = (int32_t)y.v[NL - 1] >= 0;
#pragma unroll
            for (int i = 0; i < NL; ++i) x.v[i] = ge ? y.v[i] : x.v[i];
        }
        return x;
    }
    // fully reduced, strict limbs (the stored affine coordinates)
    ZK_HD static Fs canonical_lt2p(const Fs& a) {
        Fs x = canon_floor(a);
        normalize_strict(x);
        return x;
    }

    // ---- arkworks layout <-> this representation -------------------------------------------
    // w: SAT little-endian 32-bit words of x*R mod p (R = 2^(32 SAT)), canonical.  Returns x*R' (strict, in (-p, p)).
    ZK_HD static Fs from_sat(const uint32_t* w) {
        Fs t = split_words(w);
        Fs c;
#pragma unroll
        for (int i = 0; i < NL; ++i) c.v[i] = (uint32_t)P::C_IN(i);
        return mul(t, c);
    }
    // inverse of from_sat: writes the canonical x*R mod p words
    ZK_HD void to_sat(uint32_t* w) const {
        Fs c;
#pragma unroll
        for (int i = 0; i < NL; ++i) c.v[i] = (uint32_t)P::C_OUT(i);
        canon_floor(mul(*this, c)).pack_words(w);
    }
    // plain non-negative integer (no Montgomery factor change): 32-bit words -> strict limbs
    ZK_HD static Fs split_words(const uint32_t* w) {
        Fs t;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int bit = 30 * i;
            const int wi = bit >> 5, off = bit & 31;
            uint64_t lo = wi < SAT ? w[wi] : 0u;
            uint64_t hi = (wi + 1) < SAT ? w[wi + 1] : 0u;
            t.v[i] = (uint32_t)(((hi << 32) | lo) >> off) & M;
        }
        normalize_strict(t);
        return t;
    }
    // floor limbs of a non-negative value below 2^(32 SAT) -> words
    ZK_HD void pack_words(uint32_t* w) const { zk_pack_words<30>(*this, w); }

    // a^e, e little-endian 32-bit words
    ZK_HD static Fs pow_words(const Fs& a, const uint32_t* e, int n) { return zk_pow_words(a, e, n); }
    // Fermat inverse; inverse(0) = 0
    ZK_HD static Fs inverse(const Fs& a) {
        uint32_t e[SAT];
#pragma unroll
        for (int i = 0; i < SAT; ++i) e[i] = P::MODW(i);
        zk_words_minus_two(e);
        return zk_pow_words(a, e, SAT);
    }
};
