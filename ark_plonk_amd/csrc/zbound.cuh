// Bounded lazy arithmetic over the 29-bit-limb Fr type of the NTT (fieldu.cuh), with the bound carried in the TYPE: the operators,
// the loads and stores of fr_io.cuh in typed form, and the load conversion into the R' = 2^261 Montgomery form.  Shared by every
// kernel that computes lazily on that type outside the NTT passes -- the quotient (quotient.hip), the gate terms of the circuit check
// (check.hip), which tests the very summands the quotient enforces, the KZG opening and evaluation kernels (kzg.hip) and the query
// column (lookup.hip): a bound rule is corrected here, once, for all of them.
#pragma once
#include "fr_io.cuh"

#include <cmath>

namespace {

// Z<F, B> holds a value < (B / 10) * r.  A Montgomery product needs a * b < 2^261 * r / r^2 ~ 70 r^2 (169 r^2 on BN254) and
// returns < 2r; sums add their bounds; a difference a - b adds the smallest of 2r / 8r / 16r that covers b.  Every rule is a
// static_assert, so a formula that could overflow does not compile.
template <class F, int B>
struct Z {
    typedef F Field;
    F v;
    ZK_D Z() {}
    ZK_D Z(const F& f) : v(f) {}
    template <int B2>
    ZK_D Z(const Z<F, B2>& o) : v(o.v) {      // widening only
        static_assert(B2 <= B, "bound would shrink");
    }
};
template <class F, int A, int B>
ZK_D Z<F, 20> operator*(const Z<F, A>& a, const Z<F, B>& b) {
    static_assert(A * B <= 6400, "Montgomery product operands too large");
    return {F::mul(a.v, b.v)};
}
template <class F, int A>
ZK_D Z<F, 20> zsqr(const Z<F, A>& a) {
    static_assert(A * A <= 6400, "square operand too large");
    return {F::sqr(a.v)};
}
// a * a by the general product, for the kernels that were written with it (kzg.hip's power loops) and keep their instructions; one
// operand, so that the product is compiled knowing both are the same value, as it is where F::mul(a, a) stands in a kernel
template <class F, int A>
ZK_D Z<F, 20> zmul_self(const Z<F, A>& a) {
    static_assert(A * A <= 6400, "square operand too large");
    return {F::mul(a.v, a.v)};
}
template <class F, int A, int B>
ZK_D Z<F, A + B> operator+(const Z<F, A>& a, const Z<F, B>& b) {
    static_assert(A + B <= 640, "sum too large for the 261-bit container");
    return {F::add(a.v, b.v)};
}
template <int B>
struct SubK {
    static_assert(B <= 160, "subtrahend above 16r");
    static constexpr int K = B <= 20 ? 20 : B <= 80 ? 80 : 160;
};
template <class F, int A, int B>
ZK_D Z<F, A + SubK<B>::K> operator-(const Z<F, A>& a, const Z<F, B>& b) {
    static_assert(A + SubK<B>::K <= 640, "difference too large for the 261-bit container");
    if constexpr (SubK<B>::K == 20) return {F::sub2(a.v, b.v)};
    else if constexpr (SubK<B>::K == 80) return {F::sub8(a.v, b.v)};
    else return {F::sub16(a.v, b.v)};
}
// A value that starts below B0 / 10 r and takes up at most N terms below G / 10 r each, in a loop whose count is known at run time only
// (N terms of a sum: B0 = 0; N steps of a scan).  The variable has the bound after the last step, T, from the start; the sum rule is
// checked once, for that.  What keeps the count at N is the caller's: it names the constant that does.
template <class F, int B0, int G, int N>
struct ZRun {
    static_assert(B0 + N * G <= 640, "sum too large for the 261-bit container");
    typedef Z<F, B0 + N * G> T;
    ZK_D static T step(const T& acc, const Z<F, G>& term) { return {F::add(acc.v, term.v)}; }
};
// value != 0 mod r, exactly.  Zero has several encodings (0, r, 2r, ...): a value below 2r is 0 or r when it is a multiple of r;
// anything larger goes through a product with one
template <class F, int B>
ZK_D bool nonzero(const Z<F, B>& t, const Z<F, 10>& one) {
    if constexpr (B <= 20) return !t.v.is_zero_mod_reduced();
    else return !(t * one).v.is_zero_mod_reduced();
}

template <class F, int B>
ZK_D Z<F, 20> delta4(const Z<F, B>& f, const Z<F, 10>& one, const Z<F, 10>& c2, const Z<F, 10>& c3) {   // f(f-1)(f-2)(f-3)
    return (f * (f - one)) * ((f - c2) * (f - c3));
}

// The accesses of fr_io.cuh, typed.  A stored 32-byte element and a kernel-argument multiplier are canonical (the host reduces the
// latter: to_rprime); a 48-byte limb vector has the bound its buffer is declared with, T, on both sides: a value wider than T does not
// convert ("bound would shrink"), so a writer cannot outgrow what the reader was compiled for.
template <class F>
ZK_D Z<F, 10> ld_c(const void* base, uint64_t idx) { return {ld_u<F>(base, idx)}; }
template <class F>
ZK_D Z<F, 10> unpack_c(const Packed& p) { return {unpack<F>(p)}; }
template <class F>
ZK_D Z<F, 10> z_one() { return {F::one()}; }          // 1 in the R' form: x * 1 keeps the value and brings it under 2r
template <class F>
ZK_D void st_c(void* base, uint64_t idx, const Z<F, 20>& x) { st_u<F>(base, idx, x.v); }     // canonical_lt2p: below 2r
template <class T>
ZK_D T ld_z(const void* base, uint64_t idx) { return {ld_l<typename T::Field>(base, idx)}; }
template <class T>
ZK_D void st_z(void* base, uint64_t idx, const T& x) { st_l<typename T::Field>(base, idx, x.v); }

// arkworks Montgomery value x * 2^256 (canonical, 8 words) -> x * 2^261 mod r, < RP_B / 10 * r:
// shift left by 5 bits (32 v < 32 r < 2^260), subtract q2 * r with q2 = floor(T * ratio_fx / 2^13), T = floor(32 v / 2^(BITS - 3)) < 256
// (three bits below the 2^BITS place, so the truncated top costs < 2^BITS / 8r = 0.17 r), then r once more if the rest is still >= r.
// ratio_fx / 2^10 < 2^BITS / r by less than 2^-9, so q2 <= 32 v / r (the difference never goes negative) and
//     32 v / r - q2  <  1 (floor) + 2^BITS / 8r (top) + 256 / 2^12 (ratio)  <  1.23:
// the rest is < 1.23 r before and < r after the conditional subtraction, on both curves.  Measured by the host harness
// (tests/test_fieldu.py: the boundary words and 10^5 random ones per curve): the largest result is r - 1 on BLS12-381 and on BN254
// (rest before the subtraction: 1.155 r and 1.177 r), at most 31 r taken off.  With the top truncated at the 2^BITS place
// (>> top_shift, >> 10) the same inputs gave 1.083 r and 1.290 r: past the 1.2 r every L below is typed with.
// RP_B stays at 12: no rule below needs it tighter.  rtab[q] = q * r, ratio_fx and top_shift: rp_table below.
constexpr int RP_B = 12;      // a loaded value is a Z<F, RP_B>: the L type of quotient.hip and check.hip
template <class F>
ZK_D Z<F, RP_B> to_rp(const El& e, const uint32_t (*rtab)[F::NL], uint32_t ratio_fx, uint32_t top_shift) {
    uint32_t w[8] = {e.a.x, e.a.y, e.a.z, e.a.w, e.b.x, e.b.y, e.b.z, e.b.w};
    F l = F::split_words(w);
    F s;
#pragma unroll
    for (int i = F::NL - 1; i >= 1; --i) s.v[i] = ((l.v[i] << 5) | (l.v[i - 1] >> 24)) & (i == F::NL - 1 ? 0xffffffffu : F::M);
    s.v[0] = (l.v[0] << 5) & F::M;
    const uint32_t q2 = ((s.v[F::NL - 1] >> (top_shift - 3)) * ratio_fx) >> 13;
    F t;
#pragma unroll
    for (int i = 0; i < F::NL; ++i) t.v[i] = s.v[i] - rtab[q2][i];
    F::normalize(t);
    F d;
#pragma unroll
    for (int i = 0; i < F::NL; ++i) d.v[i] = t.v[i] - rtab[1][i];
    F::normalize(d);
    const bool neg = ((int32_t)d.v[F::NL - 1]) < 0;
    F r;
#pragma unroll
    for (int i = 0; i < F::NL; ++i) r.v[i] = neg ? t.v[i] : d.v[i];
    return Z<F, RP_B>(r);
}
template <class F>
ZK_D Z<F, RP_B> ld_rp(const void* base, uint64_t idx, const uint32_t (*rtab)[F::NL], uint32_t ratio_fx, uint32_t top_shift) {
    return to_rp<F>(ld_el(base, idx), rtab, ratio_fx, top_shift);
}

// ---- host side
// arkworks-form Fr (R = 2^256) -> the canonical R' = 2^261 residue as 29-bit limbs
template <class Cv>
typename Cv::FrU to_rp_host(const typename Cv::Fr& v) { return Cv::FrU::split_words(to_rprime(v).v); }
// what to_rp reads: rtab[q] = q * r as 29-bit limbs for q < len, ratio_fx = floor(2^BITS / r * 2^10) - 1 and
// top_shift = BITS - 29 * (NL - 1) (>= 3: to_rp keeps three bits below it).  len must cover the largest q2 (32 v / r < 32, and the
// estimate never exceeds it).
template <class Cv>
void rp_table(uint32_t (*rtab)[Cv::FrU::NL], uint32_t len, uint32_t& ratio_fx, uint32_t& top_shift) {
    typedef typename Cv::FrU FU;
    uint32_t rw[8];
    for (int i = 0; i < 8; ++i) rw[i] = Cv::FrP::MOD(i);
    FU acc = FU::zero();
    const FU rl = FU::split_words(rw);
    for (uint32_t k = 0; k < len; ++k) {
        for (int i = 0; i < FU::NL; ++i) rtab[k][i] = acc.v[i];
        acc = FU::add(acc, rl);
    }
    long double rv = 0;
    for (int i = Cv::Fr::N - 1; i >= 0; --i) rv = rv * 4294967296.0L + (long double)Cv::FrP::MOD(i);
    ratio_fx = (uint32_t)floorl(ldexpl(1.0L, Cv::FrP::BITS + 10) / rv) - 1;
    static_assert(Cv::FrP::BITS - 29 * (FU::NL - 1) >= 3, "to_rp reads three bits below the 2^BITS place of the top limb");
    top_shift = (uint32_t)(Cv::FrP::BITS - 29 * (FU::NL - 1));
}
// The host side of the gate-argument blocks (QArgsU of quotient.hip, CArgsU of check.hip, from zk_quotient_args and
// zk_circuit_check_args): what the two share, assigned by member name, so that neither layout matters.
// the 4 x 64-bit words of an ABI argument as they are: no reduced-element test (fr_reduced, fr_io.cuh, where one is made)
template <class Fr>
Fr fr_arg(const uint64_t* m) {
    Fr v;
    memcpy(v.v, m, 32);
    return v;
}
template <class A, class Q>
void fill_gate_columns(A& a, const Q* q) {
    a.w_l = q->w_l; a.w_r = q->w_r; a.w_o = q->w_o; a.w_4 = q->w_4; a.pi = q->pi;
    a.q_m = q->q_m; a.q_l = q->q_l; a.q_r = q->q_r; a.q_o = q->q_o; a.q_4 = q->q_4; a.q_c = q->q_c; a.q_arith = q->q_arith;
    a.q_range = q->q_range; a.q_logic = q->q_logic; a.q_fixed = q->q_fixed_group_add; a.q_var = q->q_variable_group_add;
}
// the curve coefficients, the small integers of the widgets and what to_rp reads (table_len rows of a.rtab)
template <class Cv, class A>
void fill_gate_consts(A& a, const uint64_t* coeff_a, const uint64_t* coeff_d, uint32_t table_len) {
    typedef typename Cv::Fr Fr;
    auto U = [](const Fr& v) { return to_rp_host<Cv>(v); };
    a.coeff_a = U(fr_arg<Fr>(coeff_a)); a.coeff_d = U(fr_arg<Fr>(coeff_d)); a.one = U(Fr::one());
    a.c2 = U(Fr::from_u32(2)); a.c3 = U(Fr::from_u32(3)); a.c4 = U(Fr::from_u32(4)); a.c9 = U(Fr::from_u32(9));
    a.c18 = U(Fr::from_u32(18)); a.c81 = U(Fr::from_u32(81)); a.c83 = U(Fr::from_u32(83));
    rp_table<Cv>(a.rtab, table_len, a.ratio_fx, a.top_shift);
}

}  // namespace
