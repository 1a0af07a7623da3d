// The verifier's device side: batch decoding of compressed G1 points, the per-proof scalars of the two pairing inputs,
// and the column sum that folds the key-base scalars of a range of the batch.
//
// g1_decompress applies the rules of wire.hip's g1_de_c (ark-serialize 0.3 `GroupAffine::deserialize`: SWFlags, x < q, the square
// root of x^3 + b with the sign the flag names, `is_in_correct_subgroup_assuming_on_curve`) to n encodings at once, one lane per point,
// and reports a status per point where the host function returns an error.  The field is the device form of the MSM base field
// (fields.cuh) and the group law is ecu.cuh's, as in g1_fixed_base: nothing is restated here.  Both exponents -- (q + 1) / 4 and r -- are
// constants of the curve, so every lane that reaches a loop takes the same branches in it.
#include "api_internal.h"
#include "block_inverse.cuh"
#include "domain.cuh"
#include "g1_lift.cuh"

namespace {

// an encoding's integer x (flags masked off) against q, both as little-endian words
template <class Cv>
__device__ bool x_below_modulus(const uint32_t* w) {
    typedef typename Cv::FqU F;
    for (int i = F::SAT - 1; i >= 0; --i) {
        const uint32_t m = Cv::FqP::MOD(i);
        if (w[i] != m) return w[i] < m;
    }
    return false;
}

template <class Cv>
__global__ void __launch_bounds__(128) g1_decompress(const uint8_t* in, uint64_t n, uint32_t* out_xy, uint8_t* out_inf, uint8_t* status) {
    typedef typename Cv::FqU F;
    typedef typename Cv::FqP FqP;
    constexpr int SAT = F::SAT;
    constexpr int G = (FqP::BITS + 2 + 7) / 8;                 // serialize_with_flags::<SWFlags>
    static_assert(G == 4 * SAT, "a compressed point fills the words of a base-field element");
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* src = in + i * G;
    uint32_t* dst = out_xy + i * 2 * SAT;
    uint32_t w[SAT];
#pragma unroll
    for (int k = 0; k < SAT; ++k)
        w[k] = (uint32_t)src[4 * k] | (uint32_t)src[4 * k + 1] << 8 | (uint32_t)src[4 * k + 2] << 16 | (uint32_t)src[4 * k + 3] << 24;
    const uint32_t flags = w[SAT - 1] >> 30;                   // bit 1: y is the larger of (y, -y); bit 0: infinity
    w[SAT - 1] &= 0x3fffffffu;
    // a rejected encoding leaves the null point behind (x = y = 0 words)
    auto reject = [&](uint8_t code) {
        for (int k = 0; k < 2 * SAT; ++k) dst[k] = 0;
        out_inf[i] = 0;
        status[i] = code;
    };
    if (flags == 3u) return reject(ZK_G1_BAD_FLAGS);           // SWFlags::from_u8: both bits set is invalid
    if (!x_below_modulus<Cv>(w)) return reject(ZK_G1_X_NOT_REDUCED);
    if (flags & 1u) {                                          // infinity whatever the x bits are: GroupAffine::zero() = (0, 1)
        for (int k = 0; k < SAT; ++k) {
            dst[k] = 0;
            dst[SAT + k] = FqP::R(k);
        }
        out_inf[i] = 1;
        status[i] = ZK_G1_OK;
        return;
    }
    // the lift of x (g1_lift.cuh): x into the device's Montgomery form, x^3 + b, its root, the sign the flag names
    F x, rhs, y;
    g1_curve_rhs<Cv>(w, x, rhs);
    if (!g1_sqrt<Cv>(rhs, y)) return reject(ZK_G1_NOT_ON_CURVE);
    y = g1_pick_root<Cv>(y, (flags & 2u) != 0);
    AffineU<F> p;
    p.x = F::canonical_lt2p(x);
    p.y = F::canonical_lt2p(y);
    // r * P == O (is_in_correct_subgroup_assuming_on_curve): double-and-add from the top bit, as G1Host::scalar_mul
    XYZZu<F> acc = XYZZu<F>::infinity();
    for (int limb = Cv::FrP::N - 1; limb >= 0; --limb) {
        const uint32_t word = Cv::FrP::MOD(limb);
        for (int bit = 31; bit >= 0; --bit) {
            acc = XYZZu<F>::dbl(acc);
            if ((word >> bit) & 1u) acc = XYZZu<F>::madd(acc, p);
        }
    }
    if (!acc.is_inf()) return reject(ZK_G1_NOT_IN_SUBGROUP);
    p.x.to_sat(dst);
    p.y.to_sat(dst + SAT);
    out_inf[i] = 0;
    status[i] = ZK_G1_OK;
}

template <class Cv>
int decompress_impl(zk_ctx* c, const void* d_in, size_t n, void* d_out_xy, void* d_out_inf, void* d_status) {
    ProfScope ps(c, "g1_decompress");
    hipLaunchKernelGGL(g1_decompress<Cv>, dim3(blocks_of(n, 128)), dim3(128), 0, c->stream, (const uint8_t*)d_in, (uint64_t)n, (uint32_t*)d_out_xy,
                       (uint8_t*)d_out_inf, (uint8_t*)d_status);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------------------ per-proof scalars
// One 64-lane workgroup per proof.  The lanes stride over the proof's public inputs (the barycentric sum of proof.rs:635-666), one
// denominator n (z - w^pos) each, with l_1's denominator n (z - 1) as one more item; a round of 64 items is inverted with ONE field
// inversion (block_inverse.cuh at this workgroup's width, computed in Called<Fr> and stored as Fr).  Lane 0 then
// evaluates r_0, the widget identities and the permutation and lookup terms and writes the rows.  The arithmetic is the canonical
// Fr of field.cuh: the quotient's widget functions (quotient.hip) carry the bounds of its lazy reduction in their types and are not
// reusable at a point, so the formulas stand here a second time, on canonical values.
constexpr uint32_t VT = 64;
constexpr int N_KEY = ZK_VERIFY_N_KEY_BASES, N_PROOF = ZK_VERIFY_N_PROOF_BASES;
// evaluation row (wire.hip's replay): the proof's 16, then the seven found by label
enum { E_A, E_B, E_C, E_D, E_S0, E_S1, E_S2, E_PERM, E_QLOOKUP, E_Z2N, E_H1, E_H1N, E_H2, E_F, E_T, E_TN, E_AN, E_BN, E_DN, E_QARITH, E_QC, E_QL, E_QR };
enum { C_ZETA, C_BETA, C_GAMMA, C_DELTA, C_EPS, C_ALPHA, C_RANGE, C_LOGIC, C_FIXED, C_VAR, C_LOOKUP, C_Z, C_AW, C_SAW };
// key row: the selectors of the linearisation commitment, the sigmas, the table columns, G
enum { K_QM, K_QL, K_QR, K_QO, K_Q4, K_QC, K_QRANGE, K_QLOGIC, K_QFIXED, K_QVAR, K_QLOOKUP, K_S0, K_S1, K_S2, K_S3, K_T1, K_T2, K_T3, K_T4, K_G };
// proof row: the commitments in the proof's order, then the two openings
enum { P_A, P_B, P_C, P_D, P_Z, P_F, P_H1, P_H2, P_Z2, P_T1, P_T2, P_T3, P_T4, P_WAW, P_WSAW };

struct ScalarArgs {
    const void *challenges, *evals, *pi_values, *weights;
    const uint64_t *pi_offsets, *pi_positions;
    const uint8_t *parse_status, *point_status;
    void *key_rows, *proof_rows, *open_rows;
    uint8_t* status;
    uint32_t log_n;
    Packed coeff_a, coeff_d;
};

// The canonical Fr of field.cuh with its arithmetic behind CALLS.  field.cuh's members are force-inlined, which is right for a kernel
// with a handful of products; this one has several hundred in a row, once per proof, and inlined they are minutes of compile time for
// code whose speed does not matter.  Same values, same functions: every member forwards to F's.
template <class F, class P>
struct Called : F {
    __device__ Called() {}
    __device__ Called(const F& f) : F(f) {}
    static __device__ __noinline__ Called mul(const Called& a, const Called& b) { return Called(F::mul(a, b)); }
    static __device__ __noinline__ Called add(const Called& a, const Called& b) { return Called(F::add(a, b)); }
    static __device__ __noinline__ Called sub(const Called& a, const Called& b) { return Called(F::sub(a, b)); }
    static __device__ __noinline__ Called neg(const Called& a) { return Called(F::neg(a)); }
    static __device__ Called sqr(const Called& a) { return mul(a, a); }
    static __device__ Called zero() { return Called(F::zero()); }
    static __device__ Called one() { return Called(F::one()); }
    static __device__ Called to_mont(const Called& c) { return mul(c, Called(F::r2())); }
    static __device__ Called from_mont(const Called& m) {
        Called o = zero();
        o.v[0] = 1;
        return mul(m, o);
    }
    static __device__ Called from_u64(uint64_t x) {
        Called c = zero();
        c.v[0] = (uint32_t)x;
        c.v[1] = (uint32_t)(x >> 32);
        return to_mont(c);
    }
    static __device__ Called from_u32(uint32_t x) { return from_u64(x); }
    static __device__ __noinline__ Called pow_u64(const Called& a, uint64_t e) {
        const uint32_t l[2] = {(uint32_t)e, (uint32_t)(e >> 32)};
        return zk_pow_words(a, l, 2);
    }
    static __device__ __noinline__ Called inverse(const Called& a) {          // Fermat; inverse(0) = 0
        uint32_t e[F::N];
        for (int i = 0; i < F::N; ++i) e[i] = P::MOD(i);
        zk_words_minus_two(e);
        return zk_pow_words(a, e, F::N);
    }
    __device__ Called operator+(const Called& b) const { return add(*this, b); }
    __device__ Called operator-(const Called& b) const { return sub(*this, b); }
    __device__ Called operator*(const Called& b) const { return mul(*this, b); }
};

// the kernel's LDS; 16: 128-bit LDS access
template <class Fr>
struct alignas(16) WaveLds {
    BlockInverseLds<Fr, VT> inv;
    Fr sum[VT], l1_inv;
    uint32_t on_domain;
};

template <class Fr>
ZK_D Fr fr_packed(const Packed& p) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = p.w[i];
    return r;
}
// f (f - 1) (f - 2) (f - 3): widget/range.rs:66-74, widget/logic.rs:94-102
template <class Fr>
ZK_D Fr delta4(const Fr& f) {
    const Fr one = Fr::one(), two = Fr::from_u32(2), three = Fr::from_u32(3);
    return f * (f - one) * (f - two) * (f - three);
}

template <class Cv>
__global__ void __launch_bounds__(VT) verify_scalars(ScalarArgs A) {
    typedef typename Cv::FrP FrP;
    typedef Called<typename Cv::Fr, FrP> Fr;
    __shared__ WaveLds<typename Cv::Fr> lds;
    const uint64_t j = blockIdx.x;
    const uint32_t t = threadIdx.x;
    auto zero_rows = [&](uint8_t code) {
        if (t < N_KEY) st_fr<Fr>(A.key_rows, j * N_KEY + t, Fr::zero());
        if (t < N_PROOF) st_fr<Fr>(A.proof_rows, j * N_PROOF + t, Fr::zero());
        if (t < 2) st_fr<Fr>(A.open_rows, j * 2 + t, Fr::zero());
        if (t == 0) A.status[j] = code;
    };
    // what stages 1 and 2 rejected stays rejected (uniform over the workgroup: every lane reads the same bytes)
    uint8_t st = A.parse_status ? A.parse_status[j] : 0;
    if (st == 0 && A.point_status) {
        for (int k = 0; k < N_PROOF && st == 0; ++k) {
            const uint8_t ps = A.point_status[j * N_PROOF + k];
            if (ps) st = (uint8_t)(ZK_VERIFY_BAD_POINT + ps);
        }
    }
    if (st) return zero_rows(st);

    auto Ch = [&](int k) { return ld_fr<Fr>(A.challenges, j * ZK_VERIFY_N_CHALLENGES + k); };
    auto Ev = [&](int k) { return ld_fr<Fr>(A.evals, j * ZK_VERIFY_N_EVALS + k); };
    const Fr one = Fr::one();
    const Fr z = Ch(C_Z);
    const Fr w = domain_root<FrP, Fr>(A.log_n);              // the root of unity of size n
    const Fr n_fr = Fr::from_u64((uint64_t)1 << A.log_n);

    // ---- the denominators: n (z - w^pos) per public input, then n (z - 1)
    const uint64_t o = A.pi_offsets[j], n_pi = A.pi_offsets[j + 1] - o;
    if (t == 0) lds.on_domain = 0;
    __syncthreads();
    Fr sum = Fr::zero();
    for (uint64_t base = 0; base <= n_pi; base += VT) {     // n_pi + 1 items; the bound is uniform
        const uint64_t k = base + t;
        Fr wp = one, den = one;
        if (k <= n_pi) {
            if (k < n_pi) wp = Fr::pow_u64(w, A.pi_positions[o + k]);
            den = n_fr * (z - wp);
            if (den.is_zero()) {                             // inverse(0) = 0 would pass silently: the challenge lies on the domain
                atomicOr(&lds.on_domain, 1u);
                den = one;
            }
        }
        const Fr inv = block_inverse(den, lds.inv);
        if (k < n_pi) sum = sum + ld_fr<Fr>(A.pi_values, o + k) * wp * inv;
        if (k == n_pi) lds.l1_inv = inv;
        __syncthreads();                                     // the next round writes lds.inv again
    }
    lds.sum[t] = sum;
    __syncthreads();
    if (lds.on_domain) return zero_rows(ZK_VERIFY_Z_ON_DOMAIN);
    if (t != 0) return;
    for (uint32_t k = 1; k < VT; ++k) sum = sum + lds.sum[k];

    // ---- proof.rs:427-486 (r_0) and :488-611 (the linearisation commitment's scalars)
    Fr z_n = z;
    for (uint32_t k = 0; k < A.log_n; ++k) z_n = Fr::sqr(z_n);
    const Fr zh = z_n - one;
    const Fr l1 = zh * lds.l1_inv;
    const Fr pi_eval = zh * sum;
    const Fr a = Ev(E_A), b = Ev(E_B), c = Ev(E_C), d = Ev(E_D), a_n = Ev(E_AN), b_n = Ev(E_BN), d_n = Ev(E_DN);
    const Fr s0 = Ev(E_S0), s1 = Ev(E_S1), s2 = Ev(E_S2), perm = Ev(E_PERM);
    const Fr q_arith = Ev(E_QARITH), q_c = Ev(E_QC), q_l = Ev(E_QL), q_r = Ev(E_QR);
    const Fr z2n = Ev(E_Z2N), h1n = Ev(E_H1N), h2 = Ev(E_H2), f_e = Ev(E_F), t_e = Ev(E_T), t_n = Ev(E_TN);
    const Fr al = Ch(C_ALPHA), be = Ch(C_BETA), ga = Ch(C_GAMMA), de = Ch(C_DELTA), ep = Ch(C_EPS), ze = Ch(C_ZETA), ls = Ch(C_LOOKUP);
    const Fr ca = fr_packed<Fr>(A.coeff_a), cd = fr_packed<Fr>(A.coeff_d);
    const Fr ls2 = ls * ls, ls3 = ls2 * ls, al2 = al * al;
    const Fr opd = one + de, e1d = ep * opd;
    const Fr sig = (a + be * s0 + ga) * (b + be * s1 + ga) * (c + be * s2 + ga);         // shared by r_0 and the sigma3 scalar
    const Fr r0 = pi_eval - sig * ((d + ga) * perm * al) - l1 * al2 - ls2 * z2n * (e1d + de * h2) * (e1d + h2 + de * h1n) - ls3 * l1;

    Fr lin[N_KEY], lp[N_PROOF];                               // lin: key bases; lp: proof bases (z, h_1, z_2, t_1..4 used)
    lin[K_QM] = a * b * q_arith;
    lin[K_QL] = a * q_arith;
    lin[K_QR] = b * q_arith;
    lin[K_QO] = c * q_arith;
    lin[K_Q4] = d * q_arith;
    lin[K_QC] = q_arith;
    const Fr c2 = Fr::from_u32(2), c3 = Fr::from_u32(3), c4 = Fr::from_u32(4), c9 = Fr::from_u32(9), c18 = Fr::from_u32(18),
             c81 = Fr::from_u32(81), c83 = Fr::from_u32(83);
    {   // widget/range.rs:47-63
        const Fr s = Ch(C_RANGE), k = s * s, k2 = k * k;
        lin[K_QRANGE] = (delta4(c - c4 * d) + delta4(b - c4 * c) * k + delta4(a - c4 * b) * k2 + delta4(d_n - c4 * a) * k2 * k) * s;
    }
    {   // widget/logic.rs:65-133
        const Fr s = Ch(C_LOGIC), k = s * s, k2 = k * k;
        const Fr la = a_n - c4 * a, lb = b_n - c4 * b, ld = d_n - c4 * d;
        const Fr F = c * (c * (c4 * c - c18 * (la + lb) + c81) + c18 * (la * la + lb * lb) - c81 * (la + lb) + c83);
        const Fr E = c3 * (la + lb + ld) - c2 * F;
        const Fr B = q_c * (c9 * ld - c3 * (la + lb));
        lin[K_QLOGIC] = (delta4(la) + delta4(lb) * k + delta4(ld) * k2 + (c - la * lb) * k2 * k + (B + E) * k2 * k2) * s;
    }
    {   // widget/ecc/fixed_base_scalar_mul.rs:88-156
        const Fr s = Ch(C_FIXED), k = s * s, k2 = k * k;
        const Fr bit = d_n - d - d;
        const Fr bit_cons = bit * (bit - one) * (bit + one);
        const Fr y_alpha = bit * bit * (q_r - one) + one, x_alpha = q_l * bit;
        const Fr xy_cons = (bit * q_c - c) * k;
        const Fr cab = c * a * b * cd;
        const Fr x_acc = ((a_n + a_n * cab) - (x_alpha * b + y_alpha * a)) * k2;
        const Fr y_acc = ((b_n - b_n * cab) - (y_alpha * b - ca * x_alpha * a)) * k2 * k;
        lin[K_QFIXED] = (bit_cons + x_acc + y_acc + xy_cons) * s;
    }
    {   // widget/ecc/curve_addition.rs:62-97: (x1, y1) = (a, b), (x2, y2) = (c, d), (x3, y3) = (a_n, b_n), x1 y2 = d_n
        const Fr s = Ch(C_VAR), k = s * s;
        const Fr y1x2 = b * c, y1y2 = b * d, x1x2 = a * c, x1y2 = d_n;
        const Fr dd = cd * x1y2 * y1x2;
        const Fr xy = a * d - x1y2;
        const Fr x3c = ((x1y2 + y1x2) - (a_n + a_n * dd)) * k;
        const Fr y3c = ((y1y2 - ca * x1x2) - (b_n - b_n * dd)) * k * k;
        lin[K_QVAR] = (xy + x3c + y3c) * s;
    }
    // widget/lookup.rs:223-300
    lin[K_QLOOKUP] = ((a + ze * (b + ze * (c + ze * d))) - f_e) * ls;
    lp[P_Z2] = opd * (ep + f_e) * (e1d + t_e + de * t_n) * ls2 + l1 * ls3;
    lp[P_H1] = Fr::neg(z2n * ls2 * (e1d + h2 + de * h1n));
    // permutation.rs:327-388
    const Fr bz = be * z;
    lp[P_Z] = (a + bz + ga) * (b + Fr::from_u32(PERM_K[1]) * bz + ga) * (c + Fr::from_u32(PERM_K[2]) * bz + ga) * ((d + Fr::from_u32(PERM_K[3]) * bz + ga) * al) + l1 * al2;
    lin[K_S3] = Fr::neg(sig * (be * perm * al));
    // proof.rs:590-606: -Z_H(z) z^(k n)
    Fr zp = one;
    for (int k = 0; k < 4; ++k) {
        lp[P_T1 + k] = Fr::neg(zh * zp);
        zp = zp * z_n;
    }

    // ---- the two openings, weighted: u (sum_k chi^k (C_k - v_k G) + z W_aw) + u' (sum_k chi'^k (C'_k - v'_k G) + z w W_saw)
    const Fr u = Fr::to_mont(ld_fr<Fr>(A.weights, 2 * j)), v = Fr::to_mont(ld_fr<Fr>(A.weights, 2 * j + 1));
    const Fr chi = Ch(C_AW), chj = Ch(C_SAW);
    Fr up[11], vp[7];                                        // u chi^k, u' chi'^k
    up[0] = u;
    for (int k = 1; k < 11; ++k) up[k] = up[k - 1] * chi;
    vp[0] = v;
    for (int k = 1; k < 7; ++k) vp[k] = vp[k - 1] * chj;
    Fr key[N_KEY], pr[N_PROOF];
    for (int k = K_QM; k <= K_QLOOKUP; ++k) key[k] = u * lin[k];
    key[K_S0] = up[1];
    key[K_S1] = up[2];
    key[K_S2] = up[3];
    key[K_S3] = u * lin[K_S3];
    Fr tw = up[6] + vp[6];                                   // the table commitment: table_1 + zeta table_2 + zeta^2 table_3 + zeta^3 table_4
    for (int k = 0; k < 4; ++k) {
        key[K_T1 + k] = tw;
        tw = tw * ze;
    }
    // the evaluations v_k of the aw list (v_0 = -r_0) and of the saw list, in list order
    const Fr av[11] = {Fr::neg(r0), s0, s1, s2, f_e, h2, t_e, a, b, c, d};
    const Fr sv[7] = {perm, a_n, b_n, d_n, h1n, z2n, t_n};
    Fr g = Fr::zero();
    for (int k = 0; k < 11; ++k) g = g + up[k] * av[k];
    for (int k = 0; k < 7; ++k) g = g + vp[k] * sv[k];
    key[K_G] = Fr::neg(g);
    pr[P_A] = up[7] + vp[1];
    pr[P_B] = up[8] + vp[2];
    pr[P_C] = up[9];
    pr[P_D] = up[10] + vp[3];
    pr[P_Z] = u * lp[P_Z] + vp[0];
    pr[P_F] = up[4];
    pr[P_H1] = u * lp[P_H1] + vp[4];
    pr[P_H2] = up[5];
    pr[P_Z2] = u * lp[P_Z2] + vp[5];
    for (int k = 0; k < 4; ++k) pr[P_T1 + k] = u * lp[P_T1 + k];
    pr[P_WAW] = u * z;
    pr[P_WSAW] = v * z * w;
    for (int k = 0; k < N_KEY; ++k) st_fr<Fr>(A.key_rows, j * N_KEY + k, Fr::from_mont(key[k]));
    for (int k = 0; k < N_PROOF; ++k) st_fr<Fr>(A.proof_rows, j * N_PROOF + k, Fr::from_mont(pr[k]));
    st_fr<Fr>(A.open_rows, 2 * j, Fr::from_mont(u));
    st_fr<Fr>(A.open_rows, 2 * j + 1, Fr::from_mont(v));
    A.status[j] = ZK_VERIFY_OK;
}

// out[c] = sum over rows of rows[r][c]: one workgroup per column, a tree over the lanes' strided partial sums
constexpr uint32_t CT = 256;
template <class Cv>
__global__ void __launch_bounds__(CT) fr_column_sum(const void* rows, uint64_t n_rows, uint32_t n_cols, void* out) {
    typedef typename Cv::Fr Fr;
    __shared__ alignas(16) Fr part[CT];
    const uint32_t col = blockIdx.x, t = threadIdx.x;
    Fr s = Fr::zero();
    for (uint64_t r = t; r < n_rows; r += CT) s = Fr::add(s, ld_fr<Fr>(rows, r * n_cols + col));
    part[t] = s;
    __syncthreads();
    for (uint32_t d = CT / 2; d > 0; d >>= 1) {
        if (t < d) part[t] = Fr::add(part[t], part[t + d]);
        __syncthreads();
    }
    if (t == 0) st_fr<Fr>(out, col, part[0]);
}

template <class Cv>
int scalars_impl(zk_ctx* c, size_t n_proofs, const ScalarArgs& a) {
    ProfScope ps(c, "verify_scalars");
    hipLaunchKernelGGL(verify_scalars<Cv>, dim3((unsigned)n_proofs), dim3(VT), 0, c->stream, a);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}
template <class Cv>
int column_sum_impl(zk_ctx* c, const void* d_rows, size_t n_rows, uint32_t n_cols, void* d_out) {
    ProfScope ps(c, "fr_column_sum");
    hipLaunchKernelGGL(fr_column_sum<Cv>, dim3(n_cols), dim3(CT), 0, c->stream, d_rows, (uint64_t)n_rows, n_cols, d_out);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_verify_scalars_dev(zk_ctx* c, int curve_id, uint32_t log_n, size_t n_proofs, const void* d_challenges_mont, const void* d_evals_mont,
                          const void* d_pi_offsets, const void* d_pi_positions, const void* d_pi_values_mont, const uint64_t* coeff_a_mont,
                          const uint64_t* coeff_d_mont, const void* d_weights, const void* d_parse_status, const void* d_point_status,
                          void* d_key_rows, void* d_proof_rows, void* d_open_rows, void* d_status) {
    if (!c || !zk_curve_ok(curve_id) || !coeff_a_mont || !coeff_d_mont) return ZK_ERR_BAD_ARG;
    if (n_proofs && (!d_challenges_mont || !d_evals_mont || !d_pi_offsets || !d_weights || !d_key_rows || !d_proof_rows || !d_open_rows || !d_status))
        return ZK_ERR_BAD_ARG;
    const uint32_t two_adicity = zk_on_curve(curve_id, 0u, [](auto cv) { return (uint32_t)decltype(cv)::FrP::TWO_ADICITY; });
    if (log_n > two_adicity) return ZK_ERR_DOMAIN_TOO_LARGE;
    if (n_proofs >= ((size_t)1 << 31)) return ZK_ERR_UNSUPPORTED;
    if (n_proofs == 0) return ZK_OK;
    ScalarArgs a;
    a.challenges = d_challenges_mont;
    a.evals = d_evals_mont;
    a.pi_values = d_pi_values_mont;
    a.weights = d_weights;
    a.pi_offsets = (const uint64_t*)d_pi_offsets;
    a.pi_positions = (const uint64_t*)d_pi_positions;
    a.parse_status = (const uint8_t*)d_parse_status;
    a.point_status = (const uint8_t*)d_point_status;
    a.key_rows = d_key_rows;
    a.proof_rows = d_proof_rows;
    a.open_rows = d_open_rows;
    a.status = (uint8_t*)d_status;
    a.log_n = log_n;
    for (int i = 0; i < 4; ++i) {
        a.coeff_a.w[2 * i] = (uint32_t)coeff_a_mont[i];
        a.coeff_a.w[2 * i + 1] = (uint32_t)(coeff_a_mont[i] >> 32);
        a.coeff_d.w[2 * i] = (uint32_t)coeff_d_mont[i];
        a.coeff_d.w[2 * i + 1] = (uint32_t)(coeff_d_mont[i] >> 32);
    }
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return scalars_impl<decltype(cv)>(c, n_proofs, a); });
}

int zk_fr_column_sum_dev(zk_ctx* c, int curve_id, const void* d_rows, size_t n_rows, uint32_t n_cols, void* d_out) {
    if (!c || !zk_curve_ok(curve_id) || !n_cols || !d_out || (n_rows && !d_rows)) return ZK_ERR_BAD_ARG;
    if (n_cols > 65535) return ZK_ERR_UNSUPPORTED;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return column_sum_impl<decltype(cv)>(c, d_rows, n_rows, n_cols, d_out); });
}

int zk_g1_decompress_batch_dev(zk_ctx* c, int curve_id, const void* d_in, size_t n, void* d_out_xy, void* d_out_inf, void* d_status) {
    if (!c || !zk_curve_ok(curve_id) || (n && (!d_in || !d_out_xy || !d_out_inf || !d_status))) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    if (n > ((size_t)1 << 31) * 128 - 128) return ZK_ERR_UNSUPPORTED;        // the grid of one launch
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return decompress_impl<decltype(cv)>(c, d_in, n, d_out_xy, d_out_inf, d_status); });
}
