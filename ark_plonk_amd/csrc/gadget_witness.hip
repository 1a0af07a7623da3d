// The circuit builder on the device, the part that runs once per proof: the values of the variables the gadget calls of a segment
// create (gadget_layout.hip lists the gadgets and their sources in the reference; segments, shapes and errors: gadget_common.cuh).
//
//   gadget_w_poly        one lane per call: the computed output (q_m a b + q_l a + q_r b + q_c + q_4 d + pi) (-q_o)
//   gadget_w_range       one lane per (call, accumulator j): (v mod 2^bits) >> (bits - 2 (j + 1)) of the canonical integer v
//   gadget_w_logic       one lane per (call, quad): both input prefixes, their product quad, the prefix of a ^ b or a & b
//   gadget_w_curve       one lane per call: x1 y2 and the twisted Edwards sum; ONE field inversion per block (block_inverse.cuh)
//   gadget_w_fixed_walk  one lane per call: the width-2 NAF digits in closed form (digit of weight 2^j = bit j+1 of 3e - bit j+1 of e),
//                        a running sum in extended coordinates against the segment's table of affine multiples, the M + 1
//                        projective accumulators stored to the call's workspace
//   gadget_w_fixed_norm  one lane per (call, row): normalises with one shared inversion per block; writes acc_x, acc_y, xy_alpha and
//                        the scalar accumulator (3e >> s) - (e >> s)
//   gadget_w_select      one lane per call: the constant witness, the four constants of add_dummy_constraints, the four values of a
//                        select, the eight of a point select, the five of a point negation -- each the product with -q_o that
//                        arithmetic.rs:144-155 computes
//   gadget_w_is_zero     one lane per call: (a - b,) y = 1 / a or 1, b = 1 - a y; ONE field inversion per block, a zero input
//                        enters the block's product as 1
//   gadget_w_var_bits    one lane per (call, j < 256): bit j of the canonical scalar e, the accumulator e mod 2^(j+1) for j < M, the
//                        constant one of the identity
//   gadget_w_var_walk    one lane per call: 2 M unified additions in extended coordinates (doubling, then the addition of the
//                        selected point (bit x, 1 - bit + bit y)), the 2 M + 1 projective accumulators stored to the workspace
//   gadget_w_var_norm    one lane per (call, iteration): the three accumulators of the iteration made affine with one inversion
//                        per block (through the product of their Z), the eight values of the iteration
// The output of a lookup gate (ZK_GADGET_LOOKUP_OUT) is no kernel of this unit: one query of the table's map (lookup_map.hip).
// Values are canonical Montgomery Fr (field.cuh), what `assign` and the circuit check expect; the canonical integer of an input is one
// Montgomery product, prefixes and bits are shifts and masks on its words with compile-time word indices (no array is indexed at run
// time: both walks read the scalar's bits off the top of a word array that is shifted by constants).  The flag word: an input id that
// is not below the segment's var0 (an undefined variable), a scalar whose NAF has more than M digits (the reference asserts there), a
// zero denominator of the affine group law the reference computes with, which shows as a zero Z.  Every kernel guards its own
// addresses: a refused call leaves unspecified values, never an access outside the buffers.
//
// Working memory: one allocation per call, freed on every path; 256 bytes, + 96 (M + 1) B for a fixed-base and 96 (2 M + 1) B for a
// variable-base witness.
#include "gadget_common.cuh"
#include "block_inverse.cuh"

namespace {

// ---------------------------------------------------------------------------------------------------------------- words of a scalar
// w >>= s, s < 32 NW: word steps of 1, 2, 4, 8 under selects, then the bit step
template <int NW>
ZK_D void shr_words(uint32_t (&w)[NW], uint32_t s) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const bool on = (s >> (5 + b)) & 1u;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t src = i + (1 << b) < NW ? w[i + (1 << b)] : 0u;
            w[i] = on ? src : w[i];
        }
    }
    const uint32_t bs = s & 31u;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t hi = i + 1 < NW ? w[i + 1] : 0u;
        w[i] = (uint32_t)((((uint64_t)hi << 32) | w[i]) >> bs);
    }
}
// w <<= SH
template <int SH, int NW>
ZK_D void shl_const(uint32_t (&w)[NW]) {
    constexpr int ws = SH / 32, bs = SH % 32;
#pragma unroll
    for (int i = NW - 1; i >= 0; --i) {
        const uint32_t hi = i - ws >= 0 ? w[i - ws] : 0u;
        const uint32_t lo = i - ws - 1 >= 0 ? w[i - ws - 1] : 0u;
        w[i] = bs ? (hi << bs) | (lo >> (32 - bs)) : hi;
    }
}
// v mod 2^bits of a canonical integer (8 words)
template <class Fr>
ZK_D Fr low_bits(const Fr& v, uint32_t bits) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t lo = 32u * i;
        r.v[i] = bits >= lo + 32 ? v.v[i] : bits <= lo ? 0u : v.v[i] & ((1u << (bits - lo)) - 1u);
    }
    return r;
}
// (v mod 2^bits) >> s
template <class Fr>
ZK_D Fr prefix_of(const Fr& v, uint32_t bits, uint32_t s) {
    Fr r = low_bits<Fr>(v, bits);
    shr_words<8>(r.v, s);
    return r;
}
// bit j of a canonical integer; the word is chosen by comparison, not by a run-time index
template <class Fr>
ZK_D uint32_t bit_of(const Fr& e, uint32_t j) {
    uint32_t bit = 0;
#pragma unroll
    for (uint32_t w = 0; w < 8; ++w)
        if ((j >> 5) == w) bit = (e.v[w] >> (j & 31u)) & 1u;
    return bit;
}
// e (canonical) and 3e as 9 words
template <class Fr>
ZK_D void scalar_words(const Fr& e, uint32_t (&E)[9], uint32_t (&T)[9]) {
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        E[i] = e.v[i];
        const uint64_t t = 3ull * e.v[i] + carry;
        T[i] = (uint32_t)t;
        carry = t >> 32;
    }
    E[8] = 0;
    T[8] = (uint32_t)carry;
}
// a digit of weight 2^M or more: bits M + 1 and up of 3e (e itself is below 2^M)
template <uint32_t M>
ZK_D bool naf_too_long(const uint32_t (&T)[9]) {
    uint32_t any = 0;
#pragma unroll
    for (uint32_t i = 0; i < 9; ++i) {
        const uint32_t lo = 32 * i;
        if (lo >= M + 1)
            any |= T[i];
        else if (lo + 32 > M + 1)
            any |= T[i] >> (M + 1 - lo);
    }
    return any != 0;
}

// ---------------------------------------------------------------------------------------------------------------- the embedded curve
// a point in extended coordinates: x = X / Z, y = Y / Z, T = X Y / Z
template <class Fr>
struct Ext {
    Fr X, Y, Z, T;
    ZK_D static Ext identity() { return {Fr::zero(), Fr::one(), Fr::one(), Fr::zero()}; }
};
// The unified law in extended coordinates (Hisil, Wong, Carter, Dawson 2008, section 3.1): X3 / Z3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2)
// and Y3 / Z3 = (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2), the affine law of the reference, for any two pairs of coordinates; a zero
// denominator shows as Z3 = 0.  MIXED: q is affine (q.Z = 1 is not read).
template <bool MIXED, class Fr>
ZK_D Ext<Fr> ext_add(const Ext<Fr>& p, const Ext<Fr>& q, const Fr& ca, const Fr& cd) {
    const Fr A = Fr::mul(p.X, q.X), B = Fr::mul(p.Y, q.Y), C = Fr::mul(cd, Fr::mul(p.T, q.T)), D = MIXED ? p.Z : Fr::mul(p.Z, q.Z);
    const Fr E = Fr::sub(Fr::sub(Fr::mul(Fr::add(p.X, p.Y), Fr::add(q.X, q.Y)), A), B);
    const Fr F = Fr::sub(D, C), G = Fr::add(D, C), H = Fr::sub(B, Fr::mul(ca, A));
    Ext<Fr> r;
    r.X = Fr::mul(E, F);
    r.Y = Fr::mul(G, H);
    r.T = Fr::mul(E, H);
    r.Z = Fr::mul(F, G);
    return r;
}
// (X, Y, Z) of workspace slot `slot`
template <class Fr>
ZK_D void st_slot(void* work, uint64_t slot, const Ext<Fr>& p) {
    st_fr<Fr>(work, 3 * slot, p.X);
    st_fr<Fr>(work, 3 * slot + 1, p.Y);
    st_fr<Fr>(work, 3 * slot + 2, p.Z);
}
// ... read back (an inactive lane: the identity); a zero Z -- no sum in affine coordinates -- raises the flag and is replaced by one,
// which gives values nobody reads
template <class Fr>
ZK_D Ext<Fr> ld_slot(const void* work, uint64_t slot, bool active, uint32_t* flag) {
    Ext<Fr> p = Ext<Fr>::identity();
    if (active) {
        p.X = ld_fr<Fr>(work, 3 * slot);
        p.Y = ld_fr<Fr>(work, 3 * slot + 1);
        p.Z = ld_fr<Fr>(work, 3 * slot + 2);
    }
    if (p.Z.is_zero()) {
        atomicOr(flag, FLAG_DENOM);
        p.Z = Fr::one();
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_poly(zk_gadget_args a, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (k >= a.calls) return;
    const Fr x = ld_input<Fr>(values, a, 0, k, flag), y = ld_input<Fr>(values, a, 1, k, flag), d = ld_input<Fr>(values, a, 3, k, flag);
    Fr acc = Fr::mul(coeff_of<Fr>(a, Q_M, k), Fr::mul(x, y));
    acc = Fr::add(acc, Fr::mul(coeff_of<Fr>(a, Q_L, k), x));
    acc = Fr::add(acc, Fr::mul(coeff_of<Fr>(a, Q_R, k), y));
    acc = Fr::add(acc, coeff_of<Fr>(a, Q_C, k));
    acc = Fr::add(acc, Fr::mul(coeff_of<Fr>(a, Q_4, k), d));
    if (a.pi) acc = Fr::add(acc, ld_fr<Fr>(a.pi, k));
    st_value<Fr>(values, num_vars, a.var0 + k, Fr::mul(acc, Fr::neg(coeff_of<Fr>(a, Q_O, k))));
}

template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_range(zk_gadget_args a, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    const uint32_t vars = a.num_bits / 2;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (g >= a.calls * vars) return;
    const uint64_t k = g / vars;
    const uint32_t j = (uint32_t)(g - k * vars);
    const Fr v = Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag));
    st_value<Fr>(values, num_vars, a.var0 + g, Fr::to_mont(prefix_of<Fr>(v, a.num_bits, a.num_bits - 2 * (j + 1))));
}

template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_logic(zk_gadget_args a, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    const uint32_t quads = a.num_bits / 2;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (g >= a.calls * quads) return;
    const uint64_t k = g / quads;
    const uint32_t i = (uint32_t)(g - k * quads), s = a.num_bits - 2 * (i + 1);
    const Fr x = prefix_of<Fr>(Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag)), a.num_bits, s);
    const Fr y = prefix_of<Fr>(Fr::from_mont(ld_input<Fr>(values, a, 1, k, flag)), a.num_bits, s);
    Fr o;
#pragma unroll
    for (int w = 0; w < 8; ++w) o.v[w] = (a.flags & ZK_GADGET_XOR) ? x.v[w] ^ y.v[w] : x.v[w] & y.v[w];
    const uint64_t v = a.var0 + 4 * g;
    st_value<Fr>(values, num_vars, v, Fr::to_mont(x));
    st_value<Fr>(values, num_vars, v + 1, Fr::to_mont(y));
    st_value<Fr>(values, num_vars, v + 2, Fr::from_u32((x.v[0] & 3u) * (y.v[0] & 3u)));
    st_value<Fr>(values, num_vars, v + 3, Fr::to_mont(o));
}

template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_curve(zk_gadget_args a, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    __shared__ BlockInverseLds<Fr, GT> lds;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = k < a.calls;
    Fr x1y2 = Fr::zero(), y1x2 = Fr::zero(), num_y = Fr::zero(), den_x = Fr::one(), den_y = Fr::one();
    if (active) {
        const Fr x1 = ld_input<Fr>(values, a, 0, k, flag), y1 = ld_input<Fr>(values, a, 1, k, flag);
        const Fr x2 = ld_input<Fr>(values, a, 2, k, flag), y2 = ld_input<Fr>(values, a, 3, k, flag);
        x1y2 = Fr::mul(x1, y2);
        y1x2 = Fr::mul(y1, x2);
        const Fr t = Fr::mul(fr_words<Fr>(a.coeff_d), Fr::mul(x1y2, y1x2));
        den_x = Fr::add(Fr::one(), t);
        den_y = Fr::sub(Fr::one(), t);
        num_y = Fr::sub(Fr::mul(y1, y2), Fr::mul(fr_words<Fr>(a.coeff_a), Fr::mul(x1, x2)));
    }
    Fr den = Fr::mul(den_x, den_y);
    if (den.is_zero()) {                                   // no sum in affine coordinates: the flag, and a value nobody reads
        atomicOr(flag, FLAG_DENOM);
        den = Fr::one();
    }
    const Fr inv = block_inverse(den, lds);
    if (!active) return;
    const uint64_t v = a.var0 + 3 * k;
    st_value<Fr>(values, num_vars, v, x1y2);
    st_value<Fr>(values, num_vars, v + 1, Fr::mul(Fr::add(x1y2, y1x2), Fr::mul(inv, den_y)));
    st_value<Fr>(values, num_vars, v + 2, Fr::mul(num_y, Fr::mul(inv, den_x)));
}

// Fixed base, phase one.  table: 3 M rows, (x, y, x y) of 2^(M-1-i) G for row i (canonical Montgomery).  work: slot i * calls + k holds
// the accumulator BEFORE the digit of row i, i <= M.
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_fixed_walk(zk_gadget_args a, const void* values, void* work, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (k >= a.calls) return;
    uint32_t E[9], T[9];
    scalar_words<Fr>(Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag)), E, T);
    if (naf_too_long<M>(T)) atomicOr(flag, FLAG_SCALAR);
    shl_const<287 - M>(E);                                 // bit M at the top of word 8: row i reads bit M - i there
    shl_const<287 - M>(T);
    const Fr ca = fr_words<Fr>(a.coeff_a), cd = fr_words<Fr>(a.coeff_d);
    Ext<Fr> acc = Ext<Fr>::identity();
#pragma unroll 1
    for (uint32_t i = 0; i < M; ++i) {
        st_slot<Fr>(work, (uint64_t)i * a.calls + k, acc);
        const int digit = (int)(T[8] >> 31) - (int)(E[8] >> 31);
        shl_const<1>(E);
        shl_const<1>(T);
        if (digit != 0) {                                  // + or - the table's point: -(x, y) = (-x, y)
            Ext<Fr> q;
            q.X = ld_fr<Fr>(a.table, 3 * (uint64_t)i);
            q.Y = ld_fr<Fr>(a.table, 3 * (uint64_t)i + 1);
            q.T = ld_fr<Fr>(a.table, 3 * (uint64_t)i + 2);
            if (digit < 0) {
                q.X = Fr::neg(q.X);
                q.T = Fr::neg(q.T);
            }
            acc = ext_add<true, Fr>(acc, q, ca, cd);
        }
    }
    st_slot<Fr>(work, (uint64_t)M * a.calls + k, acc);
}

// Fixed base, phase two: lane g = i * calls + k normalises accumulator i of call k and writes the variables of row i
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_fixed_norm(zk_gadget_args a, void* values, uint64_t num_vars, const void* work, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    __shared__ BlockInverseLds<Fr, GT> lds;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = g < a.calls * (M + 1);
    const Ext<Fr> p = ld_slot<Fr>(work, g, active, flag);
    const Fr zi = block_inverse(p.Z, lds);
    if (!active) return;
    const uint32_t i = (uint32_t)(g / a.calls);
    const uint64_t k = g - (uint64_t)i * a.calls;
    const uint64_t v = a.var0 + k * (4 * M + 3) + 4 * i;
    st_value<Fr>(values, num_vars, v, Fr::mul(p.X, zi));
    st_value<Fr>(values, num_vars, v + 1, Fr::mul(p.Y, zi));
    uint32_t E[9], T[9];
    scalar_words<Fr>(Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag)), E, T);
    shr_words<9>(E, M - i);                                // bit 0: the digit of row i; above it: the digits before
    shr_words<9>(T, M - i);
    const int digit = (int)(T[0] & 1u) - (int)(E[0] & 1u);
    shr_words<9>(E, 1);
    shr_words<9>(T, 1);
    Fr acc;                                                // (3e >> s) - (e >> s): the digits before row i, as a non-negative integer
    uint32_t borrow = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const uint64_t t = (uint64_t)T[w] - E[w] - borrow;
        acc.v[w] = (uint32_t)t;
        borrow = (uint32_t)(t >> 32) & 1u;
    }
    st_value<Fr>(values, num_vars, v + 2, Fr::to_mont(acc));
    if (i < M) {
        Fr xy = Fr::zero();
        if (digit != 0) {
            xy = ld_fr<Fr>(a.table, 3 * (uint64_t)i + 2);
            if (digit < 0) xy = Fr::neg(xy);
        }
        st_value<Fr>(values, num_vars, v + 3, xy);
    }
}

// conditional_select(bit, x, y) into variables v .. v + 3; returns the selected value
template <class Fr>
ZK_D Fr select_values(void* values, uint64_t num_vars, uint64_t v, const Fr& bit, const Fr& x, const Fr& y) {
    const Fr bx = Fr::mul(bit, x), nb = Fr::sub(Fr::one(), bit), nby = Fr::mul(nb, y), out = Fr::add(nby, bx);
    st_value<Fr>(values, num_vars, v, bx);
    st_value<Fr>(values, num_vars, v + 1, nb);
    st_value<Fr>(values, num_vars, v + 2, nby);
    st_value<Fr>(values, num_vars, v + 3, out);
    return out;
}

template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_select(zk_gadget_args a, uint32_t vars, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (k >= a.calls) return;
    const uint64_t v = a.var0 + k * vars;
    if (a.kind == ZK_GADGET_CONST_WITNESS) {
        st_value<Fr>(values, num_vars, v, Fr::neg(coeff_of<Fr>(a, Q_C, k)));
        return;
    }
    if (a.kind == ZK_GADGET_DUMMY) {                       // composer.rs:494-497, in add_input order
        st_value<Fr>(values, num_vars, v, Fr::from_u32(6));
        st_value<Fr>(values, num_vars, v + 1, Fr::one());
        st_value<Fr>(values, num_vars, v + 2, Fr::from_u32(7));
        st_value<Fr>(values, num_vars, v + 3, Fr::neg(Fr::from_u32(20)));
        return;
    }
    const Fr bit = ld_input<Fr>(values, a, 0, k, flag), x = ld_input<Fr>(values, a, 1, k, flag);
    if (a.kind == ZK_GADGET_POINT_NEG) {
        const Fr nx = Fr::neg(x);
        st_value<Fr>(values, num_vars, v, nx);
        select_values<Fr>(values, num_vars, v + 1, bit, nx, x);
        return;
    }
    select_values<Fr>(values, num_vars, v, bit, x, ld_input<Fr>(values, a, 2, k, flag));
    if (a.kind == ZK_GADGET_POINT_SELECT)
        select_values<Fr>(values, num_vars, v + 4, bit, ld_input<Fr>(values, a, 3, k, flag), ld_input<Fr>(values, a, 4, k, flag));
}

template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_is_zero(zk_gadget_args a, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    __shared__ BlockInverseLds<Fr, GT> lds;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = k < a.calls, eq = a.kind == ZK_GADGET_IS_EQ;
    Fr x = Fr::zero();
    if (active) {
        x = ld_input<Fr>(values, a, 0, k, flag);
        if (eq) x = Fr::sub(x, ld_input<Fr>(values, a, 1, k, flag));
    }
    const bool is_zero = x.is_zero();                      // a zero enters the block's product as 1; its y is 1 by definition
    const Fr inv = block_inverse(is_zero ? Fr::one() : x, lds);
    if (!active) return;
    const Fr y = is_zero ? Fr::one() : inv;
    uint64_t v = a.var0 + k * (eq ? 3 : 2);
    if (eq) st_value<Fr>(values, num_vars, v++, x);
    st_value<Fr>(values, num_vars, v, y);
    st_value<Fr>(values, num_vars, v + 1, Fr::sub(Fr::one(), Fr::mul(x, y)));
}

template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_var_bits(zk_gadget_args a, void* values, uint64_t num_vars, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (g >= a.calls * 256) return;
    const uint64_t k = g >> 8;
    const uint32_t j = (uint32_t)(g & 255u);
    const Fr e = Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag));
    const uint64_t v0 = a.var0 + k * (9 * M + 257);
    st_value<Fr>(values, num_vars, v0 + j, bit_of<Fr>(e, j) ? Fr::one() : Fr::zero());
    if (j < M) st_value<Fr>(values, num_vars, v0 + 256 + j, Fr::to_mont(low_bits<Fr>(e, j + 1)));
    if (j == 255) st_value<Fr>(values, num_vars, v0 + 256 + M, Fr::one());
}

// Variable base, phase one.  work: slot s * calls + k holds accumulator s of call k: s = 0 the identity, 2 i + 1 after the doubling of
// iteration i, 2 i + 2 after its addition.
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_var_walk(zk_gadget_args a, const void* values, void* work, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (k >= a.calls) return;
    const Fr e = Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag));
    const Fr px = ld_input<Fr>(values, a, 1, k, flag), py = ld_input<Fr>(values, a, 2, k, flag), pt = Fr::mul(px, py);
    uint32_t E[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) E[i] = e.v[i];
    shl_const<256 - M>(E);                                 // bit M - 1 at the top of word 7: iteration i reads bit M - 1 - i there
    const Fr ca = fr_words<Fr>(a.coeff_a), cd = fr_words<Fr>(a.coeff_d);
    Ext<Fr> acc = Ext<Fr>::identity();
    st_slot<Fr>(work, k, acc);
#pragma unroll 1
    for (uint32_t i = 0; i < M; ++i) {
        acc = ext_add<false, Fr>(acc, acc, ca, cd);
        st_slot<Fr>(work, (uint64_t)(2 * i + 1) * a.calls + k, acc);
        const bool bit = E[7] >> 31;
        shl_const<1>(E);
        Ext<Fr> sel = Ext<Fr>::identity();                 // (bit x, 1 - bit + bit y): the point, or the identity
        if (bit) sel.X = px, sel.Y = py, sel.T = pt;
        acc = ext_add<true, Fr>(acc, sel, ca, cd);
        st_slot<Fr>(work, (uint64_t)(2 * i + 2) * a.calls + k, acc);
    }
}

// Variable base, phase two: lane g = i * calls + k makes the accumulators 2 i, 2 i + 1, 2 i + 2 of call k affine and writes the
// values of iteration i
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_var_norm(zk_gadget_args a, void* values, uint64_t num_vars, const void* work, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    __shared__ BlockInverseLds<Fr, GT> lds;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = g < a.calls * M;
    const uint32_t i = active ? (uint32_t)(g / a.calls) : 0u;
    const uint64_t k = active ? g - (uint64_t)i * a.calls : 0u;
    const Ext<Fr> p0 = ld_slot<Fr>(work, (uint64_t)(2 * i) * a.calls + k, active, flag);
    const Ext<Fr> p1 = ld_slot<Fr>(work, (uint64_t)(2 * i + 1) * a.calls + k, active, flag);
    const Ext<Fr> p2 = ld_slot<Fr>(work, (uint64_t)(2 * i + 2) * a.calls + k, active, flag);
    const Fr z01 = Fr::mul(p0.Z, p1.Z);
    const Fr zi = block_inverse(Fr::mul(z01, p2.Z), lds);
    if (!active) return;
    const Fr i2 = Fr::mul(zi, z01), i1 = Fr::mul(zi, Fr::mul(p0.Z, p2.Z)), i0 = Fr::mul(zi, Fr::mul(p1.Z, p2.Z));
    const Fr rx = Fr::mul(p0.X, i0), ry = Fr::mul(p0.Y, i0), dx = Fr::mul(p1.X, i1), dy = Fr::mul(p1.Y, i1);
    const uint32_t bit = bit_of<Fr>(Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag)), M - 1 - i);
    const Fr sx = bit ? ld_input<Fr>(values, a, 1, k, flag) : Fr::zero();
    const Fr sy = bit ? ld_input<Fr>(values, a, 2, k, flag) : Fr::one();
    const uint64_t u = a.var0 + k * (9 * M + 257) + 257 + M + 8 * (uint64_t)i;
    st_value<Fr>(values, num_vars, u, Fr::mul(rx, ry));
    st_value<Fr>(values, num_vars, u + 1, dx);
    st_value<Fr>(values, num_vars, u + 2, dy);
    st_value<Fr>(values, num_vars, u + 3, sx);
    st_value<Fr>(values, num_vars, u + 4, sy);
    st_value<Fr>(values, num_vars, u + 5, Fr::mul(dx, sy));
    st_value<Fr>(values, num_vars, u + 6, Fr::mul(p2.X, i2));
    st_value<Fr>(values, num_vars, u + 7, Fr::mul(p2.Y, i2));
}

// ---------------------------------------------------------------------------------------------------------------- host side
template <class Cv>
int witness_impl(zk_ctx* c, const zk_gadget_args& a, void* d_values, uint64_t num_vars) {
    constexpr uint32_t M = Cv::FrP::BITS;
    const Shape s = gadget_shape(a.kind, a.num_bits, a.flags, M);
    const int rc = check_args(a, s);
    if (rc) return rc;
    if (a.var0 + a.calls * s.vars > num_vars) return ZK_ERR_BAD_ARG;
    if (s.vars == 0) return ZK_OK;
    if (a.kind == ZK_GADGET_LOOKUP_OUT) return lookup_out_witness(c, a, d_values);
    return run_flagged(c, gadget_work_bytes(a.kind, M, a.calls), [&](uint32_t* d_flag, void* work) -> int {
        // one kernel over `lanes` lanes under its own profile scope
        auto launch = [&](const char* name, auto kernel, uint64_t lanes, auto... args) {
            ProfScope ps(c, name);
            hipLaunchKernelGGL(kernel, dim3(blocks_of(lanes, GT)), dim3(GT), 0, c->stream, a, args...);
        };
        switch (a.kind) {
        case ZK_GADGET_POLY: launch("gadget_w_poly", gadget_w_poly<Cv>, a.calls, d_values, num_vars, d_flag); break;
        case ZK_GADGET_RANGE: launch("gadget_w_range", gadget_w_range<Cv>, a.calls * s.vars, d_values, num_vars, d_flag); break;
        case ZK_GADGET_LOGIC: launch("gadget_w_logic", gadget_w_logic<Cv>, a.calls * (a.num_bits / 2), d_values, num_vars, d_flag); break;
        case ZK_GADGET_CURVE_ADD: launch("gadget_w_curve", gadget_w_curve<Cv>, a.calls, d_values, num_vars, d_flag); break;
        case ZK_GADGET_FIXED_BASE:
            launch("gadget_w_fixed_walk", gadget_w_fixed_walk<Cv>, a.calls, d_values, work, d_flag);
            launch("gadget_w_fixed_norm", gadget_w_fixed_norm<Cv>, a.calls * (M + 1), d_values, num_vars, work, d_flag);
            break;
        case ZK_GADGET_IS_ZERO:
        case ZK_GADGET_IS_EQ: launch("gadget_w_is_zero", gadget_w_is_zero<Cv>, a.calls, d_values, num_vars, d_flag); break;
        case ZK_GADGET_VAR_BASE:
            launch("gadget_w_var_bits", gadget_w_var_bits<Cv>, a.calls * 256, d_values, num_vars, d_flag);
            launch("gadget_w_var_walk", gadget_w_var_walk<Cv>, a.calls, d_values, work, d_flag);
            launch("gadget_w_var_norm", gadget_w_var_norm<Cv>, a.calls * M, d_values, num_vars, work, d_flag);
            break;
        default:                                           // the constant witness, the dummy constants, the selects, the point negation
            launch("gadget_w_select", gadget_w_select<Cv>, a.calls, s.vars, d_values, num_vars, d_flag);
            break;
        }
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_gadget_witness_dev(zk_ctx* c, int curve_id, const void* args, void* d_values, size_t num_vars) {
    if (!c || !args || !zk_curve_ok(curve_id) || !d_values) return ZK_ERR_BAD_ARG;
    zk_gadget_args a;
    memcpy(&a, args, sizeof a);
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return witness_impl<decltype(cv)>(c, a, d_values, (uint64_t)num_vars); });
}
