// The circuit builder on the device: what `StandardComposer` (plonk-core/src/constraint_system/) holds after a gadget was called B
// times in a row -- rows, variable ids, selector values, the `add_variable_to_map` calls in call order -- and the values of the
// variables those calls create, for the arithmetic family (arithmetic.rs:103-168, composer.rs:269-350, boolean.rs:25-51), range_gate
// (range.rs:27-195), xor_gate / and_gate (logic.rs:36-345), point_addition_gate (ecc/curve_addition/variable_base_gate.rs:24-93) and
// fixed_base_scalar_mul (ecc/scalar_mul/fixed_base.rs:51-160).  A SEGMENT is B calls of one gadget with the same parameters; every
// gadget has a fixed shape per call (R rows, V new variables, I insertions: gadget_shape), so call k owns rows row0 + k R ...,
// variables var0 + k V ... and insertions k I ... and no kernel loops over calls or rows on the host.
//
//   gadget_layout        one lane per (call, row): the four variable ids and the twelve selector values of the row; input ids checked
//   gadget_insertions    one lane per (call, insertion): (variable, wire << 30 | row) -- independent of the padded size
//   gadget_w_poly        one lane per call: the computed output (q_m a b + q_l a + q_r b + q_c + q_4 d + pi) (-q_o)
//   gadget_w_range       one lane per (call, accumulator j): (v mod 2^bits) >> (bits - 2 (j + 1)) of the canonical integer v
//   gadget_w_logic       one lane per (call, quad): both input prefixes, their product quad, the prefix of a ^ b or a & b
//   gadget_w_curve       one lane per call: x1 y2 and the twisted Edwards sum; ONE field inversion per block (product scans in LDS)
//   gadget_w_fixed_walk  one lane per call: the width-2 NAF digits in closed form (digit of weight 2^j = bit j+1 of 3e - bit j+1 of e),
//                        a running sum in extended coordinates against the segment's table of affine multiples, the M + 1
//                        projective accumulators stored to the call's workspace
//   gadget_w_fixed_norm  one lane per (call, row): normalises with one shared inversion per block; writes acc_x, acc_y, xy_alpha and
//                        the scalar accumulator (3e >> s) - (e >> s)
// Values are canonical Montgomery Fr (field.cuh), what `assign` and the circuit check expect; the canonical integer of an input is one
// Montgomery product, prefixes are shifts and masks on its words with compile-time word indices (no array is indexed at run time).
// Errors are one flag word, OR-ed, read back once per call: an input id that is not below the segment's var0 (an undefined variable), a
// scalar whose NAF has more than M digits (the reference asserts there), a zero denominator of the group law.  Every kernel guards
// its own addresses: a refused call leaves unspecified values, never an access outside the buffers.
//
// Working memory: one allocation per call, freed on every path; 256 bytes, + 96 (M + 1) B for a fixed-base witness.  No buffer of the
// ctx is used, so both calls run inside an open deferred round.  The kinds after ZK_GADGET_FIXED_BASE are dispatched to gadgets_ext.hip;
// what the two units share is defined once in gadget_common.cuh.
#include "gadget_common.cuh"

namespace {

// the four variable ids (Left, Right, Output, Fourth) of row r of call k
ZK_D void row_ids(const zk_gadget_args& a, const Shape& s, uint32_t m_bits, uint64_t k, uint32_t r, uint32_t (&id)[4]) {
    const uint32_t v0 = (uint32_t)(a.var0 + k * s.vars);
    id[0] = id[1] = id[2] = id[3] = 0;
    switch (a.kind) {
    case ZK_GADGET_POLY:
        id[0] = input_id(a, 0, k);
        id[1] = input_id(a, 1, k);
        id[2] = (a.flags & ZK_GADGET_COMPUTE_OUT) ? v0 : input_id(a, 2, k);
        id[3] = input_id(a, 3, k);
        break;
    case ZK_GADGET_RANGE: {
        // quad position i of the call sits on row i / 4, wire Fourth, Output, Right, Left for i % 4 = 0 .. 3 (range.rs:30-57); the
        // first `pad` positions hold the zero variable, the last row the final accumulator alone (its other cells are pushed unmapped)
        const uint32_t g = s.rows - 2, pad = 1 + 4 * g - a.num_bits / 2;
        if (r <= g) {
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t i = 4 * r + (3 - w);
                id[w] = (i <= 4 * g && i >= pad) ? v0 + i - pad : 0u;
            }
        } else {
            id[0] = v0 + s.vars - 1;
            id[1] = input_id(a, 0, k);
        }
        break;
    }
    case ZK_GADGET_LOGIC: {
        // row r holds the prefixes after quad r - 1 and the product of quad r (logic.rs:73-235)
        const uint32_t q = a.num_bits / 2;
        if (r > 0) {
            id[0] = v0 + 4 * (r - 1);
            id[1] = v0 + 4 * (r - 1) + 1;
            id[3] = v0 + 4 * (r - 1) + 3;
        }
        if (r < q) id[2] = v0 + 4 * r + 2;
        break;
    }
    case ZK_GADGET_CURVE_ADD:
        if (r == 0) {
#pragma unroll
            for (int w = 0; w < 4; ++w) id[w] = input_id(a, w, k);
        } else {
            id[0] = v0 + 1;
            id[1] = v0 + 2;
            id[3] = v0;
        }
        break;
    case ZK_GADGET_FIXED_BASE:
        if (r < 3) {
            id[0] = id[1] = id[2] = v0 + r;
        } else if (r < 3 + m_bits) {
            const uint32_t i = r - 3;
            id[0] = v0 + 4 * i;
            id[1] = v0 + 4 * i + 1;
            id[2] = v0 + 4 * i + 3;
            id[3] = v0 + 4 * i + 2;
        } else if (r == 3 + m_bits) {
            id[0] = v0 + 4 * m_bits;
            id[1] = v0 + 4 * m_bits + 1;
            id[3] = v0 + 4 * m_bits + 2;
        } else {
            id[0] = v0 + 4 * m_bits + 2;
            id[1] = input_id(a, 0, k);
        }
        break;
    default: break;
    }
}

// ---------------------------------------------------------------------------------------------------------------- layout
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_layout(zk_gadget_args a, Shape s, uint32_t* ids, SelPtrs sel, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const uint64_t total = a.calls * s.rows;
    if (g >= total) return;
    const uint64_t k = g / s.rows;
    const uint32_t r = (uint32_t)(g - k * s.rows);
    if (r == 0) {                                          // an input that is no variable defined before the segment
        bool bad = false;
#pragma unroll
        for (int w = 0; w < 4; ++w) bad = bad || input_id(a, w, k) >= a.var0;
        if (bad) atomicOr(flag, FLAG_INPUT);
    }
    uint32_t id[4];
    row_ids(a, s, M, k, r, id);
#pragma unroll
    for (int w = 0; w < 4; ++w) ids[(uint64_t)w * total + g] = id[w];
    Fr q[N_SEL];
#pragma unroll
    for (int j = 0; j < N_SEL; ++j) q[j] = Fr::zero();
    const Fr one = Fr::one(), minus_one = Fr::neg(Fr::one());
    switch (a.kind) {
    case ZK_GADGET_POLY:
#pragma unroll
        for (int j = 0; j < 6; ++j) q[j] = coeff_of<Fr>(a, j, k);
        q[Q_ARITH] = one;
        break;
    case ZK_GADGET_RANGE:
        if (r + 2 < s.rows) q[Q_RANGE] = one;
        if (r + 1 == s.rows) {                             // assert_equal(last accumulator, witness)
            q[Q_L] = one;
            q[Q_R] = minus_one;
            q[Q_ARITH] = one;
        }
        break;
    case ZK_GADGET_LOGIC:
        if (r + 1 < s.rows) q[Q_C] = q[Q_LOGIC] = (a.flags & ZK_GADGET_XOR) ? minus_one : one;
        break;
    case ZK_GADGET_CURVE_ADD:
        if (r == 0) q[Q_VAR] = one;
        break;
    case ZK_GADGET_FIXED_BASE:
        if (r < 3) {                                       // constrain_to_constant: acc_x = 0, acc_y = 1, scalar accumulator = 0
            q[Q_L] = one;
            q[Q_ARITH] = one;
            if (r == 1) q[Q_C] = minus_one;
        } else if (r < 3 + M) {
            const uint64_t i = r - 3;
            q[Q_L] = ld_fr<Fr>(a.table, 3 * i);
            q[Q_R] = ld_fr<Fr>(a.table, 3 * i + 1);
            q[Q_C] = ld_fr<Fr>(a.table, 3 * i + 2);
            q[Q_FIXED] = one;
        } else {
            q[Q_ARITH] = one;
            if (r == 4 + M) {
                q[Q_L] = one;
                q[Q_R] = minus_one;
            }
        }
        break;
    default: break;
    }
#pragma unroll
    for (int j = 0; j < N_SEL; ++j) st_fr<Fr>(sel.p[j], g, q[j]);
}

// the t-th `add_variable_to_map` call of call k
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_insertions(zk_gadget_args a, Shape s, uint32_t* ins_var, uint32_t* ins_rec) {
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (g >= a.calls * s.ins) return;
    const uint64_t k = g / s.ins;
    const uint32_t t = (uint32_t)(g - k * s.ins);
    const uint32_t v0 = (uint32_t)(a.var0 + k * s.vars);
    uint32_t var = 0, wire = t & 3u, r = t >> 2;
    bool from_row = true;                                  // Left, Right, Output, Fourth of row t / 4 (add_variables_to_map)
    if (a.kind == ZK_GADGET_RANGE) {
        const uint32_t g4 = 4 * (s.rows - 2), pad = 1 + g4 - a.num_bits / 2;
        if (t <= g4) {                                     // add_wire(i, .) in the order of i
            from_row = false;
            wire = 3 - (t & 3u);
            var = t >= pad ? v0 + t - pad : 0u;
        } else {
            wire = t - g4 - 1;
            r = s.rows - 1;
        }
    } else if (a.kind == ZK_GADGET_LOGIC) {
        from_row = false;
        const uint32_t q = a.num_bits / 2;
        if (t < 3) {                                       // the zero variable on Left, Right, Fourth of the first row
            wire = t == 2 ? 3u : t;
            r = 0;
        } else if (t < 3 + 4 * q) {                        // Left(n), Right(n), Fourth(n), then Output(n - 1)
            const uint32_t i = (t - 3) >> 2, j = (t - 3) & 3u;
            wire = j == 2 ? 3u : j == 3 ? 2u : j;
            var = v0 + 4 * i + (j == 2 ? 3u : j == 3 ? 2u : j);
            r = j == 3 ? i : i + 1;
        } else {
            wire = 2;
            r = q;
        }
    }
    if (from_row) {
        uint32_t id[4];
        row_ids(a, s, M, k, r, id);
        var = pick4(id, wire);
    }
    ins_var[g] = var;
    ins_rec[g] = (wire << REC_SHIFT) | (uint32_t)(a.row0 + k * s.rows + r);
}

// ---------------------------------------------------------------------------------------------------------------- witness helpers
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
// (v mod 2^bits) >> s as a canonical integer (v: canonical, 8 words)
template <class Fr>
ZK_D Fr prefix_of(const Fr& v, uint32_t bits, uint32_t s) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t lo = 32u * i;
        w[i] = bits >= lo + 32 ? v.v[i] : bits <= lo ? 0u : v.v[i] & ((1u << (bits - lo)) - 1u);
    }
    shr_words<8>(w, s);
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = w[i];
    return r;
}
// ---------------------------------------------------------------------------------------------------------------- witness kernels
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
    __shared__ Fr pre[GT];
    __shared__ Fr suf[GT];
    __shared__ Fr inv_total;
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
    const Fr inv = block_inverse<Fr>(den, pre, suf, &inv_total);
    if (!active) return;
    const uint64_t v = a.var0 + 3 * k;
    st_value<Fr>(values, num_vars, v, x1y2);
    st_value<Fr>(values, num_vars, v + 1, Fr::mul(Fr::add(x1y2, y1x2), Fr::mul(inv, den_y)));
    st_value<Fr>(values, num_vars, v + 2, Fr::mul(num_y, Fr::mul(inv, den_x)));
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
template <int SH>
ZK_D void shl_const(uint32_t (&w)[9]) {
    constexpr int ws = SH / 32, bs = SH % 32;
#pragma unroll
    for (int i = 8; i >= 0; --i) {
        const uint32_t hi = i - ws >= 0 ? w[i - ws] : 0u;
        const uint32_t lo = i - ws - 1 >= 0 ? w[i - ws - 1] : 0u;
        w[i] = bs ? (hi << bs) | (lo >> (32 - bs)) : hi;
    }
}

// Phase one.  table: 3 M rows, (x, y, x y) of 2^(M-1-i) G for row i (canonical Montgomery).  work: slot i * calls + k holds the
// accumulator BEFORE the digit of row i as (X, Y, Z), i <= M.  The sum is the unified law in extended coordinates (Hisil, Wong,
// Carter, Dawson 2008, section 3.1, mixed: Z2 = 1, T2 = x2 y2): X3 / Z3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2) and
// Y3 / Z3 = (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2), the affine law of the reference; a zero denominator shows as Z = 0 in phase two.
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
    Fr X = Fr::zero(), Y = Fr::one(), Z = Fr::one(), Tt = Fr::zero();
#pragma unroll 1
    for (uint32_t i = 0; i < M; ++i) {
        const uint64_t slot = 3 * ((uint64_t)i * a.calls + k);
        st_fr<Fr>(work, slot, X);
        st_fr<Fr>(work, slot + 1, Y);
        st_fr<Fr>(work, slot + 2, Z);
        const int digit = (int)(T[8] >> 31) - (int)(E[8] >> 31);
        shl_const<1>(E);
        shl_const<1>(T);
        if (digit != 0) {
            Fr x2 = ld_fr<Fr>(a.table, 3 * (uint64_t)i), t2 = ld_fr<Fr>(a.table, 3 * (uint64_t)i + 2);
            const Fr y2 = ld_fr<Fr>(a.table, 3 * (uint64_t)i + 1);
            if (digit < 0) {
                x2 = Fr::neg(x2);
                t2 = Fr::neg(t2);
            }
            const Fr A = Fr::mul(X, x2), B = Fr::mul(Y, y2), C = Fr::mul(cd, Fr::mul(Tt, t2));
            const Fr Ee = Fr::sub(Fr::sub(Fr::mul(Fr::add(X, Y), Fr::add(x2, y2)), A), B);
            const Fr F = Fr::sub(Z, C), G = Fr::add(Z, C), H = Fr::sub(B, Fr::mul(ca, A));
            X = Fr::mul(Ee, F);
            Y = Fr::mul(G, H);
            Tt = Fr::mul(Ee, H);
            Z = Fr::mul(F, G);
        }
    }
    const uint64_t slot = 3 * ((uint64_t)M * a.calls + k);
    st_fr<Fr>(work, slot, X);
    st_fr<Fr>(work, slot + 1, Y);
    st_fr<Fr>(work, slot + 2, Z);
}

// Phase two: lane g = i * calls + k normalises accumulator i of call k and writes the variables of row i
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_fixed_norm(zk_gadget_args a, void* values, uint64_t num_vars, const void* work, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    __shared__ Fr pre[GT];
    __shared__ Fr suf[GT];
    __shared__ Fr inv_total;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = g < a.calls * (M + 1);
    Fr X = Fr::zero(), Y = Fr::one(), Z = Fr::one();
    if (active) {
        X = ld_fr<Fr>(work, 3 * g);
        Y = ld_fr<Fr>(work, 3 * g + 1);
        Z = ld_fr<Fr>(work, 3 * g + 2);
    }
    if (Z.is_zero()) {
        atomicOr(flag, FLAG_DENOM);
        Z = Fr::one();
    }
    const Fr zi = block_inverse<Fr>(Z, pre, suf, &inv_total);
    if (!active) return;
    const uint32_t i = (uint32_t)(g / a.calls);
    const uint64_t k = g - (uint64_t)i * a.calls;
    const uint64_t v = a.var0 + k * (4 * M + 3) + 4 * i;
    st_value<Fr>(values, num_vars, v, Fr::mul(X, zi));
    st_value<Fr>(values, num_vars, v + 1, Fr::mul(Y, zi));
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

// ---------------------------------------------------------------------------------------------------------------- host side
// what both entry points refuse before anything is launched
int check_args(const zk_gadget_args& a, const Shape& s) {
    if (a.kind > ZK_GADGET_FIXED_BASE || a.calls == 0 || s.rows == 0) return ZK_ERR_BAD_ARG;
    if ((a.kind == ZK_GADGET_RANGE || a.kind == ZK_GADGET_LOGIC) && (a.num_bits < 2 || a.num_bits > 256 || (a.num_bits & 1u))) return ZK_ERR_BAD_ARG;
    const int need = a.kind == ZK_GADGET_CURVE_ADD ? 4 : a.kind == ZK_GADGET_RANGE || a.kind == ZK_GADGET_FIXED_BASE ? 1 : 2;
    for (int w = 0; w < need; ++w)
        if (!a.inputs[w]) return ZK_ERR_BAD_ARG;
    if (a.kind == ZK_GADGET_POLY && !(a.flags & ZK_GADGET_COMPUTE_OUT) && !a.inputs[2]) return ZK_ERR_BAD_ARG;
    if (a.kind == ZK_GADGET_FIXED_BASE && !a.table) return ZK_ERR_BAD_ARG;
    return check_extent(a, s);
}

template <class Cv>
int layout_impl(zk_ctx* c, const zk_gadget_args& a, uint32_t* d_ids, void* const* d_sel, uint32_t* d_ins_var, uint32_t* d_ins_rec) {
    const Shape s = gadget_shape(a.kind, a.num_bits, a.flags, Cv::FrP::BITS);
    const int rc = check_args(a, s);
    if (rc) return rc;
    SelPtrs sel;
    for (int j = 0; j < N_SEL; ++j) sel.p[j] = d_sel[j];
    return run_flagged<Cv>(c, 0, [&](uint32_t* d_flag, void*) -> int {
        ProfScope ps(c, "gadget_layout");
        hipLaunchKernelGGL(gadget_layout<Cv>, dim3(blocks_of(a.calls * s.rows, GT)), dim3(GT), 0, c->stream, a, s, d_ids, sel, d_flag);
        hipLaunchKernelGGL(gadget_insertions<Cv>, dim3(blocks_of(a.calls * s.ins, GT)), dim3(GT), 0, c->stream, a, s, d_ins_var, d_ins_rec);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

template <class Cv>
int witness_impl(zk_ctx* c, const zk_gadget_args& a, void* d_values, uint64_t num_vars) {
    constexpr uint32_t M = Cv::FrP::BITS;
    const Shape s = gadget_shape(a.kind, a.num_bits, a.flags, M);
    const int rc = check_args(a, s);
    if (rc) return rc;
    if (a.var0 + a.calls * s.vars > num_vars) return ZK_ERR_BAD_ARG;
    if (s.vars == 0) return ZK_OK;
    const size_t work_bytes = gadget_work_bytes(a.kind, M, a.calls);
    return run_flagged<Cv>(c, work_bytes, [&](uint32_t* d_flag, void* work) -> int {
        hipStream_t st = c->stream;
        switch (a.kind) {
        case ZK_GADGET_POLY: {
            ProfScope ps(c, "gadget_w_poly");
            hipLaunchKernelGGL(gadget_w_poly<Cv>, dim3(blocks_of(a.calls, GT)), dim3(GT), 0, st, a, d_values, num_vars, d_flag);
            break;
        }
        case ZK_GADGET_RANGE: {
            ProfScope ps(c, "gadget_w_range");
            hipLaunchKernelGGL(gadget_w_range<Cv>, dim3(blocks_of(a.calls * s.vars, GT)), dim3(GT), 0, st, a, d_values, num_vars, d_flag);
            break;
        }
        case ZK_GADGET_LOGIC: {
            ProfScope ps(c, "gadget_w_logic");
            hipLaunchKernelGGL(gadget_w_logic<Cv>, dim3(blocks_of(a.calls * (a.num_bits / 2), GT)), dim3(GT), 0, st, a, d_values, num_vars, d_flag);
            break;
        }
        case ZK_GADGET_CURVE_ADD: {
            ProfScope ps(c, "gadget_w_curve");
            hipLaunchKernelGGL(gadget_w_curve<Cv>, dim3(blocks_of(a.calls, GT)), dim3(GT), 0, st, a, d_values, num_vars, d_flag);
            break;
        }
        default: {
            {
                ProfScope ps(c, "gadget_w_fixed_walk");
                hipLaunchKernelGGL(gadget_w_fixed_walk<Cv>, dim3(blocks_of(a.calls, GT)), dim3(GT), 0, st, a, (const void*)d_values, work, d_flag);
            }
            ProfScope ps(c, "gadget_w_fixed_norm");
            hipLaunchKernelGGL(gadget_w_fixed_norm<Cv>, dim3(blocks_of(a.calls * (M + 1), GT)), dim3(GT), 0, st, a, d_values, num_vars,
                               (const void*)work, d_flag);
            break;
        }
        }
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_gadget_shape(int kind, int curve_id, uint32_t num_bits, uint32_t flags, size_t calls, uint32_t* rows, uint32_t* vars, uint32_t* insertions,
                    size_t* work_bytes) {
    if (kind < 0 || kind > (int)LAST_KIND || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if ((kind == ZK_GADGET_RANGE || kind == ZK_GADGET_LOGIC) && (num_bits < 2 || num_bits > 256 || (num_bits & 1u))) return ZK_ERR_BAD_ARG;
    const uint32_t m_bits = zk_on_curve(curve_id, 0u, [&](auto cv) { return (uint32_t) decltype(cv)::FrP::BITS; });
    const Shape s = gadget_shape((uint32_t)kind, num_bits, flags, m_bits);
    if (s.rows == 0) return ZK_ERR_BAD_ARG;                       // a number between the kinds that names none
    if (rows) *rows = s.rows;
    if (vars) *vars = s.vars;
    if (insertions) *insertions = s.ins;
    if (work_bytes) *work_bytes = 256 + gadget_work_bytes((uint32_t)kind, m_bits, calls);
    return ZK_OK;
}

int zk_gadget_layout_dev(zk_ctx* c, int curve_id, const void* args, void* d_wire_ids, void* const* d_selectors, void* d_ins_var, void* d_ins_rec) {
    if (!c || !args || !zk_curve_ok(curve_id) || !d_wire_ids || !d_selectors || !d_ins_var || !d_ins_rec) return ZK_ERR_BAD_ARG;
    for (int j = 0; j < N_SEL; ++j)
        if (!d_selectors[j]) return ZK_ERR_BAD_ARG;
    zk_gadget_args a;
    memcpy(&a, args, sizeof a);
    Guard g(c);
    if (a.kind > ZK_GADGET_FIXED_BASE) return gadget_ext_layout(c, curve_id, a, (uint32_t*)d_wire_ids, d_selectors, (uint32_t*)d_ins_var, (uint32_t*)d_ins_rec);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return layout_impl<decltype(cv)>(c, a, (uint32_t*)d_wire_ids, d_selectors, (uint32_t*)d_ins_var, (uint32_t*)d_ins_rec);
    });
}

int zk_gadget_witness_dev(zk_ctx* c, int curve_id, const void* args, void* d_values, size_t num_vars) {
    if (!c || !args || !zk_curve_ok(curve_id) || !d_values) return ZK_ERR_BAD_ARG;
    zk_gadget_args a;
    memcpy(&a, args, sizeof a);
    Guard g(c);
    if (a.kind > ZK_GADGET_FIXED_BASE) return gadget_ext_witness(c, curve_id, a, d_values, (uint64_t)num_vars);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return witness_impl<decltype(cv)>(c, a, d_values, (uint64_t)num_vars); });
}
