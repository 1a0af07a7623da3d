// The device composer, second unit: the gadget kinds after ZK_GADGET_FIXED_BASE -- add_witness_to_circuit_description
// (composer.rs:192-196), is_zero_with_output / is_eq_with_output (composer.rs:355-392), conditional_select (composer.rs:404-433),
// conditional_point_select / conditional_point_neg (ecc/mod.rs:145-182), variable_base_scalar_mul (ecc/scalar_mul/variable_base.rs:
// 27-95) and lookup_gate (lookup.rs:18-65) -- and the blocks of a lookup table (lookup/lookup_table.rs:94-152).  The segment
// definition, the shape table and the helpers are those of gadgets.hip (gadget_common.cuh); every kind here maps all four cells of
// every row, row by row.
//
//   gadget_layout_ext      one lane per (call, row): the four variable ids and the twelve selector values of the row; input ids checked
//   gadget_insertions_ext  one lane per (call, insertion): Left, Right, Output, Fourth of row t / 4
//   gadget_w_select        one lane per call: the constant witness, the four values of a select, the eight of a point select, the
//                          five of a point negation -- each the product with -q_o that arithmetic.rs:144-155 computes
//   gadget_w_is_zero       one lane per call: (a - b,) y = 1 / a or 1, b = 1 - a y; ONE field inversion per block, a zero input
//                          enters the block's product as 1
//   gadget_w_var_bits      one lane per (call, j < 256): bit j of the canonical scalar e, the accumulator e mod 2^(j+1) for j < M, the
//                          constant one of the identity
//   gadget_w_var_walk      one lane per call: 2 M unified additions in extended coordinates (doubling, then the addition of the
//                          selected point (bit x, 1 - bit + bit y)), the 2 M + 1 projective accumulators stored to the workspace;
//                          the scalar's bits leave the top of a word array that is shifted with compile-time indices
//   gadget_w_var_norm      one lane per (call, iteration): the three accumulators of the iteration made affine with one inversion
//                          per block (through the product of their Z), the eight values of the iteration
//   lookup_table_fill      one lane per row of an insert_multi_* block
// A zero Z is a zero denominator of the affine law the reference computes with: the flag word, ZK_ERR_BAD_ARG.  Working memory of a
// VAR_BASE witness: 256 + 96 (2 M + 1) calls bytes, one allocation, freed on every path.
#include "gadget_common.cuh"

namespace {

constexpr int MAX_INPUTS = 5;

ZK_HD int inputs_needed(uint32_t kind) {
    switch (kind) {
    case ZK_GADGET_IS_ZERO: return 1;
    case ZK_GADGET_IS_EQ: return 2;
    case ZK_GADGET_SELECT: return 3;
    case ZK_GADGET_POINT_SELECT: return 5;
    case ZK_GADGET_POINT_NEG: return 2;
    case ZK_GADGET_VAR_BASE: return 3;
    case ZK_GADGET_LOOKUP: return 3;
    default: return 0;
    }
}

// the selectors a row of these kinds can carry, as small integers: q_m, q_l, q_r, q_4, q_c in {-1, 0, 1}, q_o = -1 on every arithmetic
// row with an output, pow2 >= 0: q_l = 2^pow2
struct RowSel {
    int m = 0, l = 0, r = 0, o = 0, q4 = 0, c = 0, pow2 = -1;
    bool arith = false, var_add = false, lookup = false;
};

// rows of conditional_select(bit, x, y) with new variables v .. v + 3 (composer.rs:404-433); t = 0 .. 3
ZK_D void select_row(uint32_t t, uint32_t bit, uint32_t x, uint32_t y, uint32_t v, uint32_t (&id)[4], RowSel& q) {
    q.arith = true;
    q.o = -1;
    if (t == 0) {
        id[0] = bit, id[1] = x, id[2] = v;
        q.m = 1;
    } else if (t == 1) {
        id[0] = bit, id[2] = v + 1;
        q.l = -1, q.c = 1;
    } else if (t == 2) {
        id[0] = v + 1, id[1] = y, id[2] = v + 2;
        q.m = 1;
    } else {
        id[0] = v + 2, id[1] = v, id[2] = v + 3;
        q.l = 1, q.r = 1;
    }
}

// the four variable ids (Left, Right, Output, Fourth) and the selectors of row r of call k
ZK_D void row_ext(const zk_gadget_args& a, const Shape& s, uint32_t M, uint64_t k, uint32_t r, uint32_t (&id)[4], RowSel& q) {
    const uint32_t v0 = (uint32_t)(a.var0 + k * s.vars);
    id[0] = id[1] = id[2] = id[3] = 0;
    switch (a.kind) {
    case ZK_GADGET_CONST_WITNESS:
        id[0] = id[1] = id[2] = v0;
        q.arith = true;
        q.l = 1;                                           // q_c: the segment's coefficient
        break;
    case ZK_GADGET_IS_ZERO:
    case ZK_GADGET_IS_EQ: {
        uint32_t x = input_id(a, 0, k), y = v0, b = v0 + 1, t = r;
        q.arith = true;
        q.o = -1;
        if (a.kind == ZK_GADGET_IS_EQ) {
            if (r == 0) {                                  // difference = a - b
                id[0] = x, id[1] = input_id(a, 1, k), id[2] = v0;
                q.l = 1, q.r = -1;
                break;
            }
            x = v0, y = v0 + 1, b = v0 + 2, t = r - 1;
        }
        id[0] = x;
        q.m = 1;
        if (t == 0) {                                      // a b = 0
            id[1] = b;
        } else {                                           // a y + b - 1 = 0
            id[1] = y, id[3] = b;
            q.q4 = 1, q.c = -1;
        }
        break;
    }
    case ZK_GADGET_SELECT: select_row(r, input_id(a, 0, k), input_id(a, 1, k), input_id(a, 2, k), v0, id, q); break;
    case ZK_GADGET_POINT_SELECT:
        if (r < 4)
            select_row(r, input_id(a, 0, k), input_id(a, 1, k), input_id(a, 2, k), v0, id, q);
        else
            select_row(r - 4, input_id(a, 0, k), input_id(a, 3, k), input_id(a, 4, k), v0 + 4, id, q);
        break;
    case ZK_GADGET_POINT_NEG:
        if (r == 0) {                                      // -x
            id[0] = input_id(a, 1, k), id[2] = v0;
            q.arith = true;
            q.l = -1, q.o = -1;
        } else {
            select_row(r - 1, input_id(a, 0, k), v0, input_id(a, 1, k), v0 + 1, id, q);
        }
        break;
    case ZK_GADGET_VAR_BASE: {
        const uint32_t one = v0 + 256 + M;
        if (r < 2 * M) {                                   // scalar_decomposition: boolean_gate(bit j), then the accumulator
            const uint32_t j = r >> 1;
            q.arith = true;
            q.o = -1;
            if (!(r & 1u)) {
                id[0] = id[1] = id[2] = v0 + j;
                q.m = 1;
            } else {
                id[0] = v0 + j, id[1] = j ? v0 + 255 + j : 0u, id[2] = v0 + 256 + j;
                q.pow2 = (int)j, q.r = 1;
            }
        } else if (r == 2 * M) {                           // assert_equal(last accumulator, scalar)
            id[0] = v0 + 255 + M, id[1] = input_id(a, 0, k);
            q.arith = true;
            q.l = 1, q.r = -1;
        } else if (r == 2 * M + 1) {                       // Point::identity: the constant one
            id[0] = id[1] = id[2] = one;
            q.arith = true;
            q.l = 1, q.c = -1;
        } else {
            const uint32_t t = r - (2 * M + 2), i = t / 6, st = t - 6 * i;
            const uint32_t u = v0 + 257 + M + 8 * i, bit = v0 + (M - 1 - i);
            const uint32_t rx = i ? u - 2 : 0u, ry = i ? u - 1 : one;
            if (st == 0) {                                 // point_addition_gate(result, result)
                id[0] = id[2] = rx, id[1] = id[3] = ry;
                q.var_add = true;
            } else if (st == 1) {
                id[0] = u + 1, id[1] = u + 2, id[3] = u;
            } else if (st == 2) {                          // conditional_select_zero(bit, x)
                id[0] = bit, id[1] = input_id(a, 1, k), id[2] = u + 3;
                q.arith = true;
                q.m = 1, q.o = -1;
            } else if (st == 3) {                          // conditional_select_one(bit, y)
                id[0] = bit, id[1] = input_id(a, 2, k), id[2] = u + 4;
                q.arith = true;
                q.m = 1, q.l = -1, q.o = -1, q.c = 1;
            } else if (st == 4) {                          // point_addition_gate(result, selected)
                id[0] = u + 1, id[1] = u + 2, id[2] = u + 3, id[3] = u + 4;
                q.var_add = true;
            } else {
                id[0] = u + 6, id[1] = u + 7, id[3] = u + 5;
            }
        }
        break;
    }
    case ZK_GADGET_LOOKUP:
#pragma unroll
        for (int w = 0; w < 4; ++w) id[w] = input_id(a, w, k);
        q.lookup = true;
        break;
    default: break;
    }
}

template <class Fr>
ZK_D Fr small(int v) { return v == 0 ? Fr::zero() : v > 0 ? Fr::one() : Fr::neg(Fr::one()); }
// 2^j (j < 256, below the modulus) in Montgomery form; the word is chosen by comparison, not by a run-time index
template <class Fr>
ZK_D Fr pow2_mont(uint32_t j) {
    Fr c;
#pragma unroll
    for (uint32_t w = 0; w < 8; ++w) c.v[w] = (j >> 5) == w ? 1u << (j & 31u) : 0u;
    return Fr::to_mont(c);
}

// ---------------------------------------------------------------------------------------------------------------- layout
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_layout_ext(zk_gadget_args a, Shape s, uint32_t* ids, SelPtrs sel, uint32_t* flag) {
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
        for (int w = 0; w < MAX_INPUTS; ++w) bad = bad || input_id(a, w, k) >= a.var0;
        if (bad) atomicOr(flag, FLAG_INPUT);
    }
    uint32_t id[4];
    RowSel q;
    row_ext(a, s, M, k, r, id, q);
#pragma unroll
    for (int w = 0; w < 4; ++w) ids[(uint64_t)w * total + g] = id[w];
    const Fr zero = Fr::zero();
    st_fr<Fr>(sel.p[Q_M], g, small<Fr>(q.m));
    st_fr<Fr>(sel.p[Q_L], g, q.pow2 >= 0 ? pow2_mont<Fr>((uint32_t)q.pow2) : small<Fr>(q.l));
    st_fr<Fr>(sel.p[Q_R], g, small<Fr>(q.r));
    st_fr<Fr>(sel.p[Q_O], g, small<Fr>(q.o));
    st_fr<Fr>(sel.p[Q_4], g, small<Fr>(q.q4));
    st_fr<Fr>(sel.p[Q_C], g, a.kind == ZK_GADGET_CONST_WITNESS ? coeff_of<Fr>(a, Q_C, k) : small<Fr>(q.c));
    st_fr<Fr>(sel.p[Q_ARITH], g, small<Fr>(q.arith));
    st_fr<Fr>(sel.p[Q_RANGE], g, zero);
    st_fr<Fr>(sel.p[Q_LOGIC], g, zero);
    st_fr<Fr>(sel.p[Q_FIXED], g, zero);
    st_fr<Fr>(sel.p[Q_VAR], g, small<Fr>(q.var_add));
    st_fr<Fr>(sel.p[Q_LOOKUP], g, small<Fr>(q.lookup));
}

// the t-th `add_variable_to_map` call of call k: Left, Right, Output, Fourth of row t / 4 (add_variables_to_map)
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_insertions_ext(zk_gadget_args a, Shape s, uint32_t* ins_var, uint32_t* ins_rec) {
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (g >= a.calls * s.ins) return;
    const uint64_t k = g / s.ins;
    const uint32_t t = (uint32_t)(g - k * s.ins);
    const uint32_t wire = t & 3u, r = t >> 2;
    uint32_t id[4];
    RowSel q;
    row_ext(a, s, M, k, r, id, q);
    ins_var[g] = pick4(id, wire);
    ins_rec[g] = (wire << REC_SHIFT) | (uint32_t)(a.row0 + k * s.rows + r);
}

// ---------------------------------------------------------------------------------------------------------------- witness kernels
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
    __shared__ Fr pre[GT];
    __shared__ Fr suf[GT];
    __shared__ Fr inv_total;
    const uint64_t k = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = k < a.calls, eq = a.kind == ZK_GADGET_IS_EQ;
    Fr x = Fr::zero();
    if (active) {
        x = ld_input<Fr>(values, a, 0, k, flag);
        if (eq) x = Fr::sub(x, ld_input<Fr>(values, a, 1, k, flag));
    }
    const bool is_zero = x.is_zero();                      // a zero enters the block's product as 1; its y is 1 by definition
    const Fr inv = block_inverse<Fr>(is_zero ? Fr::one() : x, pre, suf, &inv_total);
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
    Fr acc;                                                // e mod 2^(j+1)
    uint32_t bit = 0;
#pragma unroll
    for (uint32_t w = 0; w < 8; ++w) {
        const uint32_t lo = 32u * w;
        acc.v[w] = j + 1 >= lo + 32 ? e.v[w] : j + 1 <= lo ? 0u : e.v[w] & ((1u << (j + 1 - lo)) - 1u);
        if ((j >> 5) == w) bit = (e.v[w] >> (j & 31u)) & 1u;
    }
    st_value<Fr>(values, num_vars, v0 + j, bit ? Fr::one() : Fr::zero());
    if (j < M) st_value<Fr>(values, num_vars, v0 + 256 + j, Fr::to_mont(acc));
    if (j == 255) st_value<Fr>(values, num_vars, v0 + 256 + M, Fr::one());
}

// a point in extended coordinates: x = X / Z, y = Y / Z, T = X Y / Z
template <class Fr>
struct Ext {
    Fr X, Y, Z, T;
};
// The unified law in extended coordinates (Hisil, Wong, Carter, Dawson 2008, section 3.1): X3 / Z3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2)
// and Y3 / Z3 = (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2), the affine law of the reference, for any two pairs of coordinates; a zero
// denominator shows as Z3 = 0.
template <class Fr>
ZK_D Ext<Fr> ext_add(const Ext<Fr>& p, const Ext<Fr>& q, const Fr& ca, const Fr& cd) {
    const Fr A = Fr::mul(p.X, q.X), B = Fr::mul(p.Y, q.Y), C = Fr::mul(cd, Fr::mul(p.T, q.T)), D = Fr::mul(p.Z, q.Z);
    const Fr E = Fr::sub(Fr::sub(Fr::mul(Fr::add(p.X, p.Y), Fr::add(q.X, q.Y)), A), B);
    const Fr F = Fr::sub(D, C), G = Fr::add(D, C), H = Fr::sub(B, Fr::mul(ca, A));
    Ext<Fr> r;
    r.X = Fr::mul(E, F);
    r.Y = Fr::mul(G, H);
    r.T = Fr::mul(E, H);
    r.Z = Fr::mul(F, G);
    return r;
}
template <class Fr>
ZK_D void st_slot(void* work, uint64_t slot, const Ext<Fr>& p) {
    st_fr<Fr>(work, 3 * slot, p.X);
    st_fr<Fr>(work, 3 * slot + 1, p.Y);
    st_fr<Fr>(work, 3 * slot + 2, p.Z);
}
template <int SH>
ZK_D void shl8(uint32_t (&w)[8]) {
    constexpr int ws = SH / 32, bs = SH % 32;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        const uint32_t hi = i - ws >= 0 ? w[i - ws] : 0u;
        const uint32_t lo = i - ws - 1 >= 0 ? w[i - ws - 1] : 0u;
        w[i] = bs ? (hi << bs) | (lo >> (32 - bs)) : hi;
    }
}

// Phase one.  work: slot s * calls + k holds accumulator s of call k as (X, Y, Z): s = 0 the identity, 2 i + 1 after the doubling of
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
    shl8<256 - M>(E);                                      // bit M - 1 at the top of word 7: iteration i reads bit M - 1 - i there
    const Fr ca = fr_words<Fr>(a.coeff_a), cd = fr_words<Fr>(a.coeff_d);
    Ext<Fr> acc = {Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
    st_slot<Fr>(work, k, acc);
#pragma unroll 1
    for (uint32_t i = 0; i < M; ++i) {
        acc = ext_add<Fr>(acc, acc, ca, cd);
        st_slot<Fr>(work, (uint64_t)(2 * i + 1) * a.calls + k, acc);
        const bool bit = E[7] >> 31;
        shl8<1>(E);
        Ext<Fr> sel;                                       // (bit x, 1 - bit + bit y): the point, or the identity
        sel.X = bit ? px : Fr::zero();
        sel.Y = bit ? py : Fr::one();
        sel.Z = Fr::one();
        sel.T = bit ? pt : Fr::zero();
        acc = ext_add<Fr>(acc, sel, ca, cd);
        st_slot<Fr>(work, (uint64_t)(2 * i + 2) * a.calls + k, acc);
    }
}

// Phase two: lane g = i * calls + k makes the accumulators 2 i, 2 i + 1, 2 i + 2 of call k affine and writes the values of iteration i
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_w_var_norm(zk_gadget_args a, void* values, uint64_t num_vars, const void* work, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    constexpr uint32_t M = Cv::FrP::BITS;
    __shared__ Fr pre[GT];
    __shared__ Fr suf[GT];
    __shared__ Fr inv_total;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    const bool active = g < a.calls * M;
    const uint32_t i = active ? (uint32_t)(g / a.calls) : 0u;
    const uint64_t k = active ? g - (uint64_t)i * a.calls : 0u;
    Fr X[3], Y[3], Z[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        X[t] = Fr::zero();
        Y[t] = Z[t] = Fr::one();
        if (active) {
            const uint64_t slot = 3 * ((uint64_t)(2 * i + t) * a.calls + k);
            X[t] = ld_fr<Fr>(work, slot);
            Y[t] = ld_fr<Fr>(work, slot + 1);
            Z[t] = ld_fr<Fr>(work, slot + 2);
        }
        if (Z[t].is_zero()) {                              // no sum in affine coordinates: the flag, and values nobody reads
            atomicOr(flag, FLAG_DENOM);
            Z[t] = Fr::one();
        }
    }
    const Fr z01 = Fr::mul(Z[0], Z[1]);
    const Fr zi = block_inverse<Fr>(Fr::mul(z01, Z[2]), pre, suf, &inv_total);
    if (!active) return;
    const Fr i2 = Fr::mul(zi, z01), i1 = Fr::mul(zi, Fr::mul(Z[0], Z[2])), i0 = Fr::mul(zi, Fr::mul(Z[1], Z[2]));
    const Fr rx = Fr::mul(X[0], i0), ry = Fr::mul(Y[0], i0), dx = Fr::mul(X[1], i1), dy = Fr::mul(Y[1], i1);
    const Fr e = Fr::from_mont(ld_input<Fr>(values, a, 0, k, flag));
    const uint32_t j = M - 1 - i;
    uint32_t bit = 0;
#pragma unroll
    for (uint32_t w = 0; w < 8; ++w)
        if ((j >> 5) == w) bit = (e.v[w] >> (j & 31u)) & 1u;
    const Fr sx = bit ? ld_input<Fr>(values, a, 1, k, flag) : Fr::zero();
    const Fr sy = bit ? ld_input<Fr>(values, a, 2, k, flag) : Fr::one();
    const uint64_t u = a.var0 + k * (9 * M + 257) + 257 + M + 8 * (uint64_t)i;
    st_value<Fr>(values, num_vars, u, Fr::mul(rx, ry));
    st_value<Fr>(values, num_vars, u + 1, dx);
    st_value<Fr>(values, num_vars, u + 2, dy);
    st_value<Fr>(values, num_vars, u + 3, sx);
    st_value<Fr>(values, num_vars, u + 4, sy);
    st_value<Fr>(values, num_vars, u + 5, Fr::mul(dx, sy));
    st_value<Fr>(values, num_vars, u + 6, Fr::mul(X[2], i2));
    st_value<Fr>(values, num_vars, u + 7, Fr::mul(Y[2], i2));
}

// ---------------------------------------------------------------------------------------------------------------- lookup tables
template <class Cv>
__global__ void __launch_bounds__(GT) lookup_table_fill(uint32_t op, uint32_t lower, uint32_t n_bits, void* ca, void* cb, void* cc, void* cdd) {
    typedef typename Cv::Fr Fr;
    const uint32_t w = (1u << n_bits) - lower;
    const uint64_t r = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (r >= (uint64_t)w * w) return;
    const uint32_t x = lower + (uint32_t)(r / w), y = lower + (uint32_t)(r % w);        // below 2^12: a product stays below 2^24
    const uint32_t c = (op == 0 ? x + y : op == 1 ? x * y : op == 2 ? x ^ y : x & y) & ((1u << n_bits) - 1u);
    st_fr<Fr>(ca, r, Fr::from_u32(x));
    st_fr<Fr>(cb, r, Fr::from_u32(y));
    st_fr<Fr>(cc, r, Fr::from_u32(c));
    st_fr<Fr>(cdd, r, op == 0 ? Fr::zero() : op == 1 ? Fr::one() : op == 2 ? Fr::neg(Fr::one()) : Fr::from_u32(2));
}

// ---------------------------------------------------------------------------------------------------------------- host side
int check_args_ext(const zk_gadget_args& a, const Shape& s) {
    if (a.kind <= ZK_GADGET_FIXED_BASE || a.kind > LAST_KIND) return ZK_ERR_BAD_ARG;
    for (int w = 0; w < inputs_needed(a.kind); ++w)
        if (!(w < 4 ? a.inputs[w] : a.inputs_ext[w - 4])) return ZK_ERR_BAD_ARG;
    return check_extent(a, s);
}

template <class Cv>
int layout_ext_impl(zk_ctx* c, const zk_gadget_args& a, uint32_t* d_ids, void* const* d_sel, uint32_t* d_ins_var, uint32_t* d_ins_rec) {
    const Shape s = gadget_shape(a.kind, a.num_bits, a.flags, Cv::FrP::BITS);
    const int rc = check_args_ext(a, s);
    if (rc) return rc;
    SelPtrs sel;
    for (int j = 0; j < N_SEL; ++j) sel.p[j] = d_sel[j];
    return run_flagged<Cv>(c, 0, [&](uint32_t* d_flag, void*) -> int {
        ProfScope ps(c, "gadget_layout_ext");
        hipLaunchKernelGGL(gadget_layout_ext<Cv>, dim3(blocks_of(a.calls * s.rows, GT)), dim3(GT), 0, c->stream, a, s, d_ids, sel, d_flag);
        hipLaunchKernelGGL(gadget_insertions_ext<Cv>, dim3(blocks_of(a.calls * s.ins, GT)), dim3(GT), 0, c->stream, a, s, d_ins_var, d_ins_rec);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

template <class Cv>
int witness_ext_impl(zk_ctx* c, const zk_gadget_args& a, void* d_values, uint64_t num_vars) {
    constexpr uint32_t M = Cv::FrP::BITS;
    const Shape s = gadget_shape(a.kind, a.num_bits, a.flags, M);
    const int rc = check_args_ext(a, s);
    if (rc) return rc;
    if (a.var0 + a.calls * s.vars > num_vars) return ZK_ERR_BAD_ARG;
    if (s.vars == 0) return ZK_OK;
    return run_flagged<Cv>(c, gadget_work_bytes(a.kind, M, a.calls), [&](uint32_t* d_flag, void* work) -> int {
        hipStream_t st = c->stream;
        switch (a.kind) {
        case ZK_GADGET_IS_ZERO:
        case ZK_GADGET_IS_EQ: {
            ProfScope ps(c, "gadget_w_is_zero");
            hipLaunchKernelGGL(gadget_w_is_zero<Cv>, dim3(blocks_of(a.calls, GT)), dim3(GT), 0, st, a, d_values, num_vars, d_flag);
            break;
        }
        case ZK_GADGET_VAR_BASE: {
            {
                ProfScope ps(c, "gadget_w_var_bits");
                hipLaunchKernelGGL(gadget_w_var_bits<Cv>, dim3(blocks_of(a.calls * 256, GT)), dim3(GT), 0, st, a, d_values, num_vars, d_flag);
            }
            {
                ProfScope ps(c, "gadget_w_var_walk");
                hipLaunchKernelGGL(gadget_w_var_walk<Cv>, dim3(blocks_of(a.calls, GT)), dim3(GT), 0, st, a, (const void*)d_values, work, d_flag);
            }
            ProfScope ps(c, "gadget_w_var_norm");
            hipLaunchKernelGGL(gadget_w_var_norm<Cv>, dim3(blocks_of(a.calls * M, GT)), dim3(GT), 0, st, a, d_values, num_vars, (const void*)work,
                               d_flag);
            break;
        }
        default: {
            ProfScope ps(c, "gadget_w_select");
            hipLaunchKernelGGL(gadget_w_select<Cv>, dim3(blocks_of(a.calls, GT)), dim3(GT), 0, st, a, s.vars, d_values, num_vars, d_flag);
            break;
        }
        }
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

}  // namespace

int gadget_ext_layout(zk_ctx* c, int curve_id, const zk_gadget_args& a, uint32_t* d_ids, void* const* d_sel, uint32_t* d_ins_var, uint32_t* d_ins_rec) {
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return layout_ext_impl<decltype(cv)>(c, a, d_ids, d_sel, d_ins_var, d_ins_rec); });
}

int gadget_ext_witness(zk_ctx* c, int curve_id, const zk_gadget_args& a, void* d_values, uint64_t num_vars) {
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return witness_ext_impl<decltype(cv)>(c, a, d_values, num_vars); });
}

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_lookup_table_dev(zk_ctx* c, int curve_id, int op, uint32_t lower_bound, uint32_t n_bits, void* d_a, void* d_b, void* d_c, void* d_d) {
    if (!c || !zk_curve_ok(curve_id) || !d_a || !d_b || !d_c || !d_d) return ZK_ERR_BAD_ARG;
    if (op < 0 || op > 3 || n_bits > 12 || lower_bound >= (1u << n_bits)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    const uint64_t w = (1u << n_bits) - lower_bound;
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) -> int {
        ProfScope ps(c, "lookup_table_fill");
        hipLaunchKernelGGL(lookup_table_fill<decltype(cv)>, dim3(blocks_of(w * w, GT)), dim3(GT), 0, c->stream, (uint32_t)op, lower_bound, n_bits,
                           d_a, d_b, d_c, d_d);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}
