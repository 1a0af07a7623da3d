// What the two units of the device composer share -- gadget_layout.hip, the circuit description built once per circuit, and
// gadget_witness.hip, the values replayed once per proof -- each helper defined once: the shape table of every gadget kind, what both
// entry points refuse before anything is launched, the access to a segment's inputs and coefficients and the guarded value store
// (the flagged launch -- one working-memory allocation per call, one flag word read back once -- is api_internal.h's).  A SEGMENT is
// B calls of one gadget with the same parameters; every gadget has a fixed shape per call (R rows, V new variables, I insertions:
// gadget_shape), so call k owns rows row0 + k R ..., variables var0 + k V ... and insertions k I ... and no kernel loops over calls or
// rows on the host.  Errors are one flag word, OR-ed, read back once per call.  No buffer of the ctx is used, so both calls run
// inside an open deferred round.  Not part of the C ABI.
#pragma once
#include "api_internal.h"
#include "fr_io.cuh"

namespace {

constexpr uint32_t GT = 256;                       // lanes per workgroup, every kernel
constexpr uint32_t FLAG_INPUT = 1, FLAG_SCALAR = 2, FLAG_DENOM = 4;
constexpr uint32_t REC_SHIFT = 30;                 // insertion record: wire << 30 | row (rows are below 2^28)
constexpr uint64_t MAX_ROWS = (uint64_t)1 << 28, MAX_VARS = (uint64_t)1 << 31;
// selector columns in the order of prover.SELECTORS
constexpr int Q_M = 0, Q_L = 1, Q_R = 2, Q_O = 3, Q_4 = 4, Q_C = 5, Q_ARITH = 6, Q_RANGE = 7, Q_LOGIC = 8, Q_FIXED = 9, Q_VAR = 10, Q_LOOKUP = 11;
constexpr int N_SEL = 12;
constexpr uint32_t LAST_KIND = ZK_GADGET_DUMMY;

struct Shape {
    uint32_t rows, vars, ins;
};
ZK_HD Shape gadget_shape(uint32_t kind, uint32_t num_bits, uint32_t flags, uint32_t m_bits) {
    Shape s = {0, 0, 0};
    const uint32_t g = (num_bits + 7) / 8;
    switch (kind) {
    case ZK_GADGET_POLY: s = {1, (flags & ZK_GADGET_COMPUTE_OUT) ? 1u : 0u, 4}; break;
    case ZK_GADGET_RANGE: s = {g + 2, num_bits / 2, 4 * g + 5}; break;
    case ZK_GADGET_LOGIC: s = {num_bits / 2 + 1, 2 * num_bits, 2 * num_bits + 4}; break;
    case ZK_GADGET_CURVE_ADD: s = {2, 3, 8}; break;
    case ZK_GADGET_FIXED_BASE: s = {m_bits + 5, 4 * m_bits + 3, 4 * (m_bits + 5)}; break;
    case ZK_GADGET_CONST_WITNESS: s = {1, 1, 4}; break;
    case ZK_GADGET_IS_ZERO: s = {2, 2, 8}; break;
    case ZK_GADGET_IS_EQ: s = {3, 3, 12}; break;
    case ZK_GADGET_SELECT: s = {4, 4, 16}; break;
    case ZK_GADGET_POINT_SELECT: s = {8, 8, 32}; break;
    case ZK_GADGET_POINT_NEG: s = {5, 5, 20}; break;
    case ZK_GADGET_VAR_BASE: s = {8 * m_bits + 2, 9 * m_bits + 257, 32 * m_bits + 8}; break;
    case ZK_GADGET_LOOKUP: s = {1, 0, 4}; break;
    case ZK_GADGET_LOOKUP_OUT: s = {1, 1, 4}; break;
    case ZK_GADGET_DUMMY: s = {2, 4, 8}; break;
    default: break;
    }
    return s;
}
// the device bytes a witness of `calls` calls allocates beyond the 256 of the flag word: the projective accumulators between the two
// phases of a scalar multiplication, (X, Y, Z) of 32 bytes each
inline size_t gadget_work_bytes(uint32_t kind, uint32_t m_bits, uint64_t calls) {
    if (kind == ZK_GADGET_FIXED_BASE) return (size_t)96 * (m_bits + 1) * calls;
    if (kind == ZK_GADGET_VAR_BASE) return (size_t)96 * (2 * m_bits + 1) * calls;
    return 0;
}

// the handles of input w: inputs[0 .. 4), then inputs_ext; null where the segment has no such input
constexpr int MAX_INPUTS = 7;
ZK_HD const uint32_t* input_ptr(const zk_gadget_args& a, int w) { return (const uint32_t*)(w < 4 ? a.inputs[w] : a.inputs_ext[w - 4]); }
// input w of call k; an input the segment does not have reads as the zero variable
ZK_D uint32_t input_id(const zk_gadget_args& a, int w, uint64_t k) {
    const uint32_t* p = input_ptr(a, w);
    return p ? p[k] : 0u;
}
template <class Fr>
ZK_D Fr fr_words(const uint64_t* w) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.v[2 * i] = (uint32_t)w[i];
        r.v[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return r;
}
template <class Fr>
ZK_D Fr coeff_of(const zk_gadget_args& a, int j, uint64_t k) {
    return a.coeff[j] ? ld_fr<Fr>(a.coeff[j], k) : fr_words<Fr>(a.coeff_const + 4 * j);
}

// ---------------------------------------------------------------------------------------------------------------- witness helpers
template <class Fr>
ZK_D Fr ld_input(const void* values, const zk_gadget_args& a, int w, uint64_t k, uint32_t* flag) {
    const uint32_t* p = input_ptr(a, w);
    if (!p) return Fr::zero();
    const uint32_t id = p[k];
    if (id >= a.var0) {
        atomicOr(flag, FLAG_INPUT);
        return Fr::zero();
    }
    return ld_fr<Fr>(values, id);
}
template <class Fr>
ZK_D void st_value(void* values, uint64_t num_vars, uint64_t id, const Fr& v) {
    if (id < num_vars) st_fr<Fr>(values, id, v);
}
// ---------------------------------------------------------------------------------------------------------------- host side
inline int inputs_needed(uint32_t kind) {
    switch (kind) {
    case ZK_GADGET_POLY: return 2;                         // and the output, unless it is computed
    case ZK_GADGET_RANGE: return 1;
    case ZK_GADGET_LOGIC: return 2;
    case ZK_GADGET_CURVE_ADD: return 4;
    case ZK_GADGET_FIXED_BASE: return 1;                   // and the table
    case ZK_GADGET_IS_ZERO: return 1;
    case ZK_GADGET_IS_EQ: return 2;
    case ZK_GADGET_SELECT: return 3;
    case ZK_GADGET_POINT_SELECT: return 5;
    case ZK_GADGET_POINT_NEG: return 2;
    case ZK_GADGET_VAR_BASE: return 3;
    case ZK_GADGET_LOOKUP: return 3;
    default: return 0;                                     // LOOKUP_OUT: a, b, d in inputs_ext, each may be the zero variable
    }
}
// num_bits of the kinds that take one: even, 2 .. 256
inline bool bits_ok(uint32_t kind, uint32_t num_bits) {
    return (kind != ZK_GADGET_RANGE && kind != ZK_GADGET_LOGIC) || (num_bits >= 2 && num_bits <= 256 && !(num_bits & 1u));
}
// what both entry points refuse before anything is launched; a number between the kinds that names none has a shape of no rows
inline int check_args(const zk_gadget_args& a, const Shape& s) {
    if (a.kind > LAST_KIND || a.calls == 0 || s.rows == 0 || !bits_ok(a.kind, a.num_bits)) return ZK_ERR_BAD_ARG;
    for (int w = 0; w < inputs_needed(a.kind); ++w)
        if (!input_ptr(a, w)) return ZK_ERR_BAD_ARG;
    switch (a.kind) {
    case ZK_GADGET_POLY:
        if (!(a.flags & ZK_GADGET_COMPUTE_OUT) && !a.inputs[2]) return ZK_ERR_BAD_ARG;
        break;
    case ZK_GADGET_FIXED_BASE:
        if (!a.table) return ZK_ERR_BAD_ARG;
        break;
    default: break;
    }
    if (a.calls > MAX_ROWS || a.row0 > MAX_ROWS || a.row0 + a.calls * s.rows > MAX_ROWS) return ZK_ERR_UNSUPPORTED;
    if (a.var0 == 0 || a.var0 > MAX_VARS || a.var0 + a.calls * s.vars > MAX_VARS) return ZK_ERR_UNSUPPORTED;
    return ZK_OK;
}

}  // namespace
