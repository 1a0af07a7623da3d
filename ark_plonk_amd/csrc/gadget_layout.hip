// The circuit builder on the device, the part that runs once per circuit: what `StandardComposer` (plonk-core/src/constraint_system/)
// holds after a gadget was called B times in a row -- rows, variable ids, selector values, the `add_variable_to_map` calls in call
// order -- for the arithmetic family (arithmetic.rs:103-168, composer.rs:269-350, boolean.rs:25-51), range_gate (range.rs:27-195),
// xor_gate / and_gate (logic.rs:36-345), point_addition_gate (ecc/curve_addition/variable_base_gate.rs:24-93), fixed_base_scalar_mul
// (ecc/scalar_mul/fixed_base.rs:51-160), add_witness_to_circuit_description (composer.rs:192-196), is_zero_with_output /
// is_eq_with_output (composer.rs:355-392), conditional_select (composer.rs:404-433), conditional_point_select /
// conditional_point_neg (ecc/mod.rs:145-182), variable_base_scalar_mul (ecc/scalar_mul/variable_base.rs:27-95) and lookup_gate
// (lookup.rs:18-65), with a given or a computed output, add_dummy_constraints (composer.rs:493-548) -- and the blocks of a lookup table (lookup/lookup_table.rs:94-152).  Segments, shapes and errors: gadget_common.cuh.
//
//   row_of             ONE description of row r of call k for every kind: the four variable ids and the selectors
//   gadget_layout      one lane per (call, row): stores the ids and the twelve selector values of the row; input ids checked
//   gadget_insertions  one lane per (call, insertion): (variable, wire << 30 | row) -- independent of the padded size
//   lookup_table_fill  one lane per row of an insert_multi_* block
// Every kernel guards its own addresses: a refused call leaves unspecified values, never an access outside the buffers.  Working
// memory: the 256 bytes of the flag word, one allocation per call, freed on every path.
#include "gadget_common.cuh"

namespace {

struct SelPtrs {
    void* p[N_SEL];
};

// The selectors of a row.  Small integers: q_m, q_l, q_r, q_4, q_c in {-1, 0, 1}, q_o = -1 on every arithmetic row with an output
// (the dummy rows alone hold 2, 3, 4 and 127), logic = +-1: q_c = q_logic (logic.rs:237-260), pow2 >= 0: q_l = 2^pow2.  Field values are named here and read where they are stored.
enum RowSrc {
    SRC_NONE,
    SRC_COEFFS,                                            // q_m, q_l, q_r, q_o, q_4, q_c: the six coefficients of the segment (coeff_of)
    SRC_COEFF_C,                                           // q_c alone is the segment's coefficient
    SRC_TABLE                                              // q_l, q_r, q_c: row `table_row` of the segment's table
};
struct RowSel {
    int m = 0, l = 0, r = 0, o = 0, q4 = 0, c = 0, logic = 0, pow2 = -1;
    bool arith = false, range = false, fixed = false, var_add = false, lookup = false;
    RowSrc src = SRC_NONE;
    uint32_t table_row = 0;
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
ZK_D void row_of(const zk_gadget_args& a, const Shape& s, uint32_t M, uint64_t k, uint32_t r, uint32_t (&id)[4], RowSel& q) {
    const uint32_t v0 = (uint32_t)(a.var0 + k * s.vars);
    id[0] = id[1] = id[2] = id[3] = 0;
    switch (a.kind) {
    case ZK_GADGET_POLY:
        id[0] = input_id(a, 0, k);
        id[1] = input_id(a, 1, k);
        id[2] = (a.flags & ZK_GADGET_COMPUTE_OUT) ? v0 : input_id(a, 2, k);
        id[3] = input_id(a, 3, k);
        q.arith = true;
        q.src = SRC_COEFFS;
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
            q.range = r < g;
        } else {                                           // assert_equal(last accumulator, witness)
            id[0] = v0 + s.vars - 1;
            id[1] = input_id(a, 0, k);
            q.arith = true;
            q.l = 1, q.r = -1;
        }
        break;
    }
    case ZK_GADGET_LOGIC: {
        // row r holds the prefixes after quad r - 1 and the product of quad r (logic.rs:73-235)
        const uint32_t n = a.num_bits / 2;
        if (r > 0) {
            id[0] = v0 + 4 * (r - 1);
            id[1] = v0 + 4 * (r - 1) + 1;
            id[3] = v0 + 4 * (r - 1) + 3;
        }
        if (r < n) {
            id[2] = v0 + 4 * r + 2;
            q.c = q.logic = (a.flags & ZK_GADGET_XOR) ? -1 : 1;
        }
        break;
    }
    case ZK_GADGET_CURVE_ADD:
        if (r == 0) {
#pragma unroll
            for (int w = 0; w < 4; ++w) id[w] = input_id(a, w, k);
            q.var_add = true;
        } else {
            id[0] = v0 + 1;
            id[1] = v0 + 2;
            id[3] = v0;
        }
        break;
    case ZK_GADGET_FIXED_BASE:
        if (r < 3) {                                       // constrain_to_constant: acc_x = 0, acc_y = 1, scalar accumulator = 0
            id[0] = id[1] = id[2] = v0 + r;
            q.arith = true;
            q.l = 1, q.c = r == 1 ? -1 : 0;
        } else if (r < 3 + M) {                            // the digit of weight 2^(M-1-i) against row i of the table
            const uint32_t i = r - 3;
            id[0] = v0 + 4 * i;
            id[1] = v0 + 4 * i + 1;
            id[2] = v0 + 4 * i + 3;
            id[3] = v0 + 4 * i + 2;
            q.fixed = true;
            q.src = SRC_TABLE;
            q.table_row = i;
        } else if (r == 3 + M) {
            id[0] = v0 + 4 * M;
            id[1] = v0 + 4 * M + 1;
            id[3] = v0 + 4 * M + 2;
            q.arith = true;
        } else {                                           // assert_equal(scalar accumulator, scalar)
            id[0] = v0 + 4 * M + 2;
            id[1] = input_id(a, 0, k);
            q.arith = true;
            q.l = 1, q.r = -1;
        }
        break;
    case ZK_GADGET_CONST_WITNESS:
        id[0] = id[1] = id[2] = v0;
        q.arith = true;
        q.l = 1;
        q.src = SRC_COEFF_C;
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
    case ZK_GADGET_LOOKUP_OUT:                             // a, b, d: inputs 4, 5, 6; the output is the new variable
        id[0] = input_id(a, 4, k), id[1] = input_id(a, 5, k), id[2] = v0, id[3] = input_id(a, 6, k);
        q.lookup = true;
        break;
    case ZK_GADGET_DUMMY:                                  // new variables v0 .. v0 + 3: six, one, seven, minus twenty
        q.arith = q.lookup = true;
        q.m = 1;
        if (r == 0) {
            id[0] = v0, id[1] = v0 + 2, id[2] = v0 + 3, id[3] = v0 + 1;
            q.l = 2, q.r = 3, q.o = 4, q.c = 4, q.q4 = 1;
        } else {
            id[0] = v0 + 3, id[1] = v0, id[2] = v0 + 2;
            q.l = 1, q.r = 1, q.o = 1, q.c = 127;
        }
        break;
    default: break;
    }
}

ZK_D uint32_t pick4(const uint32_t (&id)[4], uint32_t w) { return w == 0 ? id[0] : w == 1 ? id[1] : w == 2 ? id[2] : id[3]; }
template <class Fr>
ZK_D Fr small(int v) {
    if (v == 0) return Fr::zero();
    const Fr m = v == 1 || v == -1 ? Fr::one() : Fr::from_u32((uint32_t)(v < 0 ? -v : v));
    return v > 0 ? m : Fr::neg(m);
}
// 2^j (j < 256, below the modulus) in Montgomery form; the word is chosen by comparison, not by a run-time index
template <class Fr>
ZK_D Fr pow2_mont(uint32_t j) {
    Fr c;
#pragma unroll
    for (uint32_t w = 0; w < 8; ++w) c.v[w] = (j >> 5) == w ? 1u << (j & 31u) : 0u;
    return Fr::to_mont(c);
}
// selector column j of a row: the named field value where the row has one, the small integer otherwise
template <class Fr>
ZK_D Fr selector_of(const zk_gadget_args& a, const RowSel& q, int j, int v, uint64_t k) {
    if (q.src == SRC_COEFFS || (q.src == SRC_COEFF_C && j == Q_C)) return coeff_of<Fr>(a, j, k);
    if (q.src == SRC_TABLE && (j == Q_L || j == Q_R || j == Q_C))
        return ld_fr<Fr>(a.table, 3 * (uint64_t)q.table_row + (j == Q_L ? 0 : j == Q_R ? 1 : 2));
    if (j == Q_L && q.pow2 >= 0) return pow2_mont<Fr>((uint32_t)q.pow2);
    return small<Fr>(v);
}

// ---------------------------------------------------------------------------------------------------------------- kernels
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
        for (int w = 0; w < MAX_INPUTS; ++w) bad = bad || input_id(a, w, k) >= a.var0;
        if (bad) atomicOr(flag, FLAG_INPUT);
    }
    uint32_t id[4];
    RowSel q;
    row_of(a, s, M, k, r, id, q);
#pragma unroll
    for (int w = 0; w < 4; ++w) ids[(uint64_t)w * total + g] = id[w];
    const int v[N_SEL] = {q.m, q.l, q.r, q.o, q.q4, q.c, q.arith, q.range, q.logic, q.fixed, q.var_add, q.lookup};      // in the order of Q_M ..
#pragma unroll
    for (int j = 0; j < N_SEL; ++j) st_fr<Fr>(sel.p[j], g, j < 6 ? selector_of<Fr>(a, q, j, v[j], k) : small<Fr>(v[j]));
}

// the t-th `add_variable_to_map` call of call k: Left, Right, Output, Fourth of row t / 4 (add_variables_to_map), but for the two
// gadgets whose call order is not the row order
template <class Cv>
__global__ void __launch_bounds__(GT) gadget_insertions(zk_gadget_args a, Shape s, uint32_t* ins_var, uint32_t* ins_rec) {
    constexpr uint32_t M = Cv::FrP::BITS;
    const uint64_t g = (uint64_t)blockIdx.x * GT + threadIdx.x;
    if (g >= a.calls * s.ins) return;
    const uint64_t k = g / s.ins;
    const uint32_t t = (uint32_t)(g - k * s.ins);
    const uint32_t v0 = (uint32_t)(a.var0 + k * s.vars);
    uint32_t var = 0, wire = t & 3u, r = t >> 2;
    bool from_row = true;
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
        const uint32_t n = a.num_bits / 2;
        if (t < 3) {                                       // the zero variable on Left, Right, Fourth of the first row
            wire = t == 2 ? 3u : t;
            r = 0;
        } else if (t < 3 + 4 * n) {                        // Left(n), Right(n), Fourth(n), then Output(n - 1)
            const uint32_t i = (t - 3) >> 2, j = (t - 3) & 3u;
            wire = j == 2 ? 3u : j == 3 ? 2u : j;
            var = v0 + 4 * i + (j == 2 ? 3u : j == 3 ? 2u : j);
            r = j == 3 ? i : i + 1;
        } else {
            wire = 2;
            r = n;
        }
    }
    if (from_row) {
        uint32_t id[4];
        RowSel q;
        row_of(a, s, M, k, r, id, q);
        var = pick4(id, wire);
    }
    ins_var[g] = var;
    ins_rec[g] = (wire << REC_SHIFT) | (uint32_t)(a.row0 + k * s.rows + r);
}

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
template <class Cv>
int layout_impl(zk_ctx* c, const zk_gadget_args& a, uint32_t* d_ids, void* const* d_sel, uint32_t* d_ins_var, uint32_t* d_ins_rec) {
    const Shape s = gadget_shape(a.kind, a.num_bits, a.flags, Cv::FrP::BITS);
    const int rc = check_args(a, s);
    if (rc) return rc;
    SelPtrs sel;
    for (int j = 0; j < N_SEL; ++j) sel.p[j] = d_sel[j];
    return run_flagged(c, 0, [&](uint32_t* d_flag, void*) -> int {
        ProfScope ps(c, "gadget_layout");
        hipLaunchKernelGGL(gadget_layout<Cv>, dim3(blocks_of(a.calls * s.rows, GT)), dim3(GT), 0, c->stream, a, s, d_ids, sel, d_flag);
        hipLaunchKernelGGL(gadget_insertions<Cv>, dim3(blocks_of(a.calls * s.ins, GT)), dim3(GT), 0, c->stream, a, s, d_ins_var, d_ins_rec);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_gadget_shape(int kind, int curve_id, uint32_t num_bits, uint32_t flags, size_t calls, uint32_t* rows, uint32_t* vars, uint32_t* insertions,
                    size_t* work_bytes) {
    if (kind < 0 || kind > (int)LAST_KIND || !zk_curve_ok(curve_id) || !bits_ok((uint32_t)kind, num_bits)) return ZK_ERR_BAD_ARG;
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
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return layout_impl<decltype(cv)>(c, a, (uint32_t*)d_wire_ids, d_selectors, (uint32_t*)d_ins_var, (uint32_t*)d_ins_rec);
    });
}

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
