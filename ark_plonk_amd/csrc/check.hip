// Which rows of a circuit does a witness violate?  zk_circuit_check_dev: for every row of the padded circuit a 32-bit mask of the
// constraints the row breaks, and a summary (rows that fail, the first of them, rows per bit) -- before any proof is computed.
//
// The reference's counterpart is `StandardComposer::check_circuit_satisfied` (plonk-core/src/constraint_system/composer.rs:661-814,
// feature `trace`): serial, stops at the first failing gate, arithmetic / logic / range only, no copy constraints, no lookups.  Here
// every row is tested at once against the summands of the identities the quotient enforces (quotient.hip; widget/arithmetic.rs:
// 51-63, range.rs:47-63, logic.rs:65-133, ecc/fixed_base_scalar_mul.rs:88-156, ecc/curve_addition.rs:62-97), taken one by one, with no
// random challenge: a bit is set iff the selector of its widget and its term are both non-zero (DESIGN.md section 6d has the table).
//   check_gates     bits 0-16: one lane per row, "next row" = (i + 1) mod n; plain store of the row's word
//   check_id_keys   the 4n identity encodings K_w * omega^row of the permutation argument (domain.cuh)
//   map_build       an open-addressing map (linear probing, capacity = the power of two >= 2 x keys) over keys of 1 or 4 field
//                   elements; a slot holds the INDEX of its key and an occupant's key is always compared in full
//   check_copy      bits 18-21: sigma_k[i] -> position through the identity map (no encoding: the flag word), the two cells compared
//   check_lookup    bit 17: rows with q_lookup != 0 whose (a, b, c, d) is no row of the table
//   check_summary   per-wave ballots -> per-block counters in LDS -> one integer atomic per block and counter; check_finish: the first
//                   row's mask
// Nothing depends on the arrival order of an atomic: which of two equal keys owns a slot is never read (only presence; the identity
// encodings are pairwise distinct), masks are OR-ed, the summary is sums and a minimum of integers.
//
// Field arithmetic of check_gates: the 29-bit-limb type of the quotient kernel (fieldu.cuh), lazily reduced, with the bound carried in
// the type (Z<F, B>, to_rp: zbound.cuh, the one definition this unit and quotient.hip include).  Zero has several encodings there
// (0, r, 2r, ...): every zero test is made on a value below 2r (a Montgomery product), which is 0 or r exactly.
//
// Working memory: one allocation per call, freed before return, no buffer of the ctx (the call runs inside an open deferred round):
// 128 n (identity keys) + 32 n (their map) + 4 * capacity(table_rows) (<= 8 n) + 4 n when the caller takes no mask + 8 KiB.
#include "api_internal.h"
#include "domain.cuh"
#include "zbound.cuh"

namespace {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t FLAG_SIGMA = 1;                // a sigma entry that is no K_w * omega^row
constexpr uint32_t CT = 256;                      // lanes per workgroup, every kernel
constexpr size_t HEAD = 1024;                      // flag word at 0, summary at 256: cleared and read back as one block
constexpr uint32_t CTAB = 48;                     // multiples of r held for the load conversion

constexpr uint32_t BIT_ARITH = 0, BIT_RANGE = 1, BIT_LOGIC = 5, BIT_FIXED = 10, BIT_CURVE = 14, BIT_LOOKUP = 17, BIT_COPY = 18;

// ---------------------------------------------------------------------------------------------------------------- key map
// A key is W field elements (Key<W>, KeyCols, ld_key, key_eq, key_hash: fr_io.cuh): element k of key i is col[k][i] (W = 4: a table
// row; W = 1: an identity encoding).
// Index of a key of the map equal to `q`, or EMPTY.  Every occupant on the way is compared in full.
template <int W>
ZK_D uint32_t map_find(const uint32_t* slots, uint32_t cap_mask, const KeyCols& cols, const Key<W>& q) {
    uint32_t s = key_hash<W>(q) & cap_mask;
    for (uint32_t step = 0; step <= cap_mask; ++step) {      // the map is at most half full: an empty slot ends the walk long before
        const uint32_t idx = slots[s];
        if (idx == EMPTY) return EMPTY;
        if (key_eq<W>(ld_key<W>(cols, idx), q)) return idx;
        s = (s + 1) & cap_mask;
    }
    return EMPTY;
}
// slots: all EMPTY before the launch.  A key equal to an occupant's is present already and claims nothing.
template <int W>
__global__ void __launch_bounds__(CT) map_build(uint32_t* slots, uint32_t cap_mask, KeyCols cols, uint64_t n_keys) {
    const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= n_keys) return;
    const Key<W> k = ld_key<W>(cols, i);
    uint32_t s = key_hash<W>(k) & cap_mask;
    for (uint32_t step = 0; step <= cap_mask; ++step) {
        const uint32_t old = atomicCAS(&slots[s], EMPTY, (uint32_t)i);
        if (old == EMPTY) return;
        if (key_eq<W>(ld_key<W>(cols, old), k)) return;      // the key columns are read-only: an index, once seen, names its key
        s = (s + 1) & cap_mask;
    }
}

// ---------------------------------------------------------------------------------------------------------------- identity keys
// consts: fill_id_consts (domain.cuh).  keys[w * n + row] = K_w * omega^row, canonical like every sigma entry.
template <class Cv>
__global__ void __launch_bounds__(CT) check_id_keys(uint32_t log_n, const void* consts, void* keys) {
    typedef typename Cv::Fr Fr;
    const uint64_t row = (uint64_t)blockIdx.x * CT + threadIdx.x;
    const uint64_t n = (uint64_t)1 << log_n;
    if (row >= n) return;
    const Fr pw = id_omega_pow<Fr>(consts, (uint32_t)row, log_n);
    st_fr<Fr>(keys, row, pw);
#pragma unroll 1
    for (uint32_t w = 1; w < 4; ++w) st_fr<Fr>(keys, w * n + row, Fr::mul(pw, ld_fr<Fr>(consts, w)));
}

// ---------------------------------------------------------------------------------------------------------------- copy and lookup
struct Cols4 {
    const void* p[4];
};
// one lane per cell (wire k, row i)
__global__ void __launch_bounds__(CT) check_copy(uint32_t log_n, Cols4 wires, Cols4 sigma, const uint32_t* slots, uint32_t cap_mask,
                                                 const void* id_keys, uint32_t* mask, uint32_t* flag) {
    const uint64_t p = (uint64_t)blockIdx.x * CT + threadIdx.x;
    const uint64_t n = (uint64_t)1 << log_n;
    if (p >= 4 * n) return;
    const uint32_t k = (uint32_t)(p >> log_n);
    const uint64_t i = p & (n - 1);
    const void* sg = k == 0 ? sigma.p[0] : k == 1 ? sigma.p[1] : k == 2 ? sigma.p[2] : sigma.p[3];
    const void* wk = k == 0 ? wires.p[0] : k == 1 ? wires.p[1] : k == 2 ? wires.p[2] : wires.p[3];
    Key<1> q;
    q.e[0] = ld_el(sg, i);
    const KeyCols cols = {{id_keys, nullptr, nullptr, nullptr}};
    const uint32_t pos = map_find<1>(slots, cap_mask, cols, q);
    if (pos == EMPTY || pos >= 4 * n) {
        atomicOr(flag, FLAG_SIGMA);
        return;
    }
    const uint32_t k2 = pos >> log_n;
    const void* w2 = k2 == 0 ? wires.p[0] : k2 == 1 ? wires.p[1] : k2 == 2 ? wires.p[2] : wires.p[3];
    if (!el_eq(ld_el(wk, i), ld_el(w2, pos & (uint32_t)(n - 1)))) atomicOr(&mask[i], 1u << (BIT_COPY + k));
}
__global__ void __launch_bounds__(CT) check_lookup(uint64_t n, Cols4 wires, const void* q_lookup, const uint32_t* slots, uint32_t cap_mask,
                                                   KeyCols table, uint64_t table_rows, uint32_t* mask) {
    const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= n) return;
    if (el_zero(ld_el(q_lookup, i))) return;
    bool found = false;
    if (table_rows) {
        const KeyCols w = {{wires.p[0], wires.p[1], wires.p[2], wires.p[3]}};
        found = map_find<4>(slots, cap_mask, table, ld_key<4>(w, i)) != EMPTY;
    }
    if (!found) atomicOr(&mask[i], 1u << BIT_LOOKUP);
}

// ---------------------------------------------------------------------------------------------------------------- summary
// s: failing_rows and bit_count zero, first_row all ones before the launch
__global__ void __launch_bounds__(CT) check_summary(const uint32_t* mask, uint64_t n, zk_circuit_check_summary* s) {
    __shared__ uint32_t cnt[32], rows, first;
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (t < 32) cnt[t] = 0;
    if (t == 32) rows = 0, first = CT;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * CT + t;
    const uint32_t m = i < n ? mask[i] : 0u;
    const uint64_t bad = __ballot(m != 0);
    if (bad) {                                               // wave-uniform
        if (lane == 0) {
            atomicAdd(&rows, (uint32_t)__popcll(bad));
            atomicMin(&first, t + (uint32_t)__ffsll((long long)bad) - 1);
        }
        for (uint32_t b = 0; b < 32; ++b) {
            const uint64_t bb = __ballot((m >> b) & 1u);
            if (bb && lane == 0) atomicAdd(&cnt[b], (uint32_t)__popcll(bb));
        }
    }
    __syncthreads();
    if (t < 32 && cnt[t]) atomicAdd((unsigned long long*)&s->bit_count[t], (unsigned long long)cnt[t]);
    if (t == 32 && rows) {
        atomicAdd((unsigned long long*)&s->failing_rows, (unsigned long long)rows);
        atomicMin((unsigned long long*)&s->first_row, (unsigned long long)blockIdx.x * CT + first);
    }
}
__global__ void check_finish(const uint32_t* mask, uint64_t n, zk_circuit_check_summary* s) {
    if (threadIdx.x | blockIdx.x) return;
    const uint64_t r = s->first_row;
    s->first_row = r < n ? r : n;
    s->first_mask = r < n ? mask[r] : 0u;
    s->reserved = 0;
}

// ---------------------------------------------------------------------------------------------------------------- gate terms
// the quotient kernel's bounded lazy arithmetic and load conversion (zbound.cuh): Z<F, B>, nonzero, to_rp, delta4
template <class F>
struct CArgsU {
    const void *w_l, *w_r, *w_o, *w_4, *pi;
    const void *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *q_arith, *q_range, *q_logic, *q_fixed, *q_var;
    // constants: canonical (< r) residues in the R' = 2^261 Montgomery form
    F coeff_a, coeff_d, one, c2, c3, c4, c9, c18, c81, c83;
    uint32_t rtab[CTAB][F::NL];                 // q * r, q < CTAB
    uint32_t ratio_fx;                          // floor(2^BITS / r * 2^10) - 1
    uint32_t top_shift;                         // BITS - 29 * (NL - 1)
};

// One lane per row; every column is read as two 16-byte words per lane, consecutive lanes consecutive rows.  A selector is tested on the
// words it was loaded as (canonical input: zero is all-zero words), and a widget whose selector is zero is skipped by the lane -- its
// bits are zero whatever its terms are -- so a row costs what its own gates cost.
template <class F>
__global__ void __launch_bounds__(CT) check_gates(const CArgsU<F>* __restrict__ Ap, uint64_t n, uint32_t* mask) {
    typedef Z<F, 10> C;      // a constant of the argument block (canonical)
    typedef Z<F, RP_B> L;      // a loaded column value
    __shared__ uint32_t rtab[CTAB][F::NL];
    const CArgsU<F>& A = *Ap;
    for (uint32_t k = threadIdx.x; k < CTAB * F::NL; k += CT) rtab[k / F::NL][k % F::NL] = A.rtab[k / F::NL][k % F::NL];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= n) return;
    const uint64_t nx = i + 1 == n ? 0 : i + 1;               // composer.rs:707-712
    const uint32_t ratio = A.ratio_fx, tsh = A.top_shift;
    auto cv = [&](const El& e) { return to_rp<F>(e, rtab, ratio, tsh); };
    auto ld = [&](const void* p, uint64_t r) { return cv(ld_el(p, r)); };
    auto K = [](const F& c) { return C{c}; };
    const C one = K(A.one), c2 = K(A.c2), c3 = K(A.c3), c4 = K(A.c4);
    uint32_t m = 0;
    const El e_arith = ld_el(A.q_arith, i), e_range = ld_el(A.q_range, i), e_logic = ld_el(A.q_logic, i), e_fixed = ld_el(A.q_fixed, i),
             e_var = ld_el(A.q_var, i);
    El e_pi;
    e_pi.a = e_pi.b = make_uint4(0, 0, 0, 0);
    if (A.pi) e_pi = ld_el(A.pi, i);
    const bool s_arith = !el_zero(e_arith), s_pi = !el_zero(e_pi), s_range = !el_zero(e_range), s_logic = !el_zero(e_logic),
               s_fixed = !el_zero(e_fixed), s_var = !el_zero(e_var);
    if (!(s_arith || s_pi || s_range || s_logic || s_fixed || s_var)) {
        mask[i] = 0;
        return;
    }
    const L a = ld(A.w_l, i), b = ld(A.w_r, i), c = ld(A.w_o, i), d = ld(A.w_4, i);
    if (s_arith) {   // q_arith * (q_m ab + q_l a + q_r b + q_o c + q_4 d + q_c) + pi   (widget/arithmetic.rs:51-63, quotient_poly.rs:262-266)
        const auto t = (a * b) * ld(A.q_m, i) + a * ld(A.q_l, i) + b * ld(A.q_r, i) + c * ld(A.q_o, i) + d * ld(A.q_4, i) + ld(A.q_c, i);
        if (nonzero(t * cv(e_arith) + cv(e_pi), one)) m |= 1u << BIT_ARITH;
    } else if (s_pi) {
        m |= 1u << BIT_ARITH;
    }
    if (s_range || s_logic || s_fixed || s_var) {
        const L a_n = ld(A.w_l, nx), b_n = ld(A.w_r, nx), d_n = ld(A.w_4, nx);
        if (s_range) {   // widget/range.rs:47-63
            if (nonzero(delta4(c - c4 * d, one, c2, c3), one)) m |= 1u << (BIT_RANGE + 0);
            if (nonzero(delta4(b - c4 * c, one, c2, c3), one)) m |= 1u << (BIT_RANGE + 1);
            if (nonzero(delta4(a - c4 * b, one, c2, c3), one)) m |= 1u << (BIT_RANGE + 2);
            if (nonzero(delta4(d_n - c4 * a, one, c2, c3), one)) m |= 1u << (BIT_RANGE + 3);
        }
        if (s_logic) {   // widget/logic.rs:65-133
            const auto la = a_n - c4 * a, lb = b_n - c4 * b, ldd = d_n - c4 * d;
            const auto ab = la + lb;
            // F = w [ w (4w - 18(a+b) + 81) + 18(a^2 + b^2) - 81(a+b) + 83 ]
            const auto in = (c4 * c - K(A.c18) * ab) + K(A.c81);
            const auto F1 = ((c * in + K(A.c18) * (zsqr(la) + zsqr(lb))) - K(A.c81) * ab) + K(A.c83);
            const auto Fw = c * F1;
            const auto E = K(A.c3) * (ab + ldd) - c2 * Fw;
            const auto Bq = ld(A.q_c, i) * (K(A.c9) * ldd - K(A.c3) * ab);
            if (nonzero(delta4(la, one, c2, c3), one)) m |= 1u << (BIT_LOGIC + 0);
            if (nonzero(delta4(lb, one, c2, c3), one)) m |= 1u << (BIT_LOGIC + 1);
            if (nonzero(delta4(ldd, one, c2, c3), one)) m |= 1u << (BIT_LOGIC + 2);
            if (nonzero(c - la * lb, one)) m |= 1u << (BIT_LOGIC + 3);
            if (nonzero(Bq + E, one)) m |= 1u << (BIT_LOGIC + 4);
        }
        if (s_fixed) {   // widget/ecc/fixed_base_scalar_mul.rs:88-156
            const L q_l = ld(A.q_l, i), q_r = ld(A.q_r, i), q_c = ld(A.q_c, i);
            const auto bit = (d_n - d) - d;
            const auto y_alpha = zsqr(bit) * (q_r - one) + one;
            const auto x_alpha = q_l * bit;
            const auto cabd = ((c * a) * b) * K(A.coeff_d);        // xy_alpha * acc_x * acc_y * D
            const auto x_lhs = a_n + a_n * cabd;
            const auto x_rhs = x_alpha * b + y_alpha * a;
            const auto y_lhs = b_n - b_n * cabd;
            const auto y_rhs = y_alpha * b - (K(A.coeff_a) * x_alpha) * a;
            if (nonzero((bit * (bit - one)) * (bit + one), one)) m |= 1u << (BIT_FIXED + 0);
            if (nonzero(bit * q_c - c, one)) m |= 1u << (BIT_FIXED + 1);
            if (nonzero(x_lhs - x_rhs, one)) m |= 1u << (BIT_FIXED + 2);
            if (nonzero(y_lhs - y_rhs, one)) m |= 1u << (BIT_FIXED + 3);
        }
        if (s_var) {   // x1 = a, x3 = a_n, y1 = b, y3 = b_n, x2 = c, y2 = d, x1*y2 = d_n   (widget/ecc/curve_addition.rs:62-97)
            const auto y1x2 = b * c, y1y2 = b * d, x1x2 = a * c;
            const auto dxy = (K(A.coeff_d) * d_n) * y1x2;
            if (nonzero(a * d - d_n, one)) m |= 1u << (BIT_CURVE + 0);
            if (nonzero((d_n + y1x2) - (a_n + a_n * dxy), one)) m |= 1u << (BIT_CURVE + 1);
            if (nonzero((y1y2 - K(A.coeff_a) * x1x2) - (b_n - b_n * dxy), one)) m |= 1u << (BIT_CURVE + 2);
        }
    }
    mask[i] = m;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline uint64_t capacity_for(uint64_t keys) {
    uint64_t cap = 2;
    while (cap < 2 * keys) cap <<= 1;
    return cap;
}

template <class Cv>
int check_impl(zk_ctx* c, uint32_t log_n, const zk_circuit_check_args* q, uint32_t* d_mask, zk_circuit_check_summary* out) {
    typedef typename Cv::Fr Fr;
    typedef typename Cv::FrU FU;
    if (!domain_log_ok<Cv>(log_n)) return ZK_ERR_DOMAIN_TOO_LARGE;
    if (log_n > ID_MAX_LOG_N) return ZK_ERR_UNSUPPORTED;
    const uint64_t n = (uint64_t)1 << log_n;
    const void* const cols[] = {q->w_l, q->w_r, q->w_o, q->w_4, q->q_m, q->q_l, q->q_r, q->q_o, q->q_4, q->q_c, q->q_arith, q->q_range, q->q_logic,
                                q->q_fixed_group_add, q->q_variable_group_add, q->q_lookup, q->sigma[0], q->sigma[1], q->sigma[2], q->sigma[3]};
    for (const void* p : cols)
        if (!p) return ZK_ERR_BAD_ARG;
    if (q->table_rows > n) return ZK_ERR_BAD_ARG;
    for (int k = 0; k < 4; ++k)
        if (q->table_rows && !q->table[k]) return ZK_ERR_BAD_ARG;

    const uint64_t cap_id = capacity_for(4 * n), cap_t = capacity_for(q->table_rows);
    const size_t o_sum = 256, o_args = HEAD, o_consts = o_args + up256(sizeof(CArgsU<FU>)), o_keys = o_consts + up256(ID_N_CONSTS * 32),
                 o_slots_id = o_keys + up256(4 * n * 32), o_slots_t = o_slots_id + up256(cap_id * 4), o_mask = o_slots_t + up256(cap_t * 4),
                 total = o_mask + (d_mask ? 0 : up256(n * 4));
    static_assert(sizeof(zk_circuit_check_summary) <= HEAD - 256, "the summary shares the head of the buffer with the flag word");
    DeviceAlloc wk;
    if (hipMalloc(&wk.base, total) != hipSuccess) {
        wk.base = nullptr;
        return zk_alloc_refused();
    }
    char* w = (char*)wk.base;
    uint32_t* d_flag = (uint32_t*)w;
    zk_circuit_check_summary* d_sum = (zk_circuit_check_summary*)(w + o_sum);
    uint32_t* slots_id = (uint32_t*)(w + o_slots_id);
    uint32_t* slots_t = (uint32_t*)(w + o_slots_t);
    uint32_t* mask = d_mask ? d_mask : (uint32_t*)(w + o_mask);
    void* id_keys = w + o_keys;
    hipStream_t st = c->stream;
    const Cols4 wires = {{q->w_l, q->w_r, q->w_o, q->w_4}};
    auto body = [&]() -> int {
        ZK_HIP_TRY(hipMemsetAsync(w, 0, HEAD, st));
        ZK_HIP_TRY(hipMemsetAsync(&d_sum->first_row, 0xff, 8, st));
        ZK_HIP_TRY(hipMemsetAsync(slots_id, 0xff, (size_t)cap_id * 4, st));
        ZK_HIP_TRY(hipMemsetAsync(slots_t, 0xff, (size_t)cap_t * 4, st));
        {   // the argument block of the gate kernel and the constants of the identity encodings: host copies live until zk_h2d returns
            CArgsU<FU> A;
            fill_gate_columns(A, q);
            fill_gate_consts<Cv>(A, q->coeff_a, q->coeff_d, CTAB);
            int r2 = zk_h2d(c, w + o_args, &A, sizeof A, st);
            if (r2) return r2;
            Fr cs[ID_N_CONSTS];
            fill_id_consts<Cv>(log_n, cs);
            r2 = zk_h2d(c, w + o_consts, cs, sizeof cs, st);
            if (r2) return r2;
        }
        {
            ProfScope ps(c, "check_gates");
            hipLaunchKernelGGL(check_gates<FU>, dim3(blocks_of(n, CT)), dim3(CT), 0, st, (const CArgsU<FU>*)(w + o_args), n, mask);
            ZK_HIP_TRY(hipGetLastError());
        }
        {
            ProfScope ps(c, "check_maps");
            hipLaunchKernelGGL(check_id_keys<Cv>, dim3(blocks_of(n, CT)), dim3(CT), 0, st, log_n, (const void*)(w + o_consts), id_keys);
            const KeyCols idc = {{id_keys, nullptr, nullptr, nullptr}};
            hipLaunchKernelGGL(map_build<1>, dim3(blocks_of(4 * n, CT)), dim3(CT), 0, st, slots_id, (uint32_t)(cap_id - 1), idc, 4 * n);
            if (q->table_rows) {
                const KeyCols tc = {{q->table[0], q->table[1], q->table[2], q->table[3]}};
                hipLaunchKernelGGL(map_build<4>, dim3(blocks_of(q->table_rows, CT)), dim3(CT), 0, st, slots_t, (uint32_t)(cap_t - 1), tc,
                                   (uint64_t)q->table_rows);
            }
            ZK_HIP_TRY(hipGetLastError());
        }
        {
            ProfScope ps(c, "check_copy");
            const Cols4 sg = {{q->sigma[0], q->sigma[1], q->sigma[2], q->sigma[3]}};
            hipLaunchKernelGGL(check_copy, dim3(blocks_of(4 * n, CT)), dim3(CT), 0, st, log_n, wires, sg, (const uint32_t*)slots_id,
                               (uint32_t)(cap_id - 1), (const void*)id_keys, mask, d_flag);
            ZK_HIP_TRY(hipGetLastError());
        }
        {
            ProfScope ps(c, "check_lookup");
            const KeyCols tc = {{q->table[0], q->table[1], q->table[2], q->table[3]}};
            hipLaunchKernelGGL(check_lookup, dim3(blocks_of(n, CT)), dim3(CT), 0, st, n, wires, q->q_lookup, (const uint32_t*)slots_t,
                               (uint32_t)(cap_t - 1), tc, (uint64_t)q->table_rows, mask);
            ZK_HIP_TRY(hipGetLastError());
        }
        ProfScope ps(c, "check_summary");
        hipLaunchKernelGGL(check_summary, dim3(blocks_of(n, CT)), dim3(CT), 0, st, (const uint32_t*)mask, n, d_sum);
        hipLaunchKernelGGL(check_finish, dim3(1), dim3(64), 0, st, (const uint32_t*)mask, n, d_sum);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    };
    int rc = body();
    struct {
        uint32_t flag[64];
        zk_circuit_check_summary sum;
    } head;
    static_assert(sizeof head <= HEAD, "flag word and summary are read back as one block");
    if (!rc) rc = zk_d2h(c, &head, w, sizeof head, st);          // the one read-back; also the wait before the buffer is freed
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (head.flag[0]) return ZK_ERR_BAD_ARG;
    *out = head.sum;
    return ZK_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_circuit_check_dev(zk_ctx* c, int curve_id, uint32_t log_n, const void* args, void* d_mask, void* out) {
    if (!c || !args || !out || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return check_impl<decltype(cv)>(c, log_n, (const zk_circuit_check_args*)args, (uint32_t*)d_mask, (zk_circuit_check_summary*)out);
    });
}
