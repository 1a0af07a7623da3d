// The output of a lookup on the device: `LookupTable::lookup` (plonk-core/src/lookup/lookup_table.rs:172-180) computes c from
// (a, b, d) as the c of the FIRST row whose columns 0, 1 and 3 match -- `.position(..)` returns the first match, and rows with one
// key and different c are legal -- and `WitnessTable::value_from_table` (lookup/witness_table.rs:48-67) is how a circuit gets the
// output of a lookup gate.  The reference scans the table per query; here the table gets a map once and a query is one probe.
//
//   lookup_map_build   one lane per table row: an open-addressing map (linear probing, capacity = the power of two >= 2 x rows, so at
//                      most half full) over the keys (a, b, d) -- Key<3>, key_hash<3>: fr_io.cuh -- whose slots hold row INDICES.  A
//                      lane claims an empty slot by compare-and-swap; a lane that meets an occupant compares the occupant's key in
//                      full and, when it is its own, lowers the slot to its index by atomicMin (lookup.hip's claim-then-minimum).
//                      Every index a slot ever holds carries the slot's key, so afterwards every distinct key names the SMALLEST row
//                      that holds it, whatever order the lanes arrive in; which slot of a probe chain a key sits in may depend on
//                      the order, what the map answers does not.
//   lookup_map_query   one lane per query: the three operands read directly or through an index vector (the witness replay reads
//                      values[id]), one probe with every occupant on the way compared in full, c of the row found copied to the
//                      output (directly or through an index vector), optionally the row index.  Read-only on the map and the
//                      table.  A miss writes 0xFFFFFFFF to its position and costs the flag atomics: per wavefront ONE atomicAdd of
//                      the ballot's population count and ONE atomicMin of the first missing lane's query (lane order is query
//                      order).  An index outside its vector raises the flag word; such a query reads and writes nothing.
// The build has NO wave-leader election for duplicate keys (lookup.hip: wave_value_leader): that exists for the padded multisets of
// the prover's round 2, where one value fills most of a vector.  A `LookupTable` holds the rows a circuit inserted -- the
// insert_multi_* blocks have pairwise distinct keys, the dummy table has three rows -- and is never padded here, so duplicates are
// the rare case and one atomicMin per duplicate lane is cheaper than the election's shuffles on every wavefront.  The queries of a
// benchmark-style circuit all read the same one or two slots: that is read contention on cached lines, not an atomic.
// Elements are compared and copied as 32-byte words (El), so no kernel is instantiated on the field; curve_id is validated only.
//
// Working memory of a query: one allocation of 256 bytes (flag word, miss count, first miss), freed on every path, read back once;
// no buffer of the ctx, so both calls run inside an open deferred round.
#include "api_internal.h"
#include "fr_io.cuh"

namespace {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t LT = 256;                      // lanes per workgroup, both kernels
constexpr uint64_t MAX_TABLE_ROWS = (uint64_t)1 << 30;     // slots <= 2^31: indices and the slot mask are 32-bit
constexpr size_t MIN_SLOTS = 64;
constexpr uint32_t FLAG_INDEX = 1;
constexpr uint32_t W_FLAG = 0, W_MISSES = 1, W_FIRST = 2;   // words of the state block

inline size_t map_slots(uint64_t rows) {
    if (rows > MAX_TABLE_ROWS) return 0;
    size_t s = MIN_SLOTS;
    while (s < 2 * rows) s <<= 1;
    return s;
}

// slots: all EMPTY before the launch; keys.col[0 .. 3): the columns a, b, d
__global__ void __launch_bounds__(LT) lookup_map_build(KeyCols keys, uint32_t rows, uint32_t* slots, uint32_t mask) {
    const uint32_t i = blockIdx.x * LT + threadIdx.x;
    if (i >= rows) return;
    const Key<3> k = ld_key<3>(keys, i);
    uint32_t s = key_hash<3>(k) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {          // the map is at most half full: an empty slot ends the walk long before
        uint32_t cur = slots[s];
        if (cur == EMPTY) {
            cur = atomicCAS(&slots[s], EMPTY, i);
            if (cur == EMPTY) return;
        }
        if (key_eq<3>(ld_key<3>(keys, cur), k)) {            // the key columns are read-only: an index, once seen, names its key
            if (cur > i) atomicMin(&slots[s], i);
            return;
        }
        s = (s + 1) & mask;
    }
}

// one operand of the queries: element i, or element ids[i]; a null vector reads as zero (an input a gadget segment does not have)
struct Operand {
    const void* vec;
    const uint32_t* ids;
    uint64_t bound;                                          // elements in vec
};
struct QueryArgs {
    KeyCols keys;                                            // a, b, d of the table
    const void* table_c;
    uint32_t rows;
    const uint32_t* slots;
    uint32_t mask;
    uint32_t n;
    Operand op[3];
    void* out;
    const uint32_t* out_ids;
    uint64_t out_bound;
    uint32_t* pos;                                           // or null
    uint32_t* state;                                         // W_FLAG, W_MISSES, W_FIRST
};

__global__ void __launch_bounds__(LT) lookup_map_query(QueryArgs q) {
    const uint32_t i = blockIdx.x * LT + threadIdx.x;
    bool live = i < q.n;
    Key<3> k;
    uint64_t jo = 0;
    if (live) {
        bool bad = false;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            k.e[w].a = k.e[w].b = make_uint4(0, 0, 0, 0);
            if (!q.op[w].vec) continue;
            const uint64_t j = q.op[w].ids ? q.op[w].ids[i] : i;
            if (j < q.op[w].bound)
                k.e[w] = ld_el(q.op[w].vec, j);
            else
                bad = true;
        }
        jo = q.out_ids ? q.out_ids[i] : i;
        bad = bad || jo >= q.out_bound;
        if (bad) {
            atomicOr(&q.state[W_FLAG], FLAG_INDEX);
            live = false;
        }
    }
    uint32_t found = EMPTY;
    if (live) {
        uint32_t s = key_hash<3>(k) & q.mask;
        for (uint32_t step = 0; step <= q.mask; ++step) {
            const uint32_t idx = q.slots[s];
            if (idx >= q.rows) break;                        // EMPTY; or no index of this table: a miss, never an address
            if (key_eq<3>(ld_key<3>(q.keys, idx), k)) {
                found = idx;
                break;
            }
            s = (s + 1) & q.mask;
        }
        if (found != EMPTY) st_el(q.out, jo, ld_el(q.table_c, found));
    }
    if (i < q.n && q.pos) q.pos[i] = found;
    const uint64_t missing = __ballot(live && found == EMPTY);
    if (missing && (int)(threadIdx.x & 63u) == __ffsll((long long)missing) - 1) {
        atomicAdd(&q.state[W_MISSES], (uint32_t)__popcll(missing));
        atomicMin(&q.state[W_FIRST], i);
    }
}

struct QueryCall {
    const void* table[4];
    uint64_t rows;
    const void* slots;
    uint64_t n_slots;
    uint64_t n;
    Operand op[3];
    void* out;
    const uint32_t* out_ids;
    uint64_t out_bound;
    void* pos;
};

// ctx lock held.  The table, the map and the operand vectors have been checked by the caller for null pointers.
int query_locked(zk_ctx* c, const QueryCall& qc, uint64_t* misses, uint64_t* first_miss) {
    if (misses) *misses = 0;
    if (first_miss) *first_miss = qc.n;
    if (qc.n >= ((uint64_t)1 << 32)) return ZK_ERR_UNSUPPORTED;
    if (qc.rows > MAX_TABLE_ROWS) return ZK_ERR_UNSUPPORTED;
    if (qc.n_slots != map_slots(qc.rows)) return ZK_ERR_BAD_ARG;
    if (qc.n == 0) return ZK_OK;
    DeviceAlloc wk;
    if (hipMalloc(&wk.base, 256) != hipSuccess) {
        wk.base = nullptr;
        return zk_alloc_refused();
    }
    hipStream_t st = c->stream;
    QueryArgs q;
    q.keys.col[0] = qc.table[0], q.keys.col[1] = qc.table[1], q.keys.col[2] = qc.table[3], q.keys.col[3] = nullptr;
    q.table_c = qc.table[2];
    q.rows = (uint32_t)qc.rows;
    q.slots = (const uint32_t*)qc.slots;
    q.mask = (uint32_t)(qc.n_slots - 1);
    q.n = (uint32_t)qc.n;
    for (int w = 0; w < 3; ++w) q.op[w] = qc.op[w];
    q.out = qc.out, q.out_ids = qc.out_ids, q.out_bound = qc.out_bound;
    q.pos = (uint32_t*)qc.pos;
    q.state = (uint32_t*)wk.base;
    uint32_t state[3] = {0, 0, 0};
    int rc = [&]() -> int {
        ProfScope ps(c, "lookup_map_query");
        ZK_HIP_TRY(hipMemsetAsync(q.state, 0, 256, st));
        ZK_HIP_TRY(hipMemsetAsync(q.state + W_FIRST, 0xff, 4, st));
        hipLaunchKernelGGL(lookup_map_query, dim3(blocks_of(qc.n, LT)), dim3(LT), 0, st, q);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    }();
    if (!rc) rc = zk_d2h(c, state, q.state, sizeof state, st);          // the one read-back; also the wait before the buffer is freed
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (state[W_FLAG]) return ZK_ERR_BAD_ARG;
    if (misses) *misses = state[W_MISSES];
    if (first_miss && state[W_MISSES]) *first_miss = state[W_FIRST];
    return state[W_MISSES] ? ZK_ERR_NOT_INDEXED : ZK_OK;
}

}  // namespace

// ---- api_internal.h: the witness of a ZK_GADGET_LOOKUP_OUT segment (gadget_witness.hip).  ctx lock held, the segment's shape checked.
int lookup_out_witness(zk_ctx* c, const zk_gadget_args& a, void* d_values) {
    if (!a.lut_map) return ZK_ERR_BAD_ARG;
    for (int w = 0; w < 4; ++w)
        if (!a.lut[w] && a.lut_rows) return ZK_ERR_BAD_ARG;
    QueryCall qc;
    for (int w = 0; w < 4; ++w) qc.table[w] = a.lut[w];
    qc.rows = a.lut_rows, qc.slots = a.lut_map, qc.n_slots = a.lut_slots, qc.n = a.calls;
    for (int w = 0; w < 3; ++w) {                            // an id that is not below var0 names no variable defined before the segment
        const uint32_t* ids = (const uint32_t*)a.inputs_ext[w];
        qc.op[w] = {ids ? d_values : nullptr, ids, a.var0};
    }
    qc.out = (char*)d_values + 32 * a.var0, qc.out_ids = nullptr, qc.out_bound = a.calls;
    qc.pos = nullptr;
    return query_locked(c, qc, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------------------------------ C ABI
size_t zk_lookup_map_slots(size_t rows) { return map_slots(rows); }

int zk_lookup_map_build_dev(zk_ctx* c, int curve_id, const void* d_a, const void* d_b, const void* d_d, size_t rows, void* d_slots, size_t slots) {
    if (!c || !zk_curve_ok(curve_id) || !d_slots) return ZK_ERR_BAD_ARG;
    if (rows && (!d_a || !d_b || !d_d)) return ZK_ERR_BAD_ARG;
    if (rows > MAX_TABLE_ROWS) return ZK_ERR_UNSUPPORTED;
    if (slots != map_slots(rows)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    ProfScope ps(c, "lookup_map_build");
    ZK_HIP_TRY(hipMemsetAsync(d_slots, 0xff, slots * 4, c->stream));
    if (rows == 0) return ZK_OK;
    KeyCols keys = {{d_a, d_b, d_d, nullptr}};
    hipLaunchKernelGGL(lookup_map_build, dim3(blocks_of(rows, LT)), dim3(LT), 0, c->stream, keys, (uint32_t)rows, (uint32_t*)d_slots,
                       (uint32_t)(slots - 1));
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

int zk_lookup_map_query_dev(zk_ctx* c, int curve_id, const void* const d_table[4], size_t rows, const void* d_slots, size_t slots, size_t n,
                            const void* const* d_operands, const void* const* d_operand_ids, size_t operand_rows, void* d_out,
                            const void* d_out_ids, size_t out_rows, void* d_pos, uint64_t* misses, uint64_t* first_miss) {
    if (!c || !zk_curve_ok(curve_id) || !d_table || !d_slots || !d_operands || !d_out) return ZK_ERR_BAD_ARG;
    QueryCall qc;
    for (int w = 0; w < 4; ++w) {
        if (!d_table[w] && rows) return ZK_ERR_BAD_ARG;
        qc.table[w] = d_table[w];
    }
    for (int w = 0; w < 3; ++w) {
        if (!d_operands[w]) return ZK_ERR_BAD_ARG;
        const uint32_t* ids = d_operand_ids ? (const uint32_t*)d_operand_ids[w] : nullptr;
        if (!ids && operand_rows < n) return ZK_ERR_BAD_ARG;
        qc.op[w] = {d_operands[w], ids, operand_rows};
    }
    if (!d_out_ids && out_rows < n) return ZK_ERR_BAD_ARG;
    qc.rows = rows, qc.slots = d_slots, qc.n_slots = slots, qc.n = n;
    qc.out = d_out, qc.out_ids = (const uint32_t*)d_out_ids, qc.out_bound = out_rows;
    qc.pos = d_pos;
    Guard g(c);
    return query_locked(c, qc, misses, first_miss);
}
