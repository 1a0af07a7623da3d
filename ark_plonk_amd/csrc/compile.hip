// Circuit compilation on the device: the one piece of `Circuit::compile` (circuit.rs:226-259 -> preprocess.rs:126-423) the library
// did not have -- the wire permutation (`Permutation::compute_sigma_permutations` + `compute_permutation_lagrange`,
// plonk-core/src/permutation/mod.rs:101-169) -- and the witness step `to_scalars` (prover.rs:188-192) as a gather.
//
// zk_perm_sigma_dev.  The reference keeps a hash map variable -> list of positions in the order `add_variable_to_map` was called and
// rotates every list by one.  Here the call sequence (ins_var[k], ins_pos[k]), k < m, is sorted by variable with a STABLE
// least-significant-digit radix sort (8 bits a pass, only as many passes as num_vars has bits), so that every variable's positions are
// one contiguous run in call order; sigma of a run's element is its right neighbour, of the last element the run's first.
//   sigma_check      range of every (variable, position)                                   -> flag word
//   sigma_sort_pass  <false>: digit counts per tile [digit][tile]; exclusive scan (dev_scan.cuh); <true>: stable scatter
//   sigma_rotate     sigma_pos[pos_j] = pos of the right neighbour / of the run's head      (a second write of one cell -> flag word)
//   sigma_encode     never-inserted cells -> themselves; evals[w][row] = K_w' * omega^row'
// Skew is the normal case (every unused wire of every gate is the zero variable, composer.rs:308): no step gives a variable's run to
// one lane, wave or workgroup.  The sort works on tiles of the call sequence whatever the keys are -- equal digits inside a wave are
// ranked with ballots, not with atomics on a shared counter -- and the only per-run work is the search for the run's head by the lane
// that holds its LAST element: a galloping search backwards (1, 2, 4, ... cells) and a bisection, i.e. O(log run length) reads for the
// one lane of a long run and two or three neighbouring reads for the short runs that make up the rest.
// Nothing depends on the arrival order of an atomic: the ranks come from lane order, every cell of sigma_pos is written once (a second
// write is the "inserted twice" error), and the flag word is only ever OR-ed.
//
// Working memory: one allocation per call, freed before return (so the calls use no buffer of the ctx and run inside an open deferred
// round).  With m <= 4n insertions: 16 m bytes (two key/value buffer pairs; 8 m when one pass is enough, none when num_vars = 1)
// + m / 4 (digit counts) + 16 n when the caller takes no positions + 2 KiB.  At most 81 n bytes: 340 MB at n = 2^22.
#include "api_internal.h"
#include "dev_scan.cuh"
#include "domain.cuh"

namespace {

constexpr uint32_t NO_POS = 0xffffffffu;          // a cell of sigma_pos nothing was written to (positions are < 2^30)
constexpr uint32_t FLAG_RANGE = 1, FLAG_TWICE = 2;

constexpr uint32_t SORT_T = 256;                  // lanes per tile
constexpr uint32_t SORT_WAVES = SORT_T / 64;
constexpr uint32_t SORT_ITEMS = 16;               // keys per lane
constexpr uint32_t WAVE_ITEMS = 64 * SORT_ITEMS;  // a wave owns this many CONSECUTIVE keys of the tile, 64 at a time
constexpr uint32_t SORT_TILE = SORT_T * SORT_ITEMS;
constexpr uint32_t RADIX = 256;

constexpr uint32_t SCAN_T = 256, SCAN_ITEMS = 4, SCAN_CHUNK = SCAN_T * SCAN_ITEMS;      // the geometry of the digit counts' scan (dev_scan.cuh)

// ---------------------------------------------------------------------------------------------------------------- range check
// Every entry is looked at before any kernel uses one as an address; the kernels below guard their own writes as well, so a bad
// entry costs a flag and a wrong (discarded) result, never an access outside the buffers.
__global__ void __launch_bounds__(256) sigma_check(const uint32_t* ins_var, const uint32_t* ins_pos, uint64_t m, uint32_t num_vars,
                                                   uint32_t n_pos, uint32_t* flag) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    if (ins_var[k] >= num_vars || ins_pos[k] >= n_pos) atomicOr(flag, FLAG_RANGE);
}

// ---------------------------------------------------------------------------------------------------------------- stable radix pass
// lanes of the wave whose digit equals this lane's (active lanes only): one ballot per digit bit
ZK_D uint64_t match_digit(uint32_t d, bool active) {
    uint64_t m = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(active && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// One pass over digit (key >> shift) & 255.  Tile `blockIdx.x` holds keys [tile * SORT_TILE, ...); wave w of it the WAVE_ITEMS keys from
// w * WAVE_ITEMS on, 64 consecutive keys per step, so that (tile, wave, step, lane) is the order of the keys themselves.
// SCATTER = false: hist[digit * n_tiles + tile] = keys of the tile with that digit.
// SCATTER = true:  hist holds the exclusive scan of those counts (digit-major: all smaller digits, then the same digit in earlier
// tiles); a key goes to that base + keys with its digit in earlier waves of the tile + in earlier steps of its wave + in lower lanes.
template <bool SCATTER>
__global__ void __launch_bounds__(SORT_T) sigma_sort_pass(const uint32_t* key_in, const uint32_t* val_in, uint64_t m, uint32_t shift,
                                                          uint32_t n_tiles, uint32_t* hist, uint32_t* key_out, uint32_t* val_out) {
    __shared__ uint32_t wcount[SORT_WAVES][RADIX];
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
    for (uint32_t i = t; i < SORT_WAVES * RADIX; i += SORT_T) (&wcount[0][0])[i] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)w * WAVE_ITEMS + lane;
    const uint64_t lower = ((uint64_t)1 << lane) - 1;
    uint32_t key[SORT_ITEMS], rank[SORT_ITEMS];
#pragma unroll
    for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
        const uint64_t idx = first + (uint64_t)r * 64;
        const bool active = idx < m;
        const uint32_t k = active ? key_in[idx] : 0u;
        const uint32_t d = (k >> shift) & (RADIX - 1);
        const uint64_t same = match_digit(d, active);
        const uint32_t below = (uint32_t)__popcll(same & lower);
        // the wave's running count of the digit: every lane reads it, then the lowest lane of each digit group adds the group
        const uint32_t before = active ? wcount[w][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (active && below == 0) wcount[w][d] = before + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        key[r] = k;
        rank[r] = before + below;
    }
    __syncthreads();
    {   // lane t = digit t: the waves' totals -> the tile's count, or each wave's base in the output
        uint32_t run = SCATTER ? hist[(size_t)t * n_tiles + blockIdx.x] : 0u;
#pragma unroll
        for (uint32_t v = 0; v < SORT_WAVES; ++v) {
            const uint32_t cnt = wcount[v][t];
            if (SCATTER) wcount[v][t] = run;
            run += cnt;
        }
        if (!SCATTER) hist[(size_t)t * n_tiles + blockIdx.x] = run;
    }
    if (!SCATTER) return;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < SORT_ITEMS; ++r) {
        const uint64_t idx = first + (uint64_t)r * 64;
        if (idx < m) {
            const uint32_t d = (key[r] >> shift) & (RADIX - 1);
            const uint64_t dst = (uint64_t)wcount[w][d] + rank[r];
            if (dst < m) {                                  // always: the bases are a scan of counts that sum to m
                key_out[dst] = key[r];
                val_out[dst] = val_in[idx];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- rotate
// var_s / pos_s: the call sequence sorted by variable (runs in call order).  Lane j writes sigma of ITS position.
__global__ void __launch_bounds__(256) sigma_rotate(const uint32_t* var_s, const uint32_t* pos_s, uint64_t m, uint32_t n_pos,
                                                    uint32_t* sigma_pos, uint32_t* flag) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t v = var_s[j], p = pos_s[j];
    uint64_t src = j + 1;
    if (src >= m || var_s[src] != v) {
        // the last element of its run: find the run's head.  good: an index of the run; bad: an index before it.
        uint64_t good = j, bad = 0, step = 1;
        bool have_bad = false;
        while (good > 0) {
            const uint64_t probe = good >= step ? good - step : 0;
            if (var_s[probe] == v) {
                good = probe;
                step <<= 1;
            } else {
                bad = probe;
                have_bad = true;
                break;
            }
        }
        if (have_bad)
            while (good - bad > 1) {
                const uint64_t mid = bad + ((good - bad) >> 1);
                if (var_s[mid] == v)
                    good = mid;
                else
                    bad = mid;
            }
        src = good;
    }
    if (p >= n_pos) return;                                // flagged by sigma_check
    if (atomicExch(&sigma_pos[p], pos_s[src]) != NO_POS) atomicOr(flag, FLAG_TWICE);
}

// ---------------------------------------------------------------------------------------------------------------- encode
// consts: fill_id_consts (domain.cuh)
struct EvalPtrs {
    void* p[4];
};
template <class Cv>
__global__ void __launch_bounds__(256) sigma_encode(uint32_t* sigma_pos, uint32_t log_n, const void* consts, EvalPtrs out) {
    typedef typename Cv::Fr Fr;
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = (uint64_t)1 << log_n;
    if (p >= 4 * n) return;
    uint32_t s = sigma_pos[p];
    if (s >= 4 * n) {                                      // never inserted (or the discarded result of a refused call): itself
        s = (uint32_t)p;
        sigma_pos[p] = s;
    }
    if (!out.p[0]) return;
    const uint32_t row = s & (uint32_t)(n - 1);
    const Fr r = id_encode<Fr>(consts, s >> log_n, row, log_n);
    const uint32_t w = (uint32_t)(p >> log_n);
    void* dst = w == 0 ? out.p[0] : w == 1 ? out.p[1] : w == 2 ? out.p[2] : out.p[3];
    st_fr<Fr>(dst, p & (n - 1), r);
}

// ---------------------------------------------------------------------------------------------------------------- gather
template <class Cv>
__global__ void __launch_bounds__(256) fr_gather(const void* values, uint64_t num_values, const uint32_t* index, uint64_t n, void* out,
                                                 uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = index[i];
    if (k >= num_values) {
        atomicOr(flag, FLAG_RANGE);
        return;
    }
    st_fr<Fr>(out, i, ld_fr<Fr>(values, k));
}

// ---------------------------------------------------------------------------------------------------------------- host side
template <class Cv>
int sigma_impl(zk_ctx* c, uint32_t log_n, const uint32_t* ins_var, const uint32_t* ins_pos, size_t m, uint32_t num_vars,
               uint32_t* d_sigma_pos, void* const* d_evals) {
    typedef typename Cv::Fr Fr;
    if (!domain_log_ok<Cv>(log_n)) return ZK_ERR_DOMAIN_TOO_LARGE;
    if (log_n > ID_MAX_LOG_N) return ZK_ERR_UNSUPPORTED;
    const uint64_t n = (uint64_t)1 << log_n, n_pos = 4 * n;
    if (m > n_pos) return ZK_ERR_BAD_ARG;
    // radix passes: as many as num_vars - 1 has digits (none when there is one variable: the call sequence is its run)
    uint32_t bits = 0;
    while (bits < 32 && num_vars > 1 && ((uint64_t)(num_vars - 1) >> bits) != 0) ++bits;
    const uint32_t passes = m ? (bits + 7) / 8 : 0;
    const uint64_t n_tiles = blocks_of(m, SORT_TILE);
    const uint64_t hist_len = passes ? RADIX * n_tiles : 0;
    // offsets behind the flag word (run_flagged)
    const size_t o_consts = 0, o_hist = o_consts + up256(ID_N_CONSTS * 32), o_sums = o_hist + up256(hist_len * 4),
                 o_sort = o_sums + up256(blocks_of(hist_len, SCAN_CHUNK) * 4), sort_one = up256(m * 4),
                 o_pos = o_sort + (passes >= 2 ? 4 : passes ? 2 : 0) * sort_one, total = o_pos + (d_sigma_pos ? 0 : up256(n_pos * 4));
    hipStream_t st = c->stream;
    return run_flagged(c, total, [&](uint32_t* d_flag, void* work) -> int {
        char* w = (char*)work;
        uint32_t* d_hist = (uint32_t*)(w + o_hist);
        uint32_t* d_sums = (uint32_t*)(w + o_sums);
        uint32_t* sigma_pos = d_sigma_pos ? d_sigma_pos : (uint32_t*)(w + o_pos);
        ZK_HIP_TRY(hipMemsetAsync(sigma_pos, 0xff, n_pos * 4, st));
        if (m) {
            const uint32_t* var_s = ins_var;
            const uint32_t* pos_s = ins_pos;
            {
                ProfScope ps(c, "perm_sigma_sort");
                hipLaunchKernelGGL(sigma_check, dim3(blocks_of(m, 256)), dim3(256), 0, st, ins_var, ins_pos, (uint64_t)m, num_vars,
                                   (uint32_t)n_pos, d_flag);
                for (uint32_t i = 0; i < passes; ++i) {
                    uint32_t* key_out = (uint32_t*)(w + o_sort + (size_t)(2 * (i & 1u)) * sort_one);
                    uint32_t* val_out = (uint32_t*)(w + o_sort + (size_t)(2 * (i & 1u) + 1) * sort_one);
                    hipLaunchKernelGGL(sigma_sort_pass<false>, dim3((unsigned)n_tiles), dim3(SORT_T), 0, st, var_s, pos_s, (uint64_t)m, 8 * i,
                                       (uint32_t)n_tiles, d_hist, (uint32_t*)nullptr, (uint32_t*)nullptr);
                    scan_excl<uint32_t, SCAN_T, SCAN_ITEMS>(d_hist, d_hist, hist_len, d_sums, nullptr, st);
                    hipLaunchKernelGGL(sigma_sort_pass<true>, dim3((unsigned)n_tiles), dim3(SORT_T), 0, st, var_s, pos_s, (uint64_t)m, 8 * i,
                                       (uint32_t)n_tiles, d_hist, key_out, val_out);
                    var_s = key_out;
                    pos_s = val_out;
                }
                ZK_HIP_TRY(hipGetLastError());
            }
            ProfScope ps(c, "perm_sigma_rotate");
            hipLaunchKernelGGL(sigma_rotate, dim3(blocks_of(m, 256)), dim3(256), 0, st, var_s, pos_s, (uint64_t)m, (uint32_t)n_pos,
                               sigma_pos, d_flag);
            ZK_HIP_TRY(hipGetLastError());
        }
        EvalPtrs out = {{nullptr, nullptr, nullptr, nullptr}};
        if (d_evals) {
            for (int k = 0; k < 4; ++k) out.p[k] = d_evals[k];
            Fr cs[ID_N_CONSTS];
            fill_id_consts<Cv>(log_n, cs);
            const int r2 = zk_h2d(c, w + o_consts, cs, sizeof cs, st);
            if (r2) return r2;
        }
        ProfScope ps(c, "perm_sigma_encode");
        hipLaunchKernelGGL(sigma_encode<Cv>, dim3(blocks_of(n_pos, 256)), dim3(256), 0, st, sigma_pos, log_n,
                           (const void*)(w + o_consts), out);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

template <class Cv>
int gather_impl(zk_ctx* c, const void* d_values, size_t num_values, const uint32_t* d_index, size_t n, void* d_out) {
    return run_flagged(c, 0, [&](uint32_t* d_flag, void*) -> int {
        ProfScope ps(c, "fr_gather");
        hipLaunchKernelGGL(fr_gather<Cv>, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, d_values, (uint64_t)num_values, d_index,
                           (uint64_t)n, d_out, d_flag);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_perm_sigma_dev(zk_ctx* c, int curve_id, uint32_t log_n, const void* d_ins_var, const void* d_ins_pos, size_t m, uint32_t num_vars,
                      void* d_sigma_pos, void* const* d_sigma_evals) {
    if (!c || !zk_curve_ok(curve_id) || (m && (!d_ins_var || !d_ins_pos)) || (!d_sigma_pos && !d_sigma_evals)) return ZK_ERR_BAD_ARG;
    if (d_sigma_evals)
        for (int k = 0; k < 4; ++k)
            if (!d_sigma_evals[k]) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return sigma_impl<decltype(cv)>(c, log_n, (const uint32_t*)d_ins_var, (const uint32_t*)d_ins_pos, m, num_vars, (uint32_t*)d_sigma_pos,
                                        d_sigma_evals);
    });
}

int zk_fr_gather_dev(zk_ctx* c, int curve_id, const void* d_values, size_t num_values, const void* d_index, size_t n, void* d_out) {
    if (!c || !zk_curve_ok(curve_id) || (n && (!d_values || !d_index || !d_out))) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG,
                       [&](auto cv) { return gather_impl<decltype(cv)>(c, d_values, num_values, (const uint32_t*)d_index, n, d_out); });
}
