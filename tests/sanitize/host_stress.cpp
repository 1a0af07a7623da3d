// TEST INFRASTRUCTURE (tests/test_sanitize.py): the host side of the whole library under a sanitizer, without a GPU.
// Linked with fake_hip.cpp (device memory = zeroed host memory, kernel launches do nothing), so every device result is the
// all-zero pattern: the point at infinity / the zero digest.  What is exercised for real is everything the sanitizers can see:
//   * the device-scoped, content-addressed, reference-counted SRS registry (zk_srs_register from several threads with the same and
//     with different bytes, zk_srs_retain / zk_srs_free, eviction through zk_srs_cache_config, zk_srs_precompute under readers);
//   * threads sharing ONE zk_ctx and threads with a ctx each over one SRS -- the pattern of tests/test_concurrency_gpu.py --
//     through the host-pointer entry points (staging buffers, pinned ring, copy stream bookkeeping), blocking batches,
//     deferred rounds (begin / open_begin / reduce / end / abort, the ZK_ERR_PENDING refusals), the commitment cache (LRU list);
//   * the persistent host pool (HostPool::run from several ctxs at once) and the host tails of a round;
//   * with REAL points: zk_g1_sum_partials(_batch) -- Jacobian -> XYZZ, host additions incl. doubling and cancellation, Fermat
//     inversion, affine normalisation -- on the group generator decoded by wire.hip's own deserialiser;
//   * every allocation of one pass over the library refused in turn (section 2d: the codes returned, the ctx afterwards, what is left
//     allocated), under a fake runtime that keeps its last error until it is read, as the real one does;
//   * a residency-cache hit whose device copy is wrong, under option "cache_verify" (section 2e).
// Exit code 0 and "host_stress ok" = every call returned what it must; the sanitizer's own report fails the test otherwise.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "ark_plonk_amd.h"

extern "C" long fake_hip_launches();
extern "C" long fake_hip_live_allocations();
extern "C" void fake_hip_set_memory(size_t budget, size_t report_extra);
extern "C" size_t fake_hip_live_bytes();
extern "C" long fake_hip_fail_alloc_after(long k);          // the k-th allocation from now fails once (negative: off); returns what was left
extern "C" long fake_hip_flip_byte(size_t alloc_bytes);     // inverts the first byte of every live allocation of that size; returns how many
void zk_process_key_reset_for_tests(const char* path);      // csrc/hostio.hip: test hook, not part of the C ABI

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "host_stress: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

static const int CURVE = ZK_CURVE_BLS12_381;
static const size_t L = 6;      // u64 limbs of Fq

// the standard compressed encodings of the BLS12-381 G1 generator in ark-serialize's form (x little-endian, flags in the last byte):
// decoded by the library itself, so the harness needs no field arithmetic of its own
static int generator(uint64_t* xy, bool negate) {
    static const uint8_t gx_be[48] = {0x17, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f,
                                      0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05, 0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58,
                                      0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};
    uint8_t enc[48];
    for (int i = 0; i < 48; ++i) enc[i] = gx_be[47 - i];
    uint8_t inf = 0;
    // the sign bit selects one of the two points with this x; try both and keep the one asked for (y differs, x is equal)
    uint64_t a[12], b[12];
    enc[47] &= 0x3f;
    if (zk_g1_deserialize_compressed(CURVE, enc, a, &inf) != ZK_OK || inf) return 1;
    enc[47] |= 0x80;
    if (zk_g1_deserialize_compressed(CURVE, enc, b, &inf) != ZK_OK || inf) return 1;
    if (memcmp(a, b, 48) != 0 || memcmp(a + 6, b + 6, 48) == 0) return 1;
    memcpy(xy, negate ? b : a, 96);
    return 0;
}

static int real_point_arithmetic() {
    uint64_t g[12], ng[12], one[6], out[12], two_g[12], again[12];
    uint8_t inf = 0;
    REQUIRE(generator(g, false) == 0 && generator(ng, true) == 0);
    // Montgomery one of Fq: the y of GroupAffine::zero() = (0, 1), which is what an empty sum returns
    REQUIRE(zk_g1_sum_partials(CURVE, nullptr, 0, out, &inf) == ZK_OK && inf == 1);
    memcpy(one, out + 6, 48);
    auto jac = [&](const uint64_t* xy, uint64_t* p) {
        memcpy(p, xy, 96);
        memcpy(p + 12, one, 48);
    };
    uint64_t parts[4 * 18];
    jac(g, parts);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 1, out, &inf) == ZK_OK && !inf && memcmp(out, g, 96) == 0);          // G
    jac(g, parts + 18);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 2, two_g, &inf) == ZK_OK && !inf && memcmp(two_g, g, 96) != 0);      // G + G: the doubling branch
    jac(ng, parts + 18);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 2, out, &inf) == ZK_OK && inf == 1);                                 // G - G: infinity
    jac(two_g, parts);
    jac(ng, parts + 18);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 2, out, &inf) == ZK_OK && !inf && memcmp(out, g, 96) == 0);          // 2G - G = G
    // batch form: 3 ranks x 2 jobs, rank-major; job 0 = G + G - G, job 1 = 2G - G + infinity
    uint64_t batch[3 * 2 * 18];
    memset(batch, 0, sizeof batch);
    jac(g, batch + 0 * 18);
    jac(two_g, batch + 1 * 18);
    jac(g, batch + 2 * 18);
    jac(ng, batch + 3 * 18);
    jac(ng, batch + 4 * 18);
    memcpy(batch + 5 * 18, one, 48);                 // (1, 1, 0): Jacobian zero as arkworks writes it
    memcpy(batch + 5 * 18 + 6, one, 48);
    uint64_t bout[2 * 12];
    uint8_t binf[2] = {9, 9};
    REQUIRE(zk_g1_sum_partials_batch(CURVE, batch, 3, 2, bout, binf) == ZK_OK);
    REQUIRE(!binf[0] && !binf[1] && memcmp(bout, g, 96) == 0 && memcmp(bout + 12, g, 96) == 0);
    // uncompressed / compressed round trips of the results through wire.hip
    uint8_t enc[96];
    REQUIRE(zk_g1_serialize_compressed(CURVE, two_g, 0, enc) == ZK_OK);
    REQUIRE(zk_g1_deserialize_compressed(CURVE, enc, again, &inf) == ZK_OK && !inf && memcmp(again, two_g, 96) == 0);
    return 0;
}

static std::atomic<int> g_fail{0};
#define TCHECK(cond)                                                                          \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            fprintf(stderr, "host_stress thread: %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail.fetch_add(1);                                                              \
            return;                                                                           \
        }                                                                                     \
    } while (0)

// ---- the scenario of the allocation-failure sweep (section 2d): one pass over the calls that allocate -- a ctx, an SRS and its 16-bit
// table, a blocking batch, a deferred round with an opening, the host-pointer calls behind both caches, an NTT with its plan, a circuit
// check, a lookup map and one IPA key fold -- at the sizes the sections above use.  Any one hipMalloc / hipHostMalloc of it may be the
// one fake_hip_fail_alloc_after() refuses.  What must hold whichever it is: every call returns ZK_OK or ZK_ERR_OOM and nothing else
// (a stale runtime error would come back as ZK_ERR_HIP or as a second ZK_ERR_OOM from a call that allocated nothing); at most ONE call
// of a pass fails, since the hook fires once and a ctx that has refused a call works again at the next; an open round can be aborted.
// A call that needs what a failed call did not deliver (the ctx, the SRS, a device buffer) is skipped.
struct Scenario {
    const std::vector<uint64_t>* srs_bytes;
    const std::vector<std::vector<uint64_t>>* polys;
    size_t n;
    int ooms = 0;           // calls of this pass that returned ZK_ERR_OOM
    int bad_line = 0;       // the first call that returned anything else, or a round that could not be aborted
    bool note(int rc, int line) {
        if (rc == ZK_ERR_OOM) ++ooms;
        else if (rc != ZK_OK && !bad_line) bad_line = line;
        return rc == ZK_OK;
    }
    // *pc: the ctx to use, created here when null (and left to the caller, who destroys it)
    void run(zk_ctx** pc) {
#define STEP(call) note((call), __LINE__)
        ooms = 0, bad_line = 0;
        if (!*pc && !STEP(zk_ctx_create(0, pc))) return;
        zk_ctx* c = *pc;
        zk_srs* s = nullptr;
        void* d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // four polynomials, an output vector, a lookup map
        const size_t slots = zk_lookup_map_slots(64);
        [&] {
            if (!STEP(zk_srs_register(c, CURVE, srs_bytes->data(), nullptr, n, &s))) return;
            STEP(zk_srs_precompute(c, s));             // refused: no table, the calls below take the per-window path
            for (int k = 0; k < 6; ++k)
                if (!STEP(zk_dev_alloc(c, k == 5 ? slots * 4 : n * 32, &d[k]))) return;
            for (int k = 0; k < 4; ++k)
                if (!STEP(zk_dev_upload(c, d[k], (*polys)[k].data(), n * 32))) return;
            const void* in[4] = {d[0], d[1], d[2], d[3]};
            const uint64_t* hp[4] = {(*polys)[0].data(), (*polys)[1].data(), (*polys)[2].data(), (*polys)[3].data()};
            size_t lens[4] = {n, n, n - 1, 64};
            uint64_t xy[16 * 12], z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
            uint8_t inf[16];
            STEP(zk_kzg_commit_batch_dev(c, s, 4, in, lens, xy, inf));
            // a deferred round: whatever refuses, the round can be dropped and leaves nothing pending
            const bool queued = STEP(zk_kzg_round_begin_dev(c, s, 2, in, lens, nullptr)) && STEP(zk_kzg_open_begin_dev(c, s, 3, in, lens, z, ch));
            if (!queued || !STEP(zk_kzg_round_end(c, 3, xy, inf))) {
                uint32_t pend = 9;
                if ((zk_kzg_round_abort(c) != ZK_OK || zk_kzg_round_pending(c, &pend) != ZK_OK || pend != 0) && !bad_line) bad_line = __LINE__;
            }
            // the host-pointer calls with the residency and the commitment cache on
            if (STEP(zk_ctx_set_residency_cache(c, 1, 0, 0)) && STEP(zk_ctx_set_commit_cache(c, 1, 8))) {
                STEP(zk_kzg_commit_batch(c, s, 4, hp, lens, xy, inf));
                STEP(zk_kzg_open(c, s, 3, hp, lens, z, ch, xy, inf));
            }
            STEP(zk_ctx_set_residency_cache(c, 0, 0, 0));
            STEP(zk_ctx_set_commit_cache(c, 0, 0));
            STEP(zk_ntt_prepare(c, CURVE, 13));
            STEP(zk_ntt_dev(c, CURVE, ZK_NTT_IFFT, 13, d[0], n, d[4]));
            {   // a circuit check over 2^13 rows: every column is one of the vectors above (the fake device computes nothing)
                zk_circuit_check_args a;
                memset(&a, 0, sizeof a);
                a.w_l = d[0], a.w_r = d[1], a.w_o = d[2], a.w_4 = d[3];
                a.q_m = a.q_l = a.q_r = a.q_o = a.q_4 = a.q_c = a.q_arith = a.q_range = a.q_logic = a.q_fixed_group_add = a.q_variable_group_add = a.q_lookup = d[0];
                for (int k = 0; k < 4; ++k) a.sigma[k] = d[k], a.table[k] = d[k];
                a.table_rows = 64;
                zk_circuit_check_summary sum;
                STEP(zk_circuit_check_dev(c, CURVE, 13, &a, nullptr, &sum));
            }
            {   // a lookup map over the first 64 rows and 64 queries of it
                const void* ops[3] = {d[0], d[1], d[3]};
                uint64_t misses = 0, first = 0;
                if (STEP(zk_lookup_map_build_dev(c, CURVE, d[0], d[1], d[3], 64, d[5], slots)))
                    STEP(zk_lookup_map_query_dev(c, CURVE, in, 64, d[5], slots, 64, ops, nullptr, 64, d[4], nullptr, 64, nullptr, &misses, &first));
            }
            STEP(zk_ipa_fold_key_dev(c, CURVE, 64, d[0], nullptr, z, d[4], nullptr));      // 128 key points in, 64 out
        }();
        for (int k = 0; k < 6; ++k)
            if (d[k]) STEP(zk_dev_free(c, d[k]));
        if (s) zk_srs_free(s);
#undef STEP
    }
};

int main() {
    REQUIRE(real_point_arithmetic() == 0);

    const size_t n = 1 << 13;           // the smallest size that takes the window-table path (ZK_PRE_MIN_N)
    std::vector<uint64_t> srs_a(n * 2 * L), srs_b(n * 2 * L);
    for (size_t i = 0; i < srs_a.size(); ++i) {
        srs_a[i] = 0x1000 + i;          // bytes only: the fake device never looks at them, the registry digests them
        srs_b[i] = 0x9000 + 3 * i;
    }
    std::vector<std::vector<uint64_t>> polys(4, std::vector<uint64_t>(n * 4));
    for (size_t k = 0; k < polys.size(); ++k)
        for (size_t i = 0; i < polys[k].size(); ++i) polys[k][i] = (k + 1) * 1000003ull + i;

    // ---- 1. several threads register the same and different SRS bytes at once, precompute, commit through ONE shared ctx
    zk_ctx* shared = nullptr;
    REQUIRE(zk_ctx_create(0, &shared) == ZK_OK);
    {
        std::vector<std::thread> th;
        for (int t = 0; t < 6; ++t)
            th.emplace_back([&, t] {
                for (int it = 0; it < 8; ++it) {
                    zk_srs* s = nullptr;
                    TCHECK(zk_srs_register(shared, CURVE, (t & 1) ? srs_b.data() : srs_a.data(), nullptr, n, &s) == ZK_OK && s);
                    TCHECK(zk_srs_len(s) == n);
                    TCHECK(zk_srs_precompute(shared, s) == ZK_OK);
                    uint32_t c = 0, w = 0;
                    TCHECK(zk_srs_table_info(s, &c, &w) == ZK_OK && c == 16 && w == 16);
                    uint64_t xy[4 * 12];
                    uint8_t inf[4] = {0, 0, 0, 0};
                    const uint64_t* ptrs[4] = {polys[0].data(), polys[1].data(), polys[2].data(), polys[3].data()};
                    size_t lens[4] = {n, n - 1, n, 100};          // table path and a short vector (per-window path)
                    TCHECK(zk_kzg_commit_batch(shared, s, 4, ptrs, lens, xy, inf) == ZK_OK);
                    TCHECK(inf[0] && inf[1] && inf[2] && inf[3]);      // all-zero device results: the point at infinity
                    uint64_t z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
                    TCHECK(zk_kzg_open(shared, s, 3, ptrs, lens, z, ch, xy, inf) == ZK_OK);
                    std::vector<uint64_t> v(polys[t % 4]);
                    TCHECK(zk_ntt(shared, CURVE, ZK_NTT_IFFT, 13, v.data(), n, v.data()) == ZK_OK);
                    if (it & 1) TCHECK(zk_srs_retain(s) == ZK_OK);
                    zk_srs_free(s);
                    if (it & 1) zk_srs_free(s);
                }
            });
        for (auto& t : th) t.join();
        REQUIRE(g_fail.load() == 0);
        uint64_t hits = 0, misses = 0, entries = 0, bytes = 0;
        REQUIRE(zk_srs_cache_stats(&hits, &misses, &entries, &bytes) == ZK_OK);
        REQUIRE(misses == 2 && hits == 6 * 8 - 2 && entries == 2);
    }

    // ---- 2. a ctx per thread over ONE SRS: deferred rounds, the refusals while a round is open, abort, the commitment cache
    zk_srs* srs = nullptr;
    REQUIRE(zk_srs_register(shared, CURVE, srs_a.data(), nullptr, n, &srs) == ZK_OK);
    {
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t] {
                zk_ctx* c = nullptr;
                TCHECK(zk_ctx_create(0, &c) == ZK_OK);
                std::vector<void*> d(4, nullptr);
                for (int k = 0; k < 4; ++k) {
                    TCHECK(zk_dev_alloc(c, n * 32, &d[k]) == ZK_OK);
                    TCHECK(zk_dev_upload(c, d[k], polys[k].data(), n * 32) == ZK_OK);
                }
                const void* in[4] = {d[0], d[1], d[2], d[3]};
                size_t lens[4] = {n, n, n - 1, 64};
                uint64_t xy[16 * 12];
                uint8_t inf[16];
                uint64_t z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
                for (int it = 0; it < 10; ++it) {
                    TCHECK(zk_kzg_round_begin_dev(c, srs, 2, in, lens, nullptr) == ZK_OK);
                    TCHECK(zk_kzg_round_begin_dev(c, srs, 2, in + 2, lens + 2, nullptr) == ZK_OK);      // a short vector joins the round
                    TCHECK(zk_kzg_open_begin_dev(c, srs, 3, in, lens, z, ch) == ZK_OK);
                    uint32_t pend = 0;
                    TCHECK(zk_kzg_round_pending(c, &pend) == ZK_OK && pend == 5);
                    TCHECK(zk_kzg_commit_dev(c, srs, d[0], n, xy, inf) == ZK_ERR_PENDING);               // blocking calls refuse
                    TCHECK(zk_kzg_round_end(c, 4, xy, inf) == ZK_ERR_BAD_ARG);                           // wrong count: stays open
                    if (it % 3 == 2) {
                        TCHECK(zk_kzg_round_abort(c) == ZK_OK);
                    } else {
                        if (it & 1) TCHECK(zk_kzg_round_reduce(c) == ZK_OK);
                        if (it & 1) TCHECK(zk_kzg_round_begin_dev(c, srs, 1, in, lens, nullptr) == ZK_ERR_PENDING);   // closed to new jobs
                        TCHECK(zk_kzg_round_end(c, 5, xy, inf) == ZK_OK);
                    }
                    TCHECK(zk_kzg_round_pending(c, &pend) == ZK_OK && pend == 0);
                    // the device form of a round's result: 2 VW sums per job on the device, summed over the ranks, combined by the host pool
                    {
                        const size_t wb = zk_winsums_dev_bytes(c, srs), pb = 256;
                        uint32_t geom[4] = {0, 0, 0, 0};
                        TCHECK(wb == 2 * 64 * pb && zk_winsums_geometry(c, srs, geom) == ZK_OK && geom[0] == 16 && geom[2] == 64);
                        void* ws = nullptr;
                        TCHECK(zk_dev_alloc(c, 2 * 4 * wb, &ws) == ZK_OK);
                        TCHECK(zk_kzg_round_begin_dev(c, srs, 4, in, lens, nullptr) == ZK_OK);
                        TCHECK(zk_kzg_round_reduce_winsums_dev(c, ws) == ZK_OK);
                        TCHECK(zk_kzg_round_end(c, 4, xy, inf) == ZK_ERR_PENDING);                // reduced towards the device: the host form refuses
                        TCHECK(zk_kzg_round_end_winsums_dev(c, 4, (char*)ws + 64) == ZK_ERR_PENDING);   // ... and so does another buffer
                        TCHECK(zk_kzg_round_end_winsums_dev(c, 4, ws) == ZK_OK);
                        TCHECK(zk_g1_sum_winsums_dev(c, srs, ws, 2, 4, xy, inf) == ZK_OK && inf[0] && inf[3]);
                        TCHECK(zk_dev_free(c, ws) == ZK_OK);
                    }
                    // tuning options: per ctx, refused while a round is open, toggled here between rounds while a second thread of the
                    // SAME ctx reads them (the ctx lock orders the two; getenv / setenv would have raced)
                    {
                        std::thread reader([&] {
                            for (int r = 0; r < 50; ++r) {
                                int64_t v = -7;
                                TCHECK(zk_ctx_get_option(c, "msm_merge", &v) == ZK_OK && (v == 0 || v == 1));
                                TCHECK(zk_ctx_get_option(c, "pre_vw", &v) == ZK_OK && (v == 0 || v == 32));
                            }
                        });
                        TCHECK(zk_ctx_set_option(c, "msm_merge", it & 1) == ZK_OK);
                        TCHECK(zk_ctx_set_option(c, "pre_vw", (it & 2) ? 32 : 0) == ZK_OK);
                        TCHECK(zk_ctx_set_option(c, "no_such_key", 1) == ZK_ERR_UNSUPPORTED && zk_ctx_set_option(c, "pre_vw", 48) == ZK_ERR_BAD_ARG);
                        TCHECK(zk_kzg_round_begin_dev(c, srs, 2, in, lens, nullptr) == ZK_OK);
                        TCHECK(zk_ctx_set_option(c, "chunk_l", 64) == ZK_ERR_PENDING);
                        TCHECK(zk_kzg_round_end(c, 2, xy, inf) == ZK_OK);
                        reader.join();
                        TCHECK(zk_ctx_set_option(c, "msm_merge", 1) == ZK_OK && zk_ctx_set_option(c, "pre_vw", 0) == ZK_OK);
                    }
                    // the residency cache of the host-pointer calls: outputs kept, inputs digested and found again, a cache of two
                    // vectors evicting under a batch of four, off = everything returned
                    {
                        const uint64_t* hp[4] = {polys[0].data(), polys[1].data(), polys[2].data(), polys[3].data()};
                        size_t hl[4] = {n, n, n - 1, 64};
                        TCHECK(zk_ctx_set_residency_cache(c, 1, (it & 1) ? 2 * n * 32 : 0, 0) == ZK_OK);
                        std::vector<uint64_t> v(polys[t % 4]);
                        TCHECK(zk_ntt(c, CURVE, ZK_NTT_IFFT, 13, v.data(), n, v.data()) == ZK_OK);          // in place: digested before it is overwritten
                        TCHECK(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
                        TCHECK(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
                        TCHECK(zk_kzg_open(c, srs, 3, hp, hl, z, ch, xy, inf) == ZK_OK);
                        uint64_t rh = 0, rm = 0, re = 0, rb = 0;
                        TCHECK(zk_residency_cache_stats(c, &rh, &rm, &re, &rb) == ZK_OK && rh >= 3 && re >= 1 && rb <= ((it & 1) ? 2 * n * 32 : ((size_t)2 << 30)));
                        TCHECK(zk_kzg_round_begin_dev(c, srs, 1, in, lens, nullptr) == ZK_OK);
                        TCHECK(zk_ctx_set_residency_cache(c, 0, 0, 0) == ZK_ERR_PENDING);
                        TCHECK(zk_kzg_round_abort(c) == ZK_OK);
                        TCHECK(zk_ctx_set_residency_cache(c, 0, 0, 0) == ZK_OK);
                        TCHECK(zk_residency_cache_stats(c, nullptr, nullptr, &re, &rb) == ZK_OK && re == 0 && rb == 0);
                    }
                    // the commitment cache: second batch is all hits
                    TCHECK(zk_ctx_set_commit_cache(c, 1, 8) == ZK_OK);
                    TCHECK(zk_kzg_commit_batch_dev(c, srs, 4, in, lens, xy, inf) == ZK_OK);
                    TCHECK(zk_kzg_commit_batch_dev(c, srs, 4, in, lens, xy, inf) == ZK_OK);
                    uint64_t h = 0, m = 0, e = 0;
                    TCHECK(zk_commit_cache_stats(c, &h, &m, &e) == ZK_OK && h >= 4 && e >= 1);
                    TCHECK(zk_ctx_set_commit_cache(c, 0, 0) == ZK_OK);
                }
                for (int k = 0; k < 4; ++k) TCHECK(zk_dev_free(c, d[k]) == ZK_OK);
                zk_ctx_destroy(c);
            });
        for (auto& t : th) t.join();
        REQUIRE(g_fail.load() == 0);
    }

    // ---- 2b. the memory budget of the deferred rounds (round 6): a begin that finds no room for another job's buffer set closes the
    // queued jobs early and reuses their sets; the option's soft limit, a "device" that really runs out (hipMalloc failing), and a
    // device too small for even one set (ZK_ERR_OOM, the ctx usable afterwards)
    {
        std::vector<void*> d(4, nullptr);
        zk_ctx* c = nullptr;
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        for (int k = 0; k < 4; ++k) {
            REQUIRE(zk_dev_alloc(c, n * 32, &d[k]) == ZK_OK);
            REQUIRE(zk_dev_upload(c, d[k], polys[k].data(), n * 32) == ZK_OK);
        }
        const void* in[8] = {d[0], d[1], d[2], d[3], d[0], d[1], d[2], d[3]};
        size_t lens[8] = {n, n, n - 1, 64, n, n - 2, n, n};
        uint64_t xy[16 * 12], z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
        uint8_t inf[16];
        uint64_t closes = 0, set_bytes = 0, fr = 0, tot = 0;
        REQUIRE(zk_ctx_set_option(c, "round_mem_limit_mb", 40) == ZK_OK && zk_ctx_set_option(c, "mem_reserve_mb", 0) == ZK_OK);
        for (int it = 0; it < 3; ++it) {
            REQUIRE(zk_kzg_round_begin_dev(c, srs, 8, in, lens, nullptr) == ZK_OK);
            REQUIRE(zk_kzg_open_begin_dev(c, srs, 3, in, lens, z, ch) == ZK_OK);
            REQUIRE(zk_kzg_round_begin_dev(c, srs, 4, in, lens, nullptr) == ZK_OK);
            if (it == 1) REQUIRE(zk_kzg_round_reduce(c) == ZK_OK);
            REQUIRE(zk_kzg_round_end(c, 13, xy, inf) == ZK_OK && inf[0] && inf[12]);
        }
        REQUIRE(zk_round_mem_stats(c, &closes, &set_bytes, &fr, &tot) == ZK_OK && closes >= 3 && set_bytes < ((size_t)110 << 20) && tot > fr);     // two table-path sets of 19 MB (nine without the
                                                                                          // budget); n - 1, n - 2 and 64 are per-window jobs
        REQUIRE(zk_kzg_commit_batch_dev(c, srs, 8, in, lens, xy, inf) == ZK_OK && inf[7]);       // the blocking batch in pieces
        REQUIRE(zk_ctx_set_option(c, "round_mem_limit_mb", 0) == ZK_OK);
        zk_ctx_destroy(c);
        // a device with room for about three sets beyond what is live: hipMemGetInfo says so first, hipMalloc itself when the reserve hides it
        for (int lie = 0; lie < 2; ++lie) {
            REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
            REQUIRE(zk_ctx_set_option(c, "mem_reserve_mb", 0) == ZK_OK);
            fake_hip_set_memory(fake_hip_live_bytes() + ((size_t)56 << 20), lie ? (size_t)1 << 30 : 0);
            REQUIRE(zk_kzg_round_begin_dev(c, srs, 8, in, lens, nullptr) == ZK_OK);
            REQUIRE(zk_kzg_open_begin_dev(c, srs, 3, in, lens, z, ch) == ZK_OK);
            REQUIRE(zk_kzg_round_end(c, 9, xy, inf) == ZK_OK && inf[8]);
            REQUIRE(zk_round_mem_stats(c, &closes, nullptr, &fr, nullptr) == ZK_OK && closes >= 1 && (lie || fr < ((size_t)56 << 20)));
            // too small for a single set: ZK_ERR_OOM, nothing queued, the round can be dropped and the ctx works again with memory back
            fake_hip_set_memory(fake_hip_live_bytes() + ((size_t)1 << 20), 0);
            zk_ctx* c2 = nullptr;
            REQUIRE(zk_ctx_create(0, &c2) == ZK_OK);
            REQUIRE(zk_kzg_round_begin_dev(c2, srs, 2, in, lens, nullptr) == ZK_ERR_OOM);
            REQUIRE(zk_kzg_round_abort(c2) == ZK_OK);
            REQUIRE(zk_kzg_commit_batch_dev(c2, srs, 2, in, lens, xy, inf) == ZK_ERR_OOM);
            fake_hip_set_memory(0, 0);
            REQUIRE(zk_kzg_commit_batch_dev(c2, srs, 2, in, lens, xy, inf) == ZK_OK && inf[1]);
            zk_ctx_destroy(c2);
            zk_ctx_destroy(c);
        }
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        for (int k = 0; k < 4; ++k) REQUIRE(zk_dev_free(c, d[k]) == ZK_OK);
        zk_ctx_destroy(c);
    }

    // ---- 2c. the caches' error paths and guarantees (round 6)
    {
        zk_ctx* c = nullptr;
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        const uint64_t* hp[4] = {polys[0].data(), polys[1].data(), polys[2].data(), polys[3].data()};
        size_t hl[4] = {n, n, n - 1, 64};
        uint64_t xy[16 * 12], z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
        uint8_t inf[16];
        uint64_t h0 = 0, m0 = 0, e0 = 0, b0 = 0, h1 = 0, m1 = 0, e1 = 0, b1 = 0;
        REQUIRE(zk_ctx_set_residency_cache(c, 1, 0, 0) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(c, srs, 2, hp, hl, xy, inf) == ZK_OK);                 // two vectors resident
        REQUIRE(zk_residency_cache_stats(c, &h0, &m0, &e0, &b0) == ZK_OK && e0 == 2);
        // a call that fails AFTER it has created entries (a staging buffer of a later polynomial finds no memory): the entries it made or
        // touched are gone -- their digests would name bytes that never arrived -- and the same call succeeds once memory is back
        fake_hip_set_memory(fake_hip_live_bytes() + 4096, 0);
        REQUIRE(zk_kzg_open(c, srs, 4, hp, hl, z, ch, xy, inf) == ZK_ERR_OOM);
        REQUIRE(zk_residency_cache_stats(c, &h1, &m1, &e1, &b1) == ZK_OK && e1 <= e0 && b1 <= b0);
        REQUIRE(zk_ctx_set_commit_cache(c, 1, 8) == ZK_OK);
        zk_ctx* cfresh = nullptr;                                                       // no staging buffers yet: its first upload fails
        REQUIRE(zk_ctx_create(0, &cfresh) == ZK_OK);
        REQUIRE(zk_ctx_set_residency_cache(cfresh, 1, 0, 0) == ZK_OK && zk_ctx_set_commit_cache(cfresh, 1, 8) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(cfresh, srs, 4, hp, hl, xy, inf) == ZK_ERR_OOM);
        REQUIRE(zk_residency_cache_stats(cfresh, nullptr, nullptr, &e1, &b1) == ZK_OK && e1 == 0 && b1 == 0);
        fake_hip_set_memory(0, 0);
        REQUIRE(zk_kzg_commit_batch(cfresh, srs, 4, hp, hl, xy, inf) == ZK_OK && inf[0] && inf[3]);
        REQUIRE(zk_kzg_open(c, srs, 4, hp, hl, z, ch, xy, inf) == ZK_OK);
        zk_ctx_destroy(cfresh);
        // cache_verify: every hit is checked against the real thing; nothing may be found wrong
        uint64_t checked = 0, wrong = 9;
        REQUIRE(zk_ctx_set_option(c, "cache_verify", 1) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
        REQUIRE(zk_kzg_open(c, srs, 3, hp, hl, z, ch, xy, inf) == ZK_OK);
        REQUIRE(zk_cache_verify_stats(c, &checked, &wrong) == ZK_OK && checked >= 6 && wrong == 0);
        REQUIRE(zk_ctx_set_option(c, "cache_verify", 0) == ZK_OK && zk_ctx_set_option(c, "cache_verify", 2) == ZK_ERR_BAD_ARG);
        zk_ctx_destroy(c);
        // no operating-system entropy behind the digest key: the caches whose hits replace a computation refuse to switch on, and the
        // SRS registry shares nothing
        zk_process_key_reset_for_tests("/nonexistent/entropy");
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        REQUIRE(zk_ctx_set_commit_cache(c, 1, 8) == ZK_ERR_UNSUPPORTED && zk_ctx_set_residency_cache(c, 1, 0, 0) == ZK_ERR_UNSUPPORTED);
        REQUIRE(zk_ctx_set_commit_cache(c, 0, 0) == ZK_OK && zk_ctx_set_residency_cache(c, 0, 0, 0) == ZK_OK);
        zk_srs *s1 = nullptr, *s2 = nullptr;
        REQUIRE(zk_srs_register(c, CURVE, srs_a.data(), nullptr, n, &s1) == ZK_OK && zk_srs_register(c, CURVE, srs_a.data(), nullptr, n, &s2) == ZK_OK);
        REQUIRE(s1 != s2 && s1 != srs);
        REQUIRE(zk_kzg_commit_batch(c, s1, 2, hp, hl, xy, inf) == ZK_OK);
        zk_srs_free(s1);
        zk_srs_free(s2);
        zk_ctx_destroy(c);
        zk_process_key_reset_for_tests(nullptr);
    }

    // ---- 2d. the allocation-failure sweep: the scenario above with its k-th allocation refused, for every k it has
    {
        std::vector<uint64_t> srs_c(n * 2 * L);
        for (size_t i = 0; i < srs_c.size(); ++i) srs_c[i] = 0x5000 + 7 * i;      // bytes no other section registers
        REQUIRE(zk_srs_cache_config(0) == ZK_OK && zk_srs_cache_config((size_t)32 << 30) == ZK_OK);      // idle entries of the sections above
        const auto t0 = std::chrono::steady_clock::now();
        const long live0 = fake_hip_live_allocations(), far = 1l << 40;
        Scenario sc{&srs_c, &polys, n};
        // one pass of the scenario on *pc (created when null), then the ctx destroyed and the SRS evicted: nothing of the pass is left
        auto pass = [&](zk_ctx** pc, bool keep_ctx) {
            sc.run(pc);
            if (!keep_ctx && *pc) {
                zk_ctx_destroy(*pc);
                *pc = nullptr;
            }
            return zk_srs_cache_config(0) == ZK_OK && zk_srs_cache_config((size_t)32 << 30) == ZK_OK && sc.bad_line == 0;
        };
        zk_ctx* c = nullptr;
        fake_hip_fail_alloc_after(far);                              // counts, never fires
        REQUIRE(pass(&c, false) && sc.ooms == 0);
        const long counted = far - fake_hip_fail_alloc_after(-1);
        REQUIRE(counted > 20 && fake_hip_live_allocations() == live0);
        long swept = 0;
        for (long k = 0;; ++k) {
            fake_hip_fail_alloc_after(k);
            const bool ok = pass(&c, true);
            const bool fired = fake_hip_fail_alloc_after(-1) < 0;
            if (!ok || sc.ooms > 1 || (!fired && sc.ooms)) {
                fprintf(stderr, "host_stress: allocation %ld refused: host_stress.cpp:%d returned neither ZK_OK nor ZK_ERR_OOM, or %d calls failed\n", k,
                        sc.bad_line, sc.ooms);
                return 1;
            }
            if (fired) {
                ++swept;
                if (c) REQUIRE(pass(&c, false) && sc.ooms == 0);      // the ctx that met the refusal: everything works
            } else if (c) {
                zk_ctx_destroy(c);
                c = nullptr;
            }
            REQUIRE(fake_hip_live_allocations() == live0);
            if (!fired) break;                                        // the scenario has no k-th allocation: every one was refused once
            REQUIRE(pass(&c, false) && sc.ooms == 0);                 // ... and so does a fresh one
            REQUIRE(fake_hip_live_allocations() == live0);
        }
        REQUIRE(swept >= counted);                                    // a scenario that shrank under injection would pass with fewer
        printf("host_stress: allocation sweep: %ld allocation sites refused one by one (%ld counted without injection), %.1f s\n", swept, counted,
               std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }

    // ---- 2e. cache_verify meets a wrong hit: the resident copy of a vector no longer holds what its digest names
    {
        zk_ctx* c = nullptr;
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        REQUIRE(zk_ctx_set_residency_cache(c, 1, 0, 0) == ZK_OK && zk_ctx_set_option(c, "cache_verify", 1) == ZK_OK);
        const size_t m = n - 5, bytes = m * 32;                       // a length no other vector of the program has
        const size_t alloc = bytes + bytes / 8 + 256;                 // what a device buffer of `bytes` allocates (DevBuf::want_for, csrc/ctx.h)
        const uint64_t* hp[3] = {polys[3].data(), polys[3].data(), polys[0].data()};
        size_t hl[3] = {m, m, n};
        uint64_t xy[3 * 12];
        uint8_t inf[3];
        REQUIRE(zk_kzg_commit_batch(c, srs, 3, hp, hl, xy, inf) == ZK_OK);              // both vectors resident
        uint64_t h0 = 0, m0 = 0, e0 = 0, b0 = 0, h1 = 0, m1 = 0, e1 = 0, b1 = 0, chk0 = 0, bad0 = 9, chk1 = 0, bad1 = 9;
        REQUIRE(zk_residency_cache_stats(c, &h0, &m0, &e0, &b0) == ZK_OK && e0 == 2 && b0 == bytes + n * 32);
        REQUIRE(zk_cache_verify_stats(c, &chk0, &bad0) == ZK_OK && bad0 == 0);
        const long live = fake_hip_live_allocations();
        REQUIRE(fake_hip_flip_byte(alloc) >= 1);                      // the device copy (and the ctx's scratch buffers of that length, which
                                                                      // nothing reads on the fake device): the one mismatch below is the proof
        // the vector twice in one batch, and the other one: the first finds the entry wrong and replaces it, the second uses the replacement
        REQUIRE(zk_kzg_commit_batch(c, srs, 3, hp, hl, xy, inf) == ZK_OK && inf[0] && inf[2]);
        REQUIRE(zk_cache_verify_stats(c, &chk1, &bad1) == ZK_OK && bad1 == bad0 + 1 && chk1 == chk0 + 2);
        REQUIRE(zk_residency_cache_stats(c, &h1, &m1, &e1, &b1) == ZK_OK && e1 == e0 && b1 == b0 && h1 == h0 + 2 && m1 == m0 + 1);
        REQUIRE(fake_hip_live_allocations() == live);                 // the dropped entry's buffer took the upload
        REQUIRE(zk_kzg_commit_batch(c, srs, 3, hp, hl, xy, inf) == ZK_OK);              // again: three hits, all checked, nothing wrong
        REQUIRE(zk_cache_verify_stats(c, &chk0, &bad0) == ZK_OK && bad0 == bad1 && chk0 == chk1 + 3);
        REQUIRE(zk_residency_cache_stats(c, &h0, &m0, &e0, &b0) == ZK_OK && e0 == e1 && b0 == b1 && h0 == h1 + 3 && m0 == m1);
        zk_ctx_destroy(c);
    }

    // ---- 3. eviction: drop every unreferenced entry, then the last references
    zk_srs_free(srs);
    REQUIRE(zk_srs_cache_config(0) == ZK_OK);
    uint64_t entries = 99;
    REQUIRE(zk_srs_cache_stats(nullptr, nullptr, &entries, nullptr) == ZK_OK && entries == 0);
    REQUIRE(zk_srs_cache_config((size_t)32 << 30) == ZK_OK);
    zk_ctx_destroy(shared);
    REQUIRE(fake_hip_launches() > 1000);
    REQUIRE(fake_hip_live_allocations() == 0);        // every device / pinned buffer of every ctx and SRS was returned
    printf("host_stress ok: %ld kernel launches (no-ops), all device memory returned\n", fake_hip_launches());
    return 0;
}
