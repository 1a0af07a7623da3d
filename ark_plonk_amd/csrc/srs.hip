// The SRS registry: device-scoped, refcounted, content-addressed (zk_srs, ctx.h) and the zk_srs_* entry points.
#include "api_internal.h"

// (PC::trim runs on every gen_proof, circuit.rs:276, so a second registration of the same powers_of_g must cost
// a lookup, not a 96 MiB upload + table build)
static std::mutex g_srs_mu;
static std::list<zk_srs*> g_srs_cache;            // cached entries, most recently used first
static std::atomic<uint64_t> g_srs_next_id{1};
static size_t g_srs_idle_limit = (size_t)32 << 30;   // bytes of UNREFERENCED cached SRS (incl. window tables) kept resident
static uint64_t g_srs_hits = 0, g_srs_misses = 0;

static size_t srs_bytes(const zk_srs* s) { return s->n * s->point_bytes * (s->d_pre ? 1 + s->pre_rows : s->pre_W ? s->pre_W : 1); }

static void srs_destroy(zk_srs* s) {
    if (s->d_xy) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        if (prev != s->device) (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();     // kernels of any ctx may still read the bases
        (void)hipFree(s->d_xy);
        if (s->d_pre) (void)hipFree(s->d_pre);
        if (prev >= 0 && prev != s->device) (void)hipSetDevice(prev);
    }
    delete s;
}

// g_srs_mu held: drop least recently used unreferenced entries beyond the idle limit
static void srs_evict_locked() {
    size_t idle = 0;
    for (zk_srs* s : g_srs_cache)
        if (s->refs.load() == 0) idle += srs_bytes(s);
    for (auto it = g_srs_cache.end(); idle > g_srs_idle_limit && it != g_srs_cache.begin();) {
        --it;
        zk_srs* s = *it;
        if (s->refs.load() != 0) continue;
        idle -= srs_bytes(s);
        it = g_srs_cache.erase(it);
        srs_destroy(s);
    }
}

// shared tail of the registration entry points: d_sat = arkworks-layout points on the device
static int srs_build(zk_ctx* c, int curve_id, const void* d_sat, const uint8_t* d_inf, size_t n, zk_srs** out) {
    zk_srs* s = new zk_srs();
    s->device = c->device;
    s->id = g_srs_next_id.fetch_add(1);
    s->curve = curve_id;
    s->n = n;
    s->point_bytes = msm_ops(curve_id)->point_bytes();
    if (n) {
        if (hipMalloc(&s->d_xy, n * s->point_bytes) != hipSuccess) {
            delete s;
            return zk_alloc_refused();
        }
        int rc = msm_ops(curve_id)->convert_bases(c, d_sat, d_inf, n, s->d_xy);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (rc || e != hipSuccess) {
            (void)hipFree(s->d_xy);
            delete s;
            return rc ? rc : ZK_ERR_HIP;
        }
    }
    *out = s;
    return ZK_OK;
}

int srs_register_host(zk_ctx* c, int curve_id, const uint64_t* bases_xy, const uint8_t* inf_flags, size_t n, zk_srs** out, bool use_cache) {
    int L = fq_limbs64(curve_id);
    if (!L) return ZK_ERR_BAD_ARG;
    Guard g(c);
    const size_t bytes = n * 2 * L * 8;
    uint64_t dig[4] = {0, 0, 0, 0};
    std::unique_lock<std::mutex> reg(g_srs_mu, std::defer_lock);
    if (!c->key_from_os) use_cache = false;      // no OS entropy behind the digest key: every registration builds its own copy
    if (use_cache) {
        host_digest256(bases_xy, bytes, 0x5125ull ^ ((uint64_t)curve_id << 32) ^ (uint64_t)n, dig);
        if (inf_flags) {
            uint64_t d2[4];
            host_digest256(inf_flags, n, 0xF1A65ull, d2);
            bool any = false;
            for (size_t i = 0; i < n && !any; ++i) any = inf_flags[i] != 0;
            if (any)   // an all-zero flag array is the same SRS as no flag array
                for (int k = 0; k < 4; ++k) dig[k] ^= d2[k];
        }
        reg.lock();   // held across the build: two threads registering the same SRS build it once
        for (auto it = g_srs_cache.begin(); it != g_srs_cache.end(); ++it) {
            zk_srs* s = *it;
            if (s->device == c->device && s->curve == curve_id && s->n == n && !memcmp(s->digest, dig, sizeof dig)) {
                s->refs.fetch_add(1);
                g_srs_cache.splice(g_srs_cache.begin(), g_srs_cache, it);
                ++g_srs_hits;
                *out = s;
                return ZK_OK;
            }
        }
        ++g_srs_misses;
    }
    int rc = c->io.b.ensure(bytes ? bytes : 1);
    if (rc) return rc;
    const uint8_t* d_inf = nullptr;
    if (n) {
        if ((rc = zk_h2d(c, c->io.b.p, bases_xy, bytes, c->stream))) return rc;
        if (inf_flags) {
            rc = c->msm_tmp.ensure(n);
            if (rc) return rc;
            if ((rc = zk_h2d(c, c->msm_tmp.p, inf_flags, n, c->stream))) return rc;
            d_inf = (const uint8_t*)c->msm_tmp.p;
        }
    }
    zk_srs* s = nullptr;
    rc = srs_build(c, curve_id, c->io.b.p, d_inf, n, &s);
    if (rc) return rc;
    if (use_cache) {
        s->cached = true;
        memcpy(s->digest, dig, sizeof dig);
        g_srs_cache.push_front(s);
        srs_evict_locked();
    }
    *out = s;
    return ZK_OK;
}

extern "C" {

int zk_srs_register_dev(zk_ctx* c, int curve_id, const void* d_bases_xy, const uint8_t* d_inf_flags, size_t n, zk_srs** out) {
    if (!c || !out || (n && !d_bases_xy)) return ZK_ERR_BAD_ARG;
    if (!zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return srs_build(c, curve_id, d_bases_xy, d_inf_flags, n, out);
}

int zk_srs_register(zk_ctx* c, int curve_id, const uint64_t* bases_xy, const uint8_t* inf_flags, size_t n, zk_srs** out) {
    if (!c || !out || (n && !bases_xy)) return ZK_ERR_BAD_ARG;
    return srs_register_host(c, curve_id, bases_xy, inf_flags, n, out, n != 0);
}

int zk_srs_precompute_rows(zk_ctx* c, zk_srs* s, uint32_t window_bits, uint32_t first_window, uint32_t window_stride) {
    if (!c || !s || s->device != c->device) return ZK_ERR_BAD_ARG;
    if (window_bits != 0 && (window_bits < 16 || window_bits > 21)) return ZK_ERR_BAD_ARG;
    if (window_stride == 0 || first_window >= window_stride) return ZK_ERR_BAD_ARG;
    Guard g(c);
    std::unique_lock<std::shared_mutex> wl(s->mu);   // no MSM of any ctx is reading or enqueueing on this SRS
    if (s->n == 0) return ZK_OK;
    if (s->pre_W)                                    // one table per SRS: the first precompute wins
        return ((window_bits == 0 || window_bits == s->pre_c) && first_window == s->pre_w0 && window_stride == s->pre_wstep) ? ZK_OK : ZK_ERR_UNSUPPORTED;
    ZK_HIP_TRY(hipDeviceSynchronize());               // ... and none it enqueued earlier is still running
    return msm_ops(s->curve)->precompute(c, s, window_bits, first_window, window_stride);
}

int zk_srs_precompute_ex(zk_ctx* c, zk_srs* s, uint32_t window_bits) { return zk_srs_precompute_rows(c, s, window_bits, 0, 1); }

int zk_srs_table_rows(zk_srs* s, uint32_t* first_window, uint32_t* window_stride, uint32_t* rows) {
    if (!s) return ZK_ERR_BAD_ARG;
    SrsRead rl(s->mu);
    if (first_window) *first_window = s->pre_w0;
    if (window_stride) *window_stride = s->pre_wstep;
    if (rows) *rows = s->pre_rows;
    return ZK_OK;
}

int zk_srs_precompute(zk_ctx* c, zk_srs* s) { return zk_srs_precompute_ex(c, s, 0); }

int zk_srs_table_info(zk_srs* s, uint32_t* window_bits, uint32_t* windows) {
    if (!s) return ZK_ERR_BAD_ARG;
    SrsRead rl(s->mu);
    if (window_bits) *window_bits = s->pre_c;
    if (windows) *windows = s->pre_W;
    return ZK_OK;
}

int zk_srs_retain(zk_srs* s) {
    if (!s) return ZK_ERR_BAD_ARG;
    std::lock_guard<std::mutex> reg(g_srs_mu);
    if (s->refs.load() <= 0) return ZK_ERR_BAD_ARG;     // only a live handle can be shared
    s->refs.fetch_add(1);
    return ZK_OK;
}

void zk_srs_free(zk_srs* s) {
    if (!s) return;
    std::lock_guard<std::mutex> reg(g_srs_mu);
    const int left = s->refs.fetch_sub(1) - 1;
    if (left > 0) return;
    if (!s->cached) {
        srs_destroy(s);
        return;
    }
    srs_evict_locked();    // stays resident for the next PC::trim unless the idle budget is exceeded
}

size_t zk_srs_len(const zk_srs* s) { return s ? s->n : 0; }

int zk_srs_cache_config(size_t max_idle_bytes) {
    std::lock_guard<std::mutex> reg(g_srs_mu);
    g_srs_idle_limit = max_idle_bytes;
    srs_evict_locked();
    return ZK_OK;
}

int zk_srs_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* resident_bytes) {
    std::lock_guard<std::mutex> reg(g_srs_mu);
    if (hits) *hits = g_srs_hits;
    if (misses) *misses = g_srs_misses;
    if (entries) *entries = g_srs_cache.size();
    if (resident_bytes) {
        uint64_t b = 0;
        for (zk_srs* s : g_srs_cache) b += srs_bytes(s);
        *resident_bytes = b;
    }
    return ZK_OK;
}

}  // extern "C"
