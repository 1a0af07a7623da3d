// C ABI (include/ark_plonk_amd.h), unit 1 of 7: error text, profiling, the process-wide host pool, ctx lifetime / stream / options,
// the statistics getters of the host I/O and the plain device-memory utilities.  The other units: residency.hip, srs.hip, commit.hip,
// round.hip, api_host.hip, api_poly.hip; what they share is declared in api_internal.h.
#include "api_internal.h"

#include <cstdio>

static thread_local char g_last_hip[256];

void zk_note_hip_error(hipError_t e, const char* what, const char* file, int line) {
    snprintf(g_last_hip, sizeof g_last_hip, "%s (%s) at %s:%d", hipGetErrorString(e), what, file, line);
    if (getenv("ZK_VERBOSE")) fprintf(stderr, "[ark_plonk_amd] HIP error: %s\n", g_last_hip);
}

// ------------------------------------------------------------------------------------- profiling
ProfScope::ProfScope(zk_ctx* ctx, const char* nm) : ProfScope(ctx, nm, ctx->stream) {}
ProfScope::ProfScope(zk_ctx* ctx, const char* nm, hipStream_t stream) : c(ctx), name(nm), st(stream) {
    if (!c->profiling) return;
    if (c->profile_level == 2 && strcmp(nm, "msm_accumulate") != 0) return;   // level 2: the dominant kernel only
    auto take = [&]() -> hipEvent_t {
        if (!c->event_pool.empty()) {
            hipEvent_t e = c->event_pool.back();
            c->event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    };
    a = take();
    b = take();
    (void)hipEventRecord(a, st);
}
ProfScope::~ProfScope() {
    if (!a) return;
    (void)hipEventRecord(b, st);
    c->prof[name].pending.emplace_back(a, b);
}
void zk_prof_collect(zk_ctx* c) {
    for (auto& kv : c->prof) {
        ProfEntry& pe = kv.second;
        for (auto& ev : pe.pending) {
            (void)hipEventSynchronize(ev.second);
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
                pe.total_ms += ms;
                pe.launches += 1;
            }
            c->event_pool.push_back(ev.first);
            c->event_pool.push_back(ev.second);
        }
        pe.pending.clear();
    }
}

void host_parallel_for(uint32_t n, const std::function<void(uint32_t)>& fn) {
    static std::mutex mu;                     // HostPool::run is one batch at a time
    static HostPool pool(7);
    std::lock_guard<std::mutex> lk(mu);
    pool.run(n, fn);
}

extern "C" {

const char* zk_strerror(int code) {
    switch (code) {
    case ZK_OK: return "ok";
    case ZK_ERR_BAD_ARG: return "bad argument";
    case ZK_ERR_DOMAIN_TOO_LARGE: return "evaluation domain larger than the field's two-adicity";
    case ZK_ERR_HIP: return g_last_hip[0] ? g_last_hip : "HIP runtime error";
    case ZK_ERR_OOM: return "out of device memory";
    case ZK_ERR_NO_DEVICE: return "no usable HIP device";
    case ZK_ERR_UNSUPPORTED: return "size not supported";
    case ZK_ERR_NOT_INVERTIBLE: return "zero denominator in a grand product";
    case ZK_ERR_NOT_INDEXED: return "lookup query value not in the table";
    case ZK_ERR_PENDING: return "a deferred commitment round is open on this ctx (zk_kzg_round_end closes it)";
    default: return "unknown error";
    }
}

const char* zk_build_info(void) { return "ark_plonk_amd gfx950 (CDNA4) hipcc; NTT+MSM hot path"; }

int zk_ctx_create(int device, zk_ctx** out) {
    if (!out) return ZK_ERR_BAD_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ZK_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return ZK_ERR_BAD_ARG;
    int prev = 0;
    (void)hipGetDevice(&prev);
    ZK_HIP_TRY(hipSetDevice(device));
    zk_ctx* c = new zk_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        (void)hipSetDevice(prev);
        return ZK_ERR_HIP;
    }
    c->stream = c->own_stream;
    {
        const unsigned hc = std::thread::hardware_concurrency();
        c->tune.host_workers = hc > 16 ? 15 : hc > 1 ? (int)hc - 1 : 0;     // + the calling thread; option "host_workers" resizes it
        c->pool.reset(new HostPool((unsigned)c->tune.host_workers));
    }
    c->key_from_os = zk_process_key(c->ccache.digest_key);
    c->ccache.digest_key[0] ^= (uint64_t)(uintptr_t)c * 0x9E3779B97F4A7C15ull;      // caches are per ctx: so are their keys
    for (int i = 0; i < ZK_MAX_JOBS && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ev_job[i], hipEventDisableTiming);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        zk_ctx_destroy(c);
        return ZK_ERR_HIP;
    }
    *out = c;
    return ZK_OK;
}

void zk_ctx_destroy(zk_ctx* c) {
    if (!c) return;
    {
        Guard g(c);
        (void)hipStreamSynchronize(c->stream);
        zk_prof_collect(c);
        for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
        ntt_ctx_free(c);
        DevBuf* bufs[] = {&c->io.a, &c->io.b, &c->msm_tmp, &c->stage_shared, &c->witness};
        for (DevBuf* b : bufs) b->release();
        for (int i = 0; i < ZK_MAX_JOBS; ++i) c->mb[i].release();
        res_clear(c);
        for (int i = 0; i < ZK_MAX_JOBS; ++i)
            if (c->ev_job[i]) (void)hipEventDestroy(c->ev_job[i]);
        if (c->round.ev) (void)hipEventDestroy(c->round.ev);
        if (c->pinned) (void)hipHostFree(c->pinned);
        if (c->pinned_small) (void)hipHostFree(c->pinned_small);
        if (c->round.pinned_jobs) (void)hipHostFree(c->round.pinned_jobs);
        zk_io_release(c);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    }
    delete c;
}

static int switch_stream(zk_ctx* c, hipStream_t st) {      // what is queued finishes on the stream it was queued on
    Guard g(c);
    ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = st;
    return ZK_OK;
}
int zk_ctx_set_stream(zk_ctx* c, void* hip_stream) { return c ? switch_stream(c, (hipStream_t)hip_stream) : ZK_ERR_BAD_ARG; }
int zk_ctx_use_own_stream(zk_ctx* c) { return c ? switch_stream(c, c->own_stream) : ZK_ERR_BAD_ARG; }

int zk_ctx_sync(zk_ctx* c) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    return ZK_OK;
}

int zk_ctx_set_msm_window(zk_ctx* c, int w) {
    if (!c || w < 0 || w > 16 || w == 1) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    c->msm_window = w;
    return ZK_OK;
}

// Tuning options (ZkTune, ctx.h).  Refused while a round is open: a job's plan must not change between its accumulation and its reduction.
static int* tune_field(zk_ctx* c, const char* key, int64_t* lo, int64_t* hi) {
    struct Row {
        const char* key;
        int ZkTune::*field;
        int64_t lo, hi;
    };
    static const Row rows[] = {
        {"msm_merge", &ZkTune::msm_merge, 0, 1},         {"pre_vw", &ZkTune::pre_vw, 0, 512},
        {"pre_logg", &ZkTune::pre_logg, -1, 5},          {"chunk_l", &ZkTune::chunk_l, 0, 1024},
        {"long_rounds", &ZkTune::long_rounds, 1, 16},    {"combine_sg", &ZkTune::combine_sg, 0, 4},
        {"pre_max_log_n", &ZkTune::pre_max_log_n, 0, 25}, {"mem_reserve_mb", &ZkTune::mem_reserve_mb, 0, 1 << 20},
        {"round_mem_limit_mb", &ZkTune::round_mem_limit_mb, 0, 1 << 20}, {"ntt_passes", &ZkTune::ntt_passes, 0, 4},
    };
    for (const Row& r : rows)
        if (strcmp(key, r.key) == 0) {
            *lo = r.lo;
            *hi = r.hi;
            return &(c->tune.*(r.field));
        }
    return nullptr;
}

int zk_ctx_set_option(zk_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    int64_t lo = 0, hi = 0;
    if (strcmp(key, "cache_verify") == 0) {
        if (value < 0 || value > 1) return ZK_ERR_BAD_ARG;
        c->cache_verify = value != 0;
        return ZK_OK;
    }
    if (strcmp(key, "host_workers") == 0) {
        if (value < 0 || value > 63) return ZK_ERR_BAD_ARG;
        c->pool.reset(new HostPool((unsigned)value));      // joins the old workers first (no batch is running: the ctx lock is held)
        c->tune.host_workers = (int)value;
        return ZK_OK;
    }
    int* f = tune_field(c, key, &lo, &hi);
    if (!f) return ZK_ERR_UNSUPPORTED;
    if (value < lo || value > hi) return ZK_ERR_BAD_ARG;
    if (f == &c->tune.pre_vw && value && (value < 8 || (value & (value - 1)))) return ZK_ERR_BAD_ARG;
    if (f == &c->tune.chunk_l && value && value < 8) return ZK_ERR_BAD_ARG;
    if (f == &c->tune.combine_sg && value == 3) return ZK_ERR_BAD_ARG;
    if (f == &c->tune.pre_max_log_n && value && value < 13) return ZK_ERR_BAD_ARG;
    *f = (int)value;
    return ZK_OK;
}

int zk_ctx_get_option(zk_ctx* c, const char* key, int64_t* value) {
    if (!c || !key || !value) return ZK_ERR_BAD_ARG;
    Guard g(c);
    int64_t lo = 0, hi = 0;
    if (strcmp(key, "host_workers") == 0) {
        *value = c->tune.host_workers;
        return ZK_OK;
    }
    if (strcmp(key, "cache_verify") == 0) {
        *value = c->cache_verify ? 1 : 0;
        return ZK_OK;
    }
    int* f = tune_field(c, key, &lo, &hi);
    if (!f) return ZK_ERR_UNSUPPORTED;
    *value = *f;
    return ZK_OK;
}

int zk_cache_verify_stats(zk_ctx* c, uint64_t* checked, uint64_t* mismatches) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (checked) *checked = c->verify_checked;
    if (mismatches) *mismatches = c->verify_mismatch;
    return ZK_OK;
}

int zk_profile_enable(zk_ctx* c, int on) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    c->profiling = on != 0;
    c->profile_level = on;
    return ZK_OK;
}
int zk_profile_reset(zk_ctx* c) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    zk_prof_collect(c);
    for (auto& kv : c->prof) {
        kv.second.total_ms = 0;
        kv.second.launches = 0;
    }
    return ZK_OK;
}
int zk_profile_get(zk_ctx* c, const char* name, double* total_ms, uint64_t* launches) {
    if (!c || !name) return ZK_ERR_BAD_ARG;
    Guard g(c);
    zk_prof_collect(c);
    auto it = c->prof.find(name);
    double t = 0;
    uint64_t n = 0;
    if (it != c->prof.end()) {
        t = it->second.total_ms;
        n = it->second.launches;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = n;
    return ZK_OK;
}

int zk_io_stats(zk_ctx* c, uint64_t* h2d_bytes, uint64_t* d2h_bytes, int reset) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (h2d_bytes) *h2d_bytes = c->io.h2d_bytes;
    if (d2h_bytes) *d2h_bytes = c->io.d2h_bytes;
    if (reset) c->io.h2d_bytes = c->io.d2h_bytes = 0;
    return ZK_OK;
}

int zk_ctx_set_staging(zk_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 1) return ZK_ERR_BAD_ARG;
    Guard g(c);
    c->io.staging_mode = mode;
    return ZK_OK;
}

int zk_dev_alloc(zk_ctx* c, size_t bytes, void** d_ptr) {
    if (!c || !d_ptr) return ZK_ERR_BAD_ARG;
    Guard g(c);
    *d_ptr = nullptr;
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) {
        *d_ptr = nullptr;
        return zk_alloc_refused();
    }
    return ZK_OK;
}
int zk_dev_free(zk_ctx* c, void* d_ptr) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    if (d_ptr) ZK_HIP_TRY(hipFree(d_ptr));
    return ZK_OK;
}
// a plain copy on the ctx stream; wait: the host has the bytes (or its buffer back) when the call returns
static int copy_on_stream(zk_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, bool wait) {
    if (!c || (bytes && (!dst || !src))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (bytes) ZK_HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    if (wait) ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    return ZK_OK;
}
int zk_dev_upload(zk_ctx* c, void* d_dst, const void* h_src, size_t bytes) { return copy_on_stream(c, d_dst, h_src, bytes, hipMemcpyHostToDevice, true); }
int zk_dev_download(zk_ctx* c, void* h_dst, const void* d_src, size_t bytes) { return copy_on_stream(c, h_dst, d_src, bytes, hipMemcpyDeviceToHost, true); }
int zk_dev_copy(zk_ctx* c, void* d_dst, const void* d_src, size_t bytes) { return copy_on_stream(c, d_dst, d_src, bytes, hipMemcpyDeviceToDevice, false); }

}  // extern "C"
