// Residency cache of the host-pointer entry points (zk_ctx::Residency, ctx.h): every function that writes its state.  ctx lock held
// by the callers (api_internal.h).
#include "api_internal.h"

constexpr uint64_t RES_SEED = 0x52455349444Eull;

// the buffer of an evicted / dropped entry: kept for reuse (no hipMalloc in the steady state) while the free list stays within an
// eighth of the cache's capacity and eight buffers -- device memory beyond the capacity that no statistic showed
static void res_recycle(zk_ctx* c, DevBuf& buf) {
    size_t held = 0;
    for (const DevBuf& b : c->res.free_bufs) held += b.cap;
    if (c->res.free_bufs.size() < 8 && held + buf.cap <= c->res.cap / 8) c->res.free_bufs.push_back(buf);
    else buf.release();
    buf = DevBuf();
}

// *held: the running call had touched the entry before this look-up -- an earlier input of the call may use its buffer
static ResEntry* res_find(zk_ctx* c, size_t bytes, const uint64_t dig[4], bool* held) {
    for (auto it = c->res.entries.begin(); it != c->res.entries.end(); ++it)
        if (it->valid && it->bytes == bytes && memcmp(it->dig, dig, 32) == 0) {
            *held = it->epoch == c->res.epoch;
            it->epoch = c->res.epoch;
            if (it != c->res.entries.begin()) c->res.entries.splice(c->res.entries.begin(), c->res.entries, it);
            ++c->res.hits;
            return &c->res.entries.front();
        }
    ++c->res.misses;
    return nullptr;
}

static void res_drop(zk_ctx* c, ResEntry* e);

// option "cache_verify": a hit is believed only after the resident bytes were compared with the caller's (both streams drained, one
// blocking download); a mismatch -- two vectors under one keyed digest, or a bug -- is counted, the entry dropped, the call uploads.
// An entry the running call already held (`held`: res_find) is NOT dropped: an earlier input of this res_resolve was given its buffer
// (two different vectors of one length under one digest in one batch: the first matched the resident bytes, the second does not).
// Dropped, the buffer would go to the free list, the res_new that follows for this very input would take it from there, and the
// upload would overwrite what the earlier input reads.  Such an entry is invalidated in place instead: it keeps its buffer and its
// epoch, so nothing evicts it while the call runs; no look-up finds it again, and eviction reclaims it like any other entry.  (No
// test builds two vectors under one keyed 256-bit digest; the argument stands in for one.)
static bool res_verify_hit(zk_ctx* c, ResEntry* e, const void* host_bytes, bool held) {
    if (!c->cache_verify) return true;
    if (e->born == c->res.epoch) return true;       // created by this very call (the same vector twice in one batch): its upload has not been queued yet
    (void)hipStreamSynchronize(c->stream);
    if (c->io.copy_stream) (void)hipStreamSynchronize(c->io.copy_stream);
    c->res.verify_host.resize(e->bytes);
    ++c->verify_checked;
    bool same = hipMemcpy(c->res.verify_host.data(), e->buf.p, e->bytes, hipMemcpyDeviceToHost) == hipSuccess &&
                memcmp(c->res.verify_host.data(), host_bytes, e->bytes) == 0;
    if (!same) {
        ++c->verify_mismatch;
        --c->res.hits;
        ++c->res.misses;
        if (held) e->valid = false;
        else res_drop(c, e);
    }
    return same;
}

ResEntry* res_new(zk_ctx* c, size_t bytes) {
    while (c->res.bytes + bytes > c->res.cap) {
        auto it = c->res.entries.end();
        bool found = false;
        while (it != c->res.entries.begin()) {
            --it;
            if (it->epoch != c->res.epoch) {
                found = true;
                break;
            }
        }
        if (!found) return nullptr;
        c->res.bytes -= it->bytes;
        res_recycle(c, it->buf);
        c->res.entries.erase(it);
    }
    DevBuf buf;
    for (size_t i = 0; i < c->res.free_bufs.size(); ++i)
        if (c->res.free_bufs[i].cap >= bytes && (buf.cap == 0 || c->res.free_bufs[i].cap < buf.cap)) buf = c->res.free_bufs[i];
    if (buf.cap) {
        for (size_t i = 0; i < c->res.free_bufs.size(); ++i)
            if (c->res.free_bufs[i].p == buf.p) {
                c->res.free_bufs.erase(c->res.free_bufs.begin() + (long)i);
                break;
            }
    } else if (buf.ensure(bytes) != ZK_OK) {
        return nullptr;
    }
    c->res.entries.emplace_front();
    ResEntry& e = c->res.entries.front();
    e.bytes = bytes;
    e.buf = buf;
    e.epoch = c->res.epoch;
    e.born = c->res.epoch;
    e.valid = false;
    c->res.bytes += bytes;
    return &e;
}

void res_digest(zk_ctx* c, const void* host, size_t bytes, uint64_t dig[4]) {
    host_digest256_multi(c->pool.get(), &host, &bytes, 1, RES_SEED, (uint64_t(*)[4])dig);
}
ResEntry* res_lookup(zk_ctx* c, const void* host, size_t bytes, uint64_t dig[4]) {
    res_digest(c, host, bytes, dig);
    bool held = false;
    ResEntry* e = res_find(c, bytes, dig, &held);
    return e && res_verify_hit(c, e, host, held) ? e : nullptr;
}

static void res_drop(zk_ctx* c, ResEntry* e) {        // an entry whose production failed
    for (auto it = c->res.entries.begin(); it != c->res.entries.end(); ++it)
        if (&*it == e) {
            c->res.bytes -= it->bytes;
            res_recycle(c, it->buf);
            c->res.entries.erase(it);
            return;
        }
}

void res_fail_call(zk_ctx* c) {
    for (auto it = c->res.entries.begin(); it != c->res.entries.end();) {
        if (it->epoch == c->res.epoch) {
            c->res.bytes -= it->bytes;
            res_recycle(c, it->buf);
            it = c->res.entries.erase(it);
        } else {
            ++it;
        }
    }
}

void res_clear(zk_ctx* c) {
    for (auto& e : c->res.entries) e.buf.release();
    c->res.entries.clear();
    for (auto& b : c->res.free_bufs) b.release();
    c->res.free_bufs.clear();
    c->res.bytes = 0;
}

void res_resolve(zk_ctx* c, uint32_t n, const void* const* h_ptrs, const size_t* bytes, ResInput* out) {
    const void* hp[ZK_MAX_JOBS];
    size_t hb[ZK_MAX_JOBS];
    uint32_t idx[ZK_MAX_JOBS], m = 0;
    for (uint32_t k = 0; k < n && k < (uint32_t)ZK_MAX_JOBS; ++k) {
        out[k] = ResInput();
        if (res_wants(c, bytes[k]) && h_ptrs[k]) {
            hp[m] = h_ptrs[k];
            hb[m] = bytes[k];
            idx[m++] = k;
        }
    }
    if (!m) return;
    uint64_t dig[ZK_MAX_JOBS][4];
    host_digest256_multi(c->pool.get(), hp, hb, m, RES_SEED, dig);
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t k = idx[j];
        bool held = false;
        ResEntry* e = res_find(c, hb[j], dig[j], &held);
        if (e && !res_verify_hit(c, e, hp[j], held)) e = nullptr;
        if (e) {
            out[k].d_ptr = e->buf.p;
            out[k].upload = false;
        } else if (ResEntry* f = res_new(c, hb[j])) {
            memcpy(f->dig, dig[j], 32);
            f->valid = true;            // its bytes go up in stream order before anything reads them
            out[k].d_ptr = f->buf.p;
        }
    }
}

extern "C" {

int zk_ctx_set_residency_cache(zk_ctx* c, int enable, size_t capacity_bytes, size_t max_vector_bytes) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    if (enable && !c->key_from_os) return ZK_ERR_UNSUPPORTED;     // as zk_ctx_set_commit_cache
    ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    if (capacity_bytes) c->res.cap = capacity_bytes;
    if (max_vector_bytes) c->res.max_vec = max_vector_bytes;
    c->res.on = enable != 0;
    if (!c->res.on) res_clear(c);
    return ZK_OK;
}

int zk_residency_cache_stats(zk_ctx* c, uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* bytes) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (hits) *hits = c->res.hits;
    if (misses) *misses = c->res.misses;
    if (entries) *entries = c->res.entries.size();
    if (bytes) *bytes = c->res.bytes;
    return ZK_OK;
}

}  // extern "C"
