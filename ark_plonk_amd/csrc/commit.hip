// MSM and KZG commitment entry points over device inputs that block until the result is on the host, and the ctx's commitment cache
// (zk_ctx::CommitCache, ctx.h): every function that writes its state.
#include "api_internal.h"
#include "g1_host.h"

static int ensure_pinned_small(zk_ctx* c) {
    if (c->pinned_small) return ZK_OK;
    if (hipHostMalloc(&c->pinned_small, 4096, hipHostMallocDefault) != hipSuccess) return zk_alloc_refused();
    return ZK_OK;
}

static int srs_slice(zk_srs* s, size_t base_offset, size_t n, const void** d_bases) {
    if (!s) return ZK_ERR_BAD_ARG;
    if (base_offset > s->n || n > s->n - base_offset) return ZK_ERR_BAD_ARG;
    *d_bases = (const char*)s->d_xy + base_offset * s->point_bytes;
    return ZK_OK;
}

// ctx lock and SRS read lock held
static int msm_partial_locked(zk_ctx* c, zk_srs* s, size_t base_offset, const void* d_scalars, size_t n, uint64_t* out_xyz) {
    const void* d_bases = nullptr;
    int rc = srs_slice(s, base_offset, n, &d_bases);
    if (rc) return rc;
    if (s->pre_W && n >= ZK_PRE_MIN_N && n <= zk_pre_max_n(c) && c->msm_window == 0) return msm_ops(s->curve)->run_pre(c, s, base_offset, d_scalars, n, out_xyz);
    if (s->pre_wstep > 1 && s->pre_w0 != 0) {
        // window-sharded table: what the MSM entry points of this SRS return is the rank's PARTIAL, and the ranks' partials add up, so a
        // vector that does not take the table path is computed (whole, per-window path) by the owner of window 0 only; here: infinity
        st_jacobian_inf(s->curve, out_xyz);
        return ZK_OK;
    }
    return msm_ops(s->curve)->run(c, d_bases, d_scalars, n, out_xyz);
}

// ------------------------------------------------------------------------------------ KZG commit
int commit_one_locked(zk_ctx* c, zk_srs* s, const void* d_in, size_t n, bool canonical, uint64_t* out_xyz) {
    if (n > s->n) return ZK_ERR_BAD_ARG;
    const void* sc = d_in;
    if (!canonical) {
        int rc = c->mb[0].scalars.ensure((n ? n : 1) * 32);
        if (rc) return rc;
        if ((rc = fr_convert_dev(c, s->curve, 0, d_in, n, c->mb[0].scalars.p))) return rc;
        sc = c->mb[0].scalars.p;
    }
    return msm_partial_locked(c, s, 0, sc, n, out_xyz);
}

int batch_locked(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens, const uint8_t* kinds,
                 uint64_t* out_xyz, uint64_t* out_xy, uint8_t* out_inf, const BeforeJob* before_job) {
    const int L = fq_limbs64(s->curve);
    bool fused = s->pre_W != 0 && c->msm_window == 0;
    for (uint32_t k = 0; k < n_jobs; ++k) {
        if (lens[k] > s->n || (lens[k] && !d_inputs[k])) return ZK_ERR_BAD_ARG;
        if (lens[k] < ZK_PRE_MIN_N || lens[k] > zk_pre_max_n(c)) fused = false;
    }
    if (fused) {
        uint64_t tmp[ZK_MAX_JOBS * ZK_MAX_JACOBIAN64];
        return msm_ops(s->curve)->batch_pre(c, s, n_jobs, d_inputs, lens, out_xyz ? out_xyz : tmp, kinds, out_xy, out_inf, before_job);
    }
    for (uint32_t k = 0; k < n_jobs; ++k) {
        int rc;
        if (before_job && (rc = (*before_job)(k))) return rc;
        uint64_t xyz[ZK_MAX_JACOBIAN64];
        if ((rc = commit_one_locked(c, s, d_inputs[k], lens[k], kinds && kinds[k], out_xyz ? out_xyz + (size_t)k * 3 * L : xyz))) return rc;
        if (out_xy && (rc = finish_point(s->curve, xyz, out_xy + (size_t)k * 2 * L, out_inf ? out_inf + k : nullptr))) return rc;
    }
    return ZK_OK;
}

namespace {
// the key of the commitment cache: a job's, or an entry's
struct CommitKey {
    uint64_t srs_id, n;
    uint32_t kind;
    const uint64_t* dig;
    bool operator==(const CommitKey& o) const { return srs_id == o.srs_id && n == o.n && kind == o.kind && !memcmp(dig, o.dig, 32); }
};
CommitKey key_of(const zk_ctx::CommitCache::Entry& e) { return CommitKey{e.srs_id, e.n, e.kind, e.dig}; }
}  // namespace

int batch_cached_locked(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens, const uint8_t* kinds,
                        uint64_t* out_xy, uint8_t* out_inf) {
    const int L = fq_limbs64(s->curve);
    if (!c->ccache.on || n_jobs == 0) return batch_locked(c, s, n_jobs, d_inputs, lens, kinds, nullptr, out_xy, out_inf, nullptr);
    int rc;
    if ((rc = c->ccache.digest_dev.ensure(ZK_MAX_JOBS * 32))) return rc;
    if ((rc = ensure_pinned_small(c))) return rc;
    if ((rc = dev_digest256(d_inputs, lens, n_jobs, (uint64_t*)c->ccache.digest_dev.p, c->stream, c->ccache.digest_key))) return rc;
    ZK_HIP_TRY(hipMemcpyAsync(c->pinned_small, c->ccache.digest_dev.p, (size_t)n_jobs * 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t* dig = (const uint64_t*)c->pinned_small;
    auto key = [&](uint32_t k) { return CommitKey{s->id, lens[k], kinds && kinds[k] ? 1u : 0u, dig + 4 * k}; };
    const void* miss_in[ZK_MAX_JOBS];
    size_t miss_len[ZK_MAX_JOBS];
    uint8_t miss_kind[ZK_MAX_JOBS];
    uint32_t miss_job[ZK_MAX_JOBS], n_miss = 0;
    int alias[ZK_MAX_JOBS];     // job k repeats miss alias[k] of this very call
    bool was_hit[ZK_MAX_JOBS] = {false};      // option "cache_verify": a hit is computed all the same and compared below
    uint64_t hit_xy[ZK_MAX_JOBS * ZK_MAX_AFFINE64];
    uint8_t hit_inf[ZK_MAX_JOBS];
    auto compute = [&](uint32_t k) {     // job k joins the batch that is computed below
        miss_in[n_miss] = d_inputs[k];
        miss_len[n_miss] = lens[k];
        miss_kind[n_miss] = (uint8_t)key(k).kind;
        miss_job[n_miss] = k;
        ++n_miss;
    };
    for (uint32_t k = 0; k < n_jobs; ++k) {
        alias[k] = -1;
        bool hit = false;
        for (auto it = c->ccache.entries.begin(); it != c->ccache.entries.end(); ++it) {
            if (key_of(*it) == key(k)) {
                copy_affine(out_xy, k, it->xy, 0, L);
                if (out_inf) out_inf[k] = it->inf;
                c->ccache.entries.splice(c->ccache.entries.begin(), c->ccache.entries, it);
                hit = true;
                break;
            }
        }
        if (hit) {
            ++c->ccache.hits;
            if (!c->cache_verify) continue;
            was_hit[k] = true;
            copy_affine(hit_xy, k, out_xy, k, L);
            hit_inf[k] = c->ccache.entries.front().inf;
            compute(k);
            continue;
        }
        for (uint32_t m = 0; m < n_miss && alias[k] < 0; ++m)
            if (key(miss_job[m]) == key(k)) alias[k] = (int)m;
        if (alias[k] >= 0) {
            ++c->ccache.hits;
            continue;
        }
        ++c->ccache.misses;
        compute(k);
    }
    uint64_t m_xy[ZK_MAX_JOBS * ZK_MAX_AFFINE64];
    uint8_t m_inf[ZK_MAX_JOBS];
    if (n_miss) {
        if ((rc = batch_locked(c, s, n_miss, miss_in, miss_len, miss_kind, nullptr, m_xy, m_inf, nullptr))) return rc;
        for (uint32_t m = 0; m < n_miss; ++m) {
            const uint32_t k = miss_job[m];
            copy_affine(out_xy, k, m_xy, m, L);
            if (out_inf) out_inf[k] = m_inf[m];
            if (was_hit[k]) {          // cache_verify: the entry exists; what it held against what was just computed
                ++c->verify_checked;
                if (hit_inf[k] != m_inf[m] || (!m_inf[m] && memcmp(hit_xy + (size_t)k * 2 * L, m_xy + (size_t)m * 2 * L, sizeof(uint64_t) * 2 * L))) {
                    ++c->verify_mismatch;
                    for (auto& ce : c->ccache.entries)
                        if (key_of(ce) == key(k)) {
                            copy_affine(ce.xy, 0, m_xy, m, L);
                            ce.inf = m_inf[m];
                        }
                }
                continue;
            }
            zk_ctx::CommitCache::Entry e;
            memset(&e, 0, sizeof e);
            e.srs_id = s->id;
            e.n = lens[k];
            e.kind = miss_kind[m];
            memcpy(e.dig, dig + 4 * k, 32);
            copy_affine(e.xy, 0, m_xy, m, L);
            e.inf = m_inf[m];
            c->ccache.entries.push_front(e);
        }
        while (c->ccache.entries.size() > c->ccache.cap) c->ccache.entries.pop_back();
    }
    for (uint32_t k = 0; k < n_jobs; ++k)
        if (alias[k] >= 0) {
            copy_affine(out_xy, k, m_xy, (size_t)alias[k], L);
            if (out_inf) out_inf[k] = m_inf[alias[k]];
        }
    return ZK_OK;
}

extern "C" {

int zk_msm_g1_srs_partial_dev(zk_ctx* c, zk_srs* s, size_t base_offset, const void* d_scalars, size_t n, uint64_t* out_xyz) {
    if (!c || !s || s->device != c->device || !out_xyz || (n && !d_scalars)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    return msm_partial_locked(c, s, base_offset, d_scalars, n, out_xyz);
}

int zk_msm_g1_srs_dev(zk_ctx* c, zk_srs* s, size_t base_offset, const void* d_scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    if (!out_xy) return ZK_ERR_BAD_ARG;
    uint64_t xyz[ZK_MAX_JACOBIAN64];
    int rc = zk_msm_g1_srs_partial_dev(c, s, base_offset, d_scalars, n, xyz);
    if (rc) return rc;
    return finish_point(s->curve, xyz, out_xy, out_inf);
}

int zk_msm_g1_srs(zk_ctx* c, zk_srs* s, size_t base_offset, const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !s || s->device != c->device || !out_xy || (n && !scalars)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    {
        int rc = c->mb[0].scalars.ensure((n ? n : 1) * 32);
        if (rc) return rc;
        if (n && (rc = zk_h2d(c, c->mb[0].scalars.p, scalars, n * 32, c->stream))) return rc;
    }
    return zk_msm_g1_srs_dev(c, s, base_offset, c->mb[0].scalars.p, n, out_xy, out_inf);
}

int zk_msm_g1(zk_ctx* c, int curve_id, const uint64_t* bases_xy, const uint8_t* inf_flags, const uint64_t* scalars, size_t n,
              uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !out_xy || (n && (!bases_xy || !scalars))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    zk_srs* s = nullptr;
    int rc = srs_register_host(c, curve_id, bases_xy, inf_flags, n, &s, false);   // ad-hoc bases: never cached
    if (rc) return rc;
    rc = zk_msm_g1_srs(c, s, 0, scalars, n, out_xy, out_inf);
    zk_srs_free(s);
    return rc;
}

int zk_g1_sum_partials(int curve_id, const uint64_t* partials_xyz, size_t count, uint64_t* out_xy, uint8_t* out_inf) {
    if (!out_xy || (count && !partials_xyz)) return ZK_ERR_BAD_ARG;
    return msm_ops(curve_id)->sum_partials_host(partials_xyz, count, out_xy, out_inf);
}

int zk_g1_sum_partials_batch(int curve_id, const uint64_t* partials_xyz, size_t ranks, uint32_t n_jobs, uint64_t* out_xy, uint8_t* out_inf) {
    if (n_jobs == 0) return ZK_OK;
    if (!out_xy || !partials_xyz || ranks == 0) return ZK_ERR_BAD_ARG;
    if (!zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    const size_t L = (size_t)fq_limbs64(curve_id);
    std::vector<int> rcs(n_jobs, 0);
    auto one = [&](uint32_t k) {
        std::vector<uint64_t> mine(ranks * 3 * L);
        for (size_t r = 0; r < ranks; ++r) copy_jacobian(mine.data(), r, partials_xyz, r * n_jobs + k, (int)L);
        rcs[k] = msm_ops(curve_id)->sum_partials_host(mine.data(), ranks, out_xy + (size_t)k * 2 * L, out_inf ? out_inf + k : nullptr);
    };
    for (uint32_t base = 0; base < n_jobs; base += 16) {   // bounded thread count
        const uint32_t cnt = n_jobs - base < 16 ? n_jobs - base : 16;
        host_parallel_for(cnt, [&](uint32_t k) { one(base + k); });
    }
    for (uint32_t k = 0; k < n_jobs; ++k)
        if (rcs[k]) return rcs[k];
    return ZK_OK;
}

int zk_ctx_set_commit_cache(zk_ctx* c, int enable, uint32_t capacity) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    if (enable && !c->key_from_os) return ZK_ERR_UNSUPPORTED;     // the digests that would address it have no OS entropy behind their key
    c->ccache.on = enable != 0;
    if (capacity) c->ccache.cap = capacity;
    if (!enable) c->ccache.entries.clear();
    while (c->ccache.entries.size() > c->ccache.cap) c->ccache.entries.pop_back();
    return ZK_OK;
}

int zk_commit_cache_stats(zk_ctx* c, uint64_t* hits, uint64_t* misses, uint64_t* entries) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (hits) *hits = c->ccache.hits;
    if (misses) *misses = c->ccache.misses;
    if (entries) *entries = c->ccache.entries.size();
    return ZK_OK;
}

int zk_kzg_commit_dev(zk_ctx* c, zk_srs* s, const void* d_coeffs_mont, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !s || s->device != c->device || !out_xy || (n && !d_coeffs_mont)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    if (n > s->n) return ZK_ERR_BAD_ARG;
    if (c->ccache.on && n) return batch_cached_locked(c, s, 1, &d_coeffs_mont, &n, nullptr, out_xy, out_inf);
    uint64_t xyz[ZK_MAX_JACOBIAN64];
    int rc = commit_one_locked(c, s, d_coeffs_mont, n, false, xyz);
    if (rc) return rc;
    return finish_point(s->curve, xyz, out_xy, out_inf);
}

int zk_kzg_commit_batch_partial_dev(zk_ctx* c, zk_srs* s, uint32_t n_polys, const void* const* d_coeffs_mont, const size_t* lens,
                                    uint64_t* out_xyz) {
    return zk_kzg_round_batch_partial_dev(c, s, n_polys, d_coeffs_mont, lens, nullptr, out_xyz);
}

int zk_kzg_round_batch_partial_dev(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens,
                                   const uint8_t* kinds, uint64_t* out_xyz) {
    if (!c || !s || s->device != c->device || (n_jobs && (!d_inputs || !lens || !out_xyz))) return ZK_ERR_BAD_ARG;
    if (n_jobs > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    return batch_locked(c, s, n_jobs, d_inputs, lens, kinds, out_xyz, nullptr, nullptr, nullptr);
}

int zk_kzg_commit_batch_dev(zk_ctx* c, zk_srs* s, uint32_t n_polys, const void* const* d_coeffs_mont, const size_t* lens,
                            uint64_t* out_xy, uint8_t* out_inf) {
    return zk_kzg_round_batch_dev(c, s, n_polys, d_coeffs_mont, lens, nullptr, out_xy, out_inf);
}

int zk_kzg_round_batch_dev(zk_ctx* c, zk_srs* s, uint32_t n_polys, const void* const* d_coeffs_mont, const size_t* lens,
                           const uint8_t* kinds, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !s || s->device != c->device || (n_polys && (!d_coeffs_mont || !lens || !out_xy))) return ZK_ERR_BAD_ARG;
    if (n_polys > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    return batch_cached_locked(c, s, n_polys, d_coeffs_mont, lens, kinds, out_xy, out_inf);
}

int zk_kzg_open_dev(zk_ctx* c, zk_srs* s, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* z_mont,
                    const uint64_t* challenge_mont, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !s || s->device != c->device || !out_xy || !z_mont || !challenge_mont || (n_polys && (!d_polys || !lens))) return ZK_ERR_BAD_ARG;
    void* d_w = nullptr;
    size_t wlen = 0;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    {
        int rc = kzg_open_prepare_dev(c, s->curve, n_polys, d_polys, lens, z_mont, challenge_mont, &d_w, &wlen);
        if (rc) return rc;
    }
    if (wlen > s->n) return ZK_ERR_BAD_ARG;
    uint64_t xyz[ZK_MAX_JACOBIAN64];
    int rc = msm_partial_locked(c, s, 0, d_w, wlen, xyz);
    if (rc) return rc;
    return finish_point(s->curve, xyz, out_xy, out_inf);
}

int zk_kzg_witness_dev(zk_ctx* c, int curve_id, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* z_mont,
                       const uint64_t* challenge_mont, void* d_out, size_t* out_len) {
    if (!c || !z_mont || !challenge_mont || !out_len || (n_polys && (!d_polys || !lens))) return ZK_ERR_BAD_ARG;
    void* d_w = nullptr;
    size_t wlen = 0;
    Guard g(c);
    int rc = kzg_open_prepare_dev(c, curve_id, n_polys, d_polys, lens, z_mont, challenge_mont, &d_w, &wlen);
    if (rc) return rc;
    *out_len = wlen;
    if (wlen) {
        if (!d_out) return ZK_ERR_BAD_ARG;
        ZK_HIP_TRY(hipMemcpyAsync(d_out, d_w, wlen * 32, hipMemcpyDeviceToDevice, c->stream));
    }
    return ZK_OK;
}

}  // extern "C"
