// Deferred rounds (zk_kzg_round_begin_dev / zk_kzg_open_begin_dev ... zk_kzg_round_end): every function that writes the open round's
// state (zk_ctx::Round, ctx.h), apart from the three fields the MSM plan keeps there (ev, n_reduced, flushes).
#include "api_internal.h"

constexpr size_t PINNED_JOB_SLOT = 512;
static int ensure_pinned_jobs(zk_ctx* c) {
    if (c->round.pinned_jobs) return ZK_OK;
    if (hipHostMalloc(&c->round.pinned_jobs, ZK_MAX_JOBS * PINNED_JOB_SLOT, hipHostMallocDefault) != hipSuccess) return zk_alloc_refused();
    return ZK_OK;
}

// ---------------------------------------------------------------------- deferred rounds (begin ... end)
// ctx lock held.  Entry points that would reuse the buffer sets of queued jobs refuse while a round is open (ZK_ERR_PENDING).

static void round_clear(zk_ctx* c) {
    for (int k = 0; k < ZK_MAX_JOBS; ++k) c->mb[k].stage_of_job = 0;
    c->round.n = 0;
    c->round.srs = nullptr;
    c->round.reduced = false;
    c->round.partials = nullptr;
    c->round.n_reduced = 0;
}

// The memory budget closes the jobs queued so far: sorted, accumulated, reduced and combined NOW, their points parked
// in the pending entries in call order; their buffer sets are free for the jobs that follow.  The round itself stays open and
// zk_kzg_round_end returns the same points.  The caller holds the SRS lock.
static int round_flush_locked(zk_ctx* c) {
    zk_srs* s = c->round.srs;
    uint32_t slots[ZK_MAX_JOBS];
    size_t qlens[ZK_MAX_JOBS];
    const uint32_t nq = c->round.queued(slots, qlens);
    if (!nq) return ZK_OK;
    const int L = fq_limbs64(s->curve);
    uint64_t q_xyz[ZK_MAX_JOBS * ZK_MAX_JACOBIAN64];
    int rc = msm_ops(s->curve)->batch_pre_end(c, s, nq, slots, qlens, q_xyz, nullptr, nullptr);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    for (uint32_t q = 0; q < nq; ++q) {
        zk_ctx::Round::Job& pj = c->round.jobs[slots[q]];
        pj.queued = false;
        pj.have_xyz = true;
        copy_jacobian(pj.xyz, 0, q_xyz, q, L);
    }
    ++c->round.flushes;
    return ZK_OK;
}

// one table-path job into the buffer set of its slot, under the memory budget: no room -> close what is queued and reuse its sets;
// still no room -> give back every free set's buffers; only then ZK_ERR_OOM
static int round_begin_job_locked(zk_ctx* c, zk_srs* s, uint32_t slot, const void* d_in, size_t len, uint8_t kind) {
    int rc = msm_ops(s->curve)->batch_pre_begin(c, s, slot, 1, &d_in, &len, &kind, nullptr);
    if (rc != ZK_ERR_OOM) return rc;
    if ((rc = round_flush_locked(c))) return rc;
    rc = msm_ops(s->curve)->batch_pre_begin(c, s, slot, 1, &d_in, &len, &kind, nullptr);
    if (rc != ZK_ERR_OOM) return rc;
    zk_release_free_work(c, (int)slot);
    return msm_ops(s->curve)->batch_pre_begin(c, s, slot, 1, &d_in, &len, &kind, nullptr);
}

// jobs [0, n_jobs) appended to the open round; inputs on the device
static int round_append_locked(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens, const uint8_t* kinds) {
    if (c->round.n && c->round.srs != s) return ZK_ERR_BAD_ARG;
    if (c->round.reduced) return ZK_ERR_PENDING;          // zk_kzg_round_reduce closed the round to new jobs: zk_kzg_round_end first
    if (c->round.n + n_jobs > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_UNSUPPORTED;
    for (uint32_t k = 0; k < n_jobs; ++k)
        if (lens[k] > s->n || (lens[k] && !d_inputs[k])) return ZK_ERR_BAD_ARG;
    const uint32_t slot0 = c->round.n;
    int rc;
    if (c->ccache.on) {
        // the cache answers (or computes) at once; no job of such a round is ever queued, so the buffer sets are free
        uint64_t xy[ZK_MAX_JOBS * ZK_MAX_AFFINE64];
        uint8_t inf[ZK_MAX_JOBS];
        const int L = fq_limbs64(s->curve);
        if ((rc = batch_cached_locked(c, s, n_jobs, d_inputs, lens, kinds, xy, inf))) return rc;
        for (uint32_t k = 0; k < n_jobs; ++k) {
            zk_ctx::Round::Job& pj = c->round.jobs[slot0 + k];
            pj = zk_ctx::Round::Job();
            pj.n = lens[k];
            copy_affine(pj.xy, 0, xy, k, L);
            pj.inf = inf[k];
        }
        c->round.n += n_jobs;
        c->round.srs = s;
        return ZK_OK;
    }
    const bool table = s->pre_W != 0 && c->msm_window == 0;
    for (uint32_t k = 0; k < n_jobs; ++k) {
        const uint32_t slot = slot0 + k;
        zk_ctx::Round::Job& pj = c->round.jobs[slot];
        pj = zk_ctx::Round::Job();
        pj.n = lens[k];
        if (table && lens[k] >= ZK_PRE_MIN_N && lens[k] <= zk_pre_max_n(c)) {
            c->round.srs = s;
            if ((rc = round_begin_job_locked(c, s, slot, d_inputs[k], lens[k], kinds ? kinds[k] : 0))) return rc;
            pj.queued = true;
        } else {
            // short vector / no table: computed now, in this job's own buffer set (set 0 may belong to a queued job)
            auto run_now = [&]() {
                if (slot) std::swap(c->mb[0], c->mb[slot]);
                const int r = commit_one_locked(c, s, d_inputs[k], lens[k], kinds && kinds[k], pj.xyz);
                if (slot) std::swap(c->mb[0], c->mb[slot]);
                return r;
            };
            rc = run_now();
            if (rc == ZK_ERR_OOM) {        // the memory budget, as for a table-path job: close what is queued, give its sets back, once more
                c->round.srs = s;
                if ((rc = round_flush_locked(c))) return rc;
                zk_release_free_work(c, -1);
                rc = run_now();
            }
            if (rc) return rc;
            pj.have_xyz = true;
        }
        c->round.n = slot + 1;      // a failure further on leaves the jobs queued so far open: zk_kzg_round_end / _abort settles them
        c->round.srs = s;
    }
    return ZK_OK;
}

// closes the round: one reduction launch per kernel for every queued job, one wait, results in submission order
static int round_end_locked(zk_ctx* c, uint32_t n_expected, uint64_t* out_xyz, uint64_t* out_xy, uint8_t* out_inf) {
    const uint32_t n = c->round.n;
    zk_srs* s = c->round.srs;
    if (n != n_expected) return ZK_ERR_BAD_ARG;          // the round stays open
    if (c->round.partials) return ZK_ERR_PENDING;         // reduced towards the device (zk_kzg_round_reduce_winsums_dev): close it with _end_winsums_dev
    if (n == 0) return ZK_OK;
    const int L = fq_limbs64(s->curve);
    uint32_t slots[ZK_MAX_JOBS];
    size_t qlens[ZK_MAX_JOBS];
    const uint32_t nq = c->round.queued(slots, qlens);
    uint64_t q_xyz[ZK_MAX_JOBS * ZK_MAX_JACOBIAN64], q_xy[ZK_MAX_JOBS * ZK_MAX_AFFINE64];
    uint8_t q_inf[ZK_MAX_JOBS];
    int rc = ZK_OK;
    if (nq) {
        SrsRead rl(s->mu);
        rc = msm_ops(s->curve)->batch_pre_end(c, s, nq, slots, qlens, q_xyz, out_xy ? q_xy : nullptr, q_inf);
        // a failure before the wait (a plan, the pinned buffer) leaves the round's kernels in flight: they still read the caller's
        // inputs and the SRS, which the header lets the caller free once this call has returned
        if (rc) (void)hipStreamSynchronize(c->stream);
    }
    uint32_t q = 0;
    for (uint32_t k = 0; k < n && !rc; ++k) {
        const zk_ctx::Round::Job& pj = c->round.jobs[k];
        if (pj.queued) {
            if (out_xyz) copy_jacobian(out_xyz, k, q_xyz, q, L);
            if (out_xy) {
                copy_affine(out_xy, k, q_xy, q, L);
                if (out_inf) out_inf[k] = q_inf[q];
            }
            ++q;
        } else if (pj.have_xyz) {
            if (out_xyz) copy_jacobian(out_xyz, k, pj.xyz, 0, L);
            if (out_xy) rc = finish_point(s->curve, pj.xyz, out_xy + (size_t)k * 2 * L, out_inf ? out_inf + k : nullptr);
        } else {
            if (out_xyz) rc = ZK_ERR_UNSUPPORTED;         // the commitment cache holds affine points only
            if (out_xy) {
                copy_affine(out_xy, k, pj.xy, 0, L);
                if (out_inf) out_inf[k] = pj.inf;
            }
        }
    }
    round_clear(c);
    return rc;
}

// ctx lock held: queues everything up to every job's window sums at d_out + k * zk_winsums_dev_bytes, k = submission order.
// Whatever makes the device form impossible is found BEFORE anything is queued, so that ZK_ERR_UNSUPPORTED really leaves the
// round as it was (the accumulation used to have run, with the long-chunk plan, when a c >= 18 table was refused).
static int round_reduce_winsums_dev_locked(zk_ctx* c, void* d_out) {
    zk_srs* s = c->round.srs;
    const size_t pb = msm_ops(s->curve)->partial_dev_bytes();
    if (pb > PINNED_JOB_SLOT) return ZK_ERR_UNSUPPORTED;
    uint32_t slots[ZK_MAX_JOBS];
    size_t qlens[ZK_MAX_JOBS];
    void* outs[ZK_MAX_JOBS];
    uint32_t n_host = 0;
    for (uint32_t k = 0; k < c->round.n; ++k) {
        const zk_ctx::Round::Job& pj = c->round.jobs[k];
        if (!pj.queued && !pj.have_xyz) return ZK_ERR_UNSUPPORTED;         // the commitment cache holds affine points only
        if (!pj.queued) ++n_host;
    }
    SrsRead rl(s->mu);
    uint32_t vw = 0, vb = 0;
    if (!msm_ops(s->curve)->partial_dev_supported(c, s, &vw, &vb)) return ZK_ERR_UNSUPPORTED;   // no table, or one whose reduction finishes on the host (c >= 18)
    const size_t jb = (size_t)2 * vw * pb;                                  // bytes per job in d_out
    const uint32_t nq = c->round.queued(slots, qlens);
    for (uint32_t q = 0; q < nq; ++q) outs[q] = (char*)d_out + (size_t)slots[q] * jb;
    int rc;
    if (n_host && (rc = ensure_pinned_jobs(c))) return rc;
    if (nq && (rc = msm_ops(s->curve)->batch_pre_reduce(c, s, nq, slots, qlens, outs))) return rc;
    // jobs computed at submission (vectors too short for the table path) or parked by the memory budget: their host Jacobian, converted,
    // goes up in one small copy each from a pinned slot of its own (truly asynchronous; the slot is reused by the next round of this ctx
    // only, which begins after this one was waited for).  As window sums such a job is S_0 = the point, every other sum the point at infinity.
    for (uint32_t k = 0; k < c->round.n; ++k) {
        const zk_ctx::Round::Job& pj = c->round.jobs[k];
        if (pj.queued) continue;
        unsigned char* slot = (unsigned char*)c->round.pinned_jobs + (size_t)k * PINNED_JOB_SLOT;
        if ((rc = msm_ops(s->curve)->jacobian_to_partial_host(pj.xyz, slot))) return rc;
        char* dst = (char*)d_out + (size_t)k * jb;
        ZK_HIP_TRY(hipMemsetAsync(dst, 0, jb, c->stream));
        ZK_HIP_TRY(hipMemcpyAsync(dst, slot, pb, hipMemcpyHostToDevice, c->stream));
    }
    c->round.reduced = true;
    c->round.partials = d_out;
    return ZK_OK;
}

extern "C" {

int zk_kzg_round_begin_dev(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens, const uint8_t* kinds) {
    if (!c || !s || s->device != c->device || (n_jobs && (!d_inputs || !lens))) return ZK_ERR_BAD_ARG;
    if (n_jobs > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_BAD_ARG;
    Guard g(c);
    SrsRead rl(s->mu);
    return round_append_locked(c, s, n_jobs, d_inputs, lens, kinds);
}

int zk_kzg_open_begin_dev(zk_ctx* c, zk_srs* s, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* z_mont,
                          const uint64_t* challenge_mont) {
    if (!c || !s || s->device != c->device || !z_mont || !challenge_mont || (n_polys && (!d_polys || !lens))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    SrsRead rl(s->mu);
    if (c->round.reduced) return ZK_ERR_PENDING;
    if (c->round.n >= (uint32_t)ZK_MAX_JOBS) return ZK_ERR_UNSUPPORTED;
    if (c->round.n && c->round.srs != s) return ZK_ERR_BAD_ARG;
    void* d_w = nullptr;
    size_t wlen = 0;
    int rc = kzg_open_prepare_dev(c, s->curve, n_polys, d_polys, lens, z_mont, challenge_mont, &d_w, &wlen);
    if (rc == ZK_ERR_OOM) {
        // the combination / witness vectors (2 x 32 B per coefficient) found no room: close what is queued, free its sets, once more
        if ((rc = round_flush_locked(c))) return rc;
        zk_release_free_work(c, -1);
        rc = kzg_open_prepare_dev(c, s->curve, n_polys, d_polys, lens, z_mont, challenge_mont, &d_w, &wlen);
    }
    if (rc) return rc;
    if (wlen > s->n) return ZK_ERR_BAD_ARG;
    const void* in = d_w;
    const uint8_t kind = 1;
    return round_append_locked(c, s, 1, &in, &wlen, &kind);
}

int zk_kzg_round_reduce(zk_ctx* c) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (c->round.n == 0 || c->round.reduced) return ZK_OK;
    zk_srs* s = c->round.srs;
    uint32_t slots[ZK_MAX_JOBS];
    size_t qlens[ZK_MAX_JOBS];
    const uint32_t nq = c->round.queued(slots, qlens);
    if (nq) {
        SrsRead rl(s->mu);
        int rc = msm_ops(s->curve)->batch_pre_reduce(c, s, nq, slots, qlens, nullptr);
        if (rc) return rc;
    }
    c->round.reduced = true;
    return ZK_OK;
}

// ---- the same round closed with its result left ON THE DEVICE (multi-GPU exchange without a host hop): every job's 2 VW
// virtual-window sums S_v | T_v as the last reduction kernel writes them (zk_winsums_dev_bytes: 32 KiB per job at the default geometry).
// The combination sum_v S_v + B_v sum_v v T_v is linear in them, so the ranks add them element-wise after the all-gather
// (zk_g1_sum_winsums_dev: one throughput-shaped kernel) and the one combine per job stays on the host pool, as on a single GPU.
// (Round 4's other device form -- ONE point per job, formed by a further dependent quad launch -- measured last of the three
// exchanges on one card and was retired in round 6: profiles/design_history_msm.md.)
size_t zk_winsums_dev_bytes(zk_ctx* c, zk_srs* s) {
    if (!c || !s) return 0;
    Guard g(c);
    SrsRead rl(s->mu);
    uint32_t vw = 0, vb = 0;
    if (!msm_ops(s->curve)->partial_dev_supported(c, s, &vw, &vb)) return 0;
    return (size_t)2 * vw * msm_ops(s->curve)->partial_dev_bytes();
}

int zk_winsums_geometry(zk_ctx* c, zk_srs* s, uint32_t out[4]) {
    if (!c || !s || !out) return ZK_ERR_BAD_ARG;
    Guard g(c);
    SrsRead rl(s->mu);
    uint32_t vw = 0, vb = 0;
    if (!msm_ops(s->curve)->partial_dev_supported(c, s, &vw, &vb)) return ZK_ERR_UNSUPPORTED;
    out[0] = s->pre_c;
    out[1] = s->pre_W;
    out[2] = vw;
    out[3] = vb;
    return ZK_OK;
}

int zk_kzg_round_reduce_winsums_dev(zk_ctx* c, void* d_out) {
    if (!c || !d_out) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (c->round.n == 0) return ZK_OK;
    if (c->round.reduced) return c->round.partials == d_out ? ZK_OK : ZK_ERR_PENDING;
    return round_reduce_winsums_dev_locked(c, d_out);
}

int zk_kzg_round_end_winsums_dev(zk_ctx* c, uint32_t n_jobs, void* d_out) {
    if (!c || (n_jobs && !d_out)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (c->round.n != n_jobs) return ZK_ERR_BAD_ARG;           // the round stays open
    if (n_jobs == 0) return ZK_OK;
    int rc = ZK_OK;
    if (!c->round.reduced) rc = round_reduce_winsums_dev_locked(c, d_out);
    else if (c->round.partials != d_out) rc = ZK_ERR_PENDING;    // reduced towards the host or another buffer
    if (rc == ZK_ERR_PENDING || rc == ZK_ERR_UNSUPPORTED) return rc;   // nothing was queued by this call: the round stays open for the host form
    if (rc) (void)hipStreamSynchronize(c->stream);          // as round_end_locked: kernels of the round may still read the inputs
    round_clear(c);
    return rc;
}

int zk_g1_sum_winsums_dev(zk_ctx* c, zk_srs* s, const void* d_all, size_t ranks, uint32_t n_jobs, uint64_t* out_xy, uint8_t* out_inf) {
    if (n_jobs == 0) return ZK_OK;
    if (!c || !s || s->device != c->device || !d_all || !out_xy || ranks == 0) return ZK_ERR_BAD_ARG;
    if (n_jobs > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    return msm_ops(s->curve)->sum_winsums(c, s, d_all, ranks, n_jobs, out_xy, out_inf);
}

int zk_kzg_round_end(zk_ctx* c, uint32_t n_jobs, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || (n_jobs && !out_xy)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return round_end_locked(c, n_jobs, nullptr, out_xy, out_inf);
}

int zk_kzg_round_end_partial(zk_ctx* c, uint32_t n_jobs, uint64_t* out_xyz) {
    if (!c || (n_jobs && !out_xyz)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return round_end_locked(c, n_jobs, out_xyz, nullptr, nullptr);
}

int zk_kzg_round_pending(zk_ctx* c, uint32_t* n_jobs) {
    if (!c || !n_jobs) return ZK_ERR_BAD_ARG;
    Guard g(c);
    *n_jobs = c->round.n;
    return ZK_OK;
}

int zk_round_mem_stats(zk_ctx* c, uint64_t* flushes, uint64_t* set_bytes, uint64_t* device_free, uint64_t* device_total) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (flushes) *flushes = c->round.flushes;
    if (set_bytes) {
        uint64_t t = c->stage_shared.cap;
        for (int k = 0; k < ZK_MAX_JOBS; ++k) t += c->mb[k].work_bytes();
        *set_bytes = t;
    }
    if (device_free || device_total) {
        size_t fr = 0, tot = 0;
        ZK_HIP_TRY(hipMemGetInfo(&fr, &tot));
        if (device_free) *device_free = fr;
        if (device_total) *device_total = tot;
    }
    return ZK_OK;
}

int zk_kzg_round_abort(zk_ctx* c) {
    if (!c) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (c->round.n) (void)hipStreamSynchronize(c->stream);     // the queued kernels still read the caller's inputs
    round_clear(c);
    return ZK_OK;
}

}  // extern "C"
