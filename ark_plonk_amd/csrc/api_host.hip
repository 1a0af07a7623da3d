// The host-pointer entry points (the drop-in boundary): the caller's slices are uploaded -- or found in the residency cache -- and the
// device entry points do the rest.
#include "api_internal.h"

static int ensure_copy_stream(zk_ctx* c) {
    if (!c->io.copy_stream) ZK_HIP_TRY(hipStreamCreateWithFlags(&c->io.copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < ZK_MAX_JOBS; ++i)
        if (!c->io.ev_up[i]) ZK_HIP_TRY(hipEventCreateWithFlags(&c->io.ev_up[i], hipEventDisableTiming));
    return ZK_OK;
}

extern "C" {

int zk_ntt(zk_ctx* c, int curve_id, int kind, uint32_t log_n, const uint64_t* in, size_t in_len, uint64_t* out) {
    if (!c || !out || (!in && in_len)) return ZK_ERR_BAD_ARG;
    if (!zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (log_n > 32) return ZK_ERR_DOMAIN_TOO_LARGE;
    Guard g(c);
    const size_t n = (size_t)1 << log_n;
    if (in_len > n) return ZK_ERR_BAD_ARG;
    int rc;
    // residency cache.  Which vectors come back is a property of the transforms' direction: the OUTPUT of an inverse transform is a
    // coefficient vector -- what PC::commit, PC::open and the coset transforms take next (prover.rs:196-213, quotient_poly.rs:72-120)
    // -- so it is produced into a cache entry and named by the digest of the bytes the caller receives; the INPUT of a forward
    // transform is a coefficient vector, so it is looked up (and not inserted on a miss: only commitments insert what they upload).
    // Inputs of inverse transforms and outputs of forward ones are evaluation vectors, made and consumed by host code: never digested.
    // (A policy about time only: a vector that is not looked up is simply uploaded.)
    const bool inverse = kind == ZK_NTT_IFFT || kind == ZK_NTT_COSET_IFFT;
    const void* d_in = nullptr;
    bool need_upload = in_len != 0;
    ResEntry* out_entry = nullptr;
    ResCall rcall(c);
    if (c->res.on) {
        if (!inverse && res_wants(c, in_len * 32)) {
            uint64_t dig[4];
            if (ResEntry* e = res_lookup(c, in, in_len * 32, dig)) {
                d_in = e->buf.p;
                need_upload = false;
            }
        }
        if (inverse && res_wants(c, n * 32)) out_entry = res_new(c, n * 32);
    }
    if (!d_in) {
        if ((rc = c->io.a.ensure((in_len ? in_len : 1) * 32))) return rc;
        d_in = c->io.a.p;
    }
    void* d_out = out_entry ? out_entry->buf.p : nullptr;
    if (!d_out) {
        if ((rc = c->io.b.ensure(n * 32))) return rc;
        d_out = c->io.b.p;
    }
    if (need_upload && (rc = zk_h2d(c, const_cast<void*>(d_in), in, in_len * 32, c->stream))) return rc;
    rc = ntt_run_dev(c, curve_id, kind, log_n, d_in, in_len, d_out);
    if (!rc) rc = zk_d2h(c, out, d_out, n * 32, c->stream);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = ZK_ERR_HIP;
    if (rc) return rc;                 // ~ResCall drops out_entry with everything else this call touched
    if (out_entry) {
        res_digest(c, out, n * 32, out_entry->dig);
        out_entry->valid = true;
    }
    return rcall.done(ZK_OK);
}

int zk_ntt_batch(zk_ctx* c, int curve_id, int kind, uint32_t log_n, uint32_t n_polys, const uint64_t* const* ins, const size_t* in_lens,
                 uint64_t* const* outs) {
    if (!c || (n_polys && (!ins || !in_lens || !outs))) return ZK_ERR_BAD_ARG;
    Guard g(c);   // one lock for the whole batch; the transforms share the plan
    for (uint32_t i = 0; i < n_polys; ++i) {
        int rc = zk_ntt(c, curve_id, kind, log_n, ins[i], in_lens[i], outs[i]);
        if (rc) return rc;
    }
    return ZK_OK;
}

// PC::commit(ck, polys) with the caller's host slices (prover.rs:213 passes 4 polynomials, :579 and :606 seven):
// polynomial k+1 is uploaded (pinned staging ring, copy stream) while polynomial k's MSM runs.
int zk_kzg_commit_batch(zk_ctx* c, zk_srs* s, uint32_t n_polys, const uint64_t* const* coeffs_mont, const size_t* lens, uint64_t* out_xy,
                        uint8_t* out_inf) {
    if (!c || !s || s->device != c->device || (n_polys && (!coeffs_mont || !lens || !out_xy))) return ZK_ERR_BAD_ARG;
    if (n_polys > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_BAD_ARG;
    for (uint32_t k = 0; k < n_polys; ++k)
        if (lens[k] && !coeffs_mont[k]) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    SrsRead rl(s->mu);
    int rc = ensure_copy_stream(c);
    if (rc) return rc;
    // residency cache: polynomials this ctx produced (zk_ntt outputs) or uploaded before are used where they lie; the others go up
    // into a fresh entry (resident from then on) or, where the cache cannot take them, into the job's staging buffer.  Polynomial k is
    // digested right before job k is queued, i.e. while the GPU runs job k - 1: like the uploads, the digests hide under the MSMs.
    // Every job gets a stable input pointer up front (a fresh entry or its staging buffer); a hit copies nothing into it and points the
    // job at the resident copy instead -- d_in[k] is read when job k is queued, after up(k) has run.
    const void* d_in[ZK_MAX_JOBS];
    bool cached[ZK_MAX_JOBS] = {false};
    ResCall rcall(c);
    for (uint32_t k = 0; k < n_polys; ++k) {
        if (lens[k] > s->n) return ZK_ERR_BAD_ARG;
        cached[k] = res_wants(c, lens[k] * 32);
        if ((rc = c->mb[k].upload.ensure((lens[k] ? lens[k] : 1) * 32))) return rc;
        d_in[k] = c->mb[k].upload.p;
    }
    BeforeJob up = [&](uint32_t k) -> int {
        if (lens[k] == 0) return ZK_OK;
        if (cached[k]) {
            uint64_t dig[4];
            if (ResEntry* e = res_lookup(c, coeffs_mont[k], lens[k] * 32, dig)) {
                d_in[k] = e->buf.p;                // resident: nothing crosses PCIe, nothing to wait for
                return ZK_OK;
            }
            if (ResEntry* f = res_new(c, lens[k] * 32)) {
                memcpy(f->dig, dig, 32);
                f->valid = true;                       // its bytes go up in stream order before anything reads them
                d_in[k] = f->buf.p;
            }
        }
        int r = zk_h2d(c, const_cast<void*>(d_in[k]), coeffs_mont[k], lens[k] * 32, c->io.copy_stream);
        if (r) return r;
        ZK_HIP_TRY(hipEventRecord(c->io.ev_up[k], c->io.copy_stream));
        ZK_HIP_TRY(hipStreamWaitEvent(c->stream, c->io.ev_up[k], 0));
        return ZK_OK;
    };
    if (c->ccache.on) {   // the digests need every input on the device first
        for (uint32_t k = 0; k < n_polys; ++k)
            if ((rc = up(k))) return rc;
        return rcall.done(batch_cached_locked(c, s, n_polys, d_in, lens, nullptr, out_xy, out_inf));
    }
    return rcall.done(batch_locked(c, s, n_polys, d_in, lens, nullptr, nullptr, out_xy, out_inf, &up));
}

int zk_kzg_commit(zk_ctx* c, zk_srs* s, const uint64_t* coeffs_mont, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    return zk_kzg_commit_batch(c, s, 1, &coeffs_mont, &n, out_xy, out_inf);
}

// PC::open with the caller's host slices: the polynomials are uploaded (staged), everything else as zk_kzg_open_dev
int zk_kzg_open(zk_ctx* c, zk_srs* s, uint32_t n_polys, const uint64_t* const* polys_mont, const size_t* lens, const uint64_t* z_mont,
                const uint64_t* challenge_mont, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !s || s->device != c->device || !out_xy || !z_mont || !challenge_mont || (n_polys && (!polys_mont || !lens))) return ZK_ERR_BAD_ARG;
    if (n_polys > (uint32_t)ZK_MAX_JOBS) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    const void* d_in[ZK_MAX_JOBS];
    ResInput ri[ZK_MAX_JOBS];
    for (uint32_t k = 0; k < n_polys; ++k)
        if (lens[k] && !polys_mont[k]) return ZK_ERR_BAD_ARG;
    ResCall rcall(c);
    if (c->res.on) {      // the eleven / seven polynomials of an opening were all transformed or committed before (prover.rs:582-618)
        const void* hp[ZK_MAX_JOBS];
        size_t hb[ZK_MAX_JOBS];
        for (uint32_t k = 0; k < n_polys; ++k) {
            hp[k] = polys_mont[k];
            hb[k] = lens[k] * 32;
        }
        res_resolve(c, n_polys, hp, hb, ri);
    }
    for (uint32_t k = 0; k < n_polys; ++k) {
        int rc;
        if (ri[k].d_ptr) {
            d_in[k] = ri[k].d_ptr;
        } else {
            if ((rc = c->mb[k].upload.ensure((lens[k] ? lens[k] : 1) * 32))) return rc;
            d_in[k] = c->mb[k].upload.p;
        }
        if (ri[k].upload && (rc = zk_h2d(c, const_cast<void*>(d_in[k]), polys_mont[k], lens[k] * 32, c->stream))) return rc;
    }
    return rcall.done(zk_kzg_open_dev(c, s, n_polys, d_in, lens, z_mont, challenge_mont, out_xy, out_inf));
}

}  // extern "C"
