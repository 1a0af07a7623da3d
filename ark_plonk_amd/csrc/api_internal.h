// What the units of the C ABI (api_ctx / residency / srs / commit / round / api_host / api_poly .hip, ipa.hip, compile.hip, check.hip, the
// gadget units, verify.hip) share.
// Every function is listed once, with the locks its caller holds.  Not part of the C ABI.
#pragma once
#include "ctx.h"

#include <cstring>

// offsets inside one working-memory allocation, and the grid of a one-lane-per-item launch
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline unsigned blocks_of(uint64_t n, uint64_t t) { return (unsigned)((n + t - 1) / t); }

// the ctx lock, and the ctx's device made current for the calling thread
struct Guard {
    zk_ctx* c;
    std::unique_lock<std::recursive_mutex> lk;
    int prev = -1;
    bool ok = true;
    explicit Guard(zk_ctx* ctx) : c(ctx), lk(ctx->mu) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) ok = hipSetDevice(c->device) == hipSuccess;
    }
    ~Guard() {
        if (prev >= 0 && prev != c->device) (void)hipSetDevice(prev);
    }
};
// readers of an SRS (the MSM entry points) hold this from reading its pointers to the end of their kernel enqueue (zk_srs, ctx.h)
typedef std::shared_lock<std::shared_mutex> SrsRead;

inline int finish_point(int curve, const uint64_t* xyz, uint64_t* out_xy, uint8_t* out_inf) {
    return msm_ops(curve)->jacobian_to_affine_host(xyz, out_xy, out_inf);
}
// point ks of src (affine: 2 L limbs each; Jacobian: 3 L) to place kd of dst
inline void copy_affine(uint64_t* dst, size_t kd, const uint64_t* src, size_t ks, int L) {
    memcpy(dst + kd * 2 * L, src + ks * 2 * L, sizeof(uint64_t) * 2 * L);
}
inline void copy_jacobian(uint64_t* dst, size_t kd, const uint64_t* src, size_t ks, int L) {
    memcpy(dst + kd * 3 * L, src + ks * 3 * L, sizeof(uint64_t) * 3 * L);
}

// the working memory of one call: a device allocation freed on every path out of the call
struct DeviceAlloc {
    void* base = nullptr;
    ~DeviceAlloc() {
        if (base) (void)hipFree(base);                     // waits for the device: nothing queued still reads it
    }
};
// A call whose kernels report errors through one flag word (compile.hip, gadget_layout.hip, gadget_witness.hip): allocates
// 256 + work_bytes, clears the 256 of the flag word, runs body(d_flag, work) -- which queues the kernels on the ctx stream and returns
// a ZK_* code -- and reads the flag back once.  A set flag is ZK_ERR_BAD_ARG.  ctx lock held.
template <class Body>
int run_flagged(zk_ctx* c, size_t work_bytes, Body&& body) {
    DeviceAlloc wk;
    if (hipMalloc(&wk.base, 256 + work_bytes) != hipSuccess) {
        wk.base = nullptr;
        return zk_alloc_refused();
    }
    uint32_t* d_flag = (uint32_t*)wk.base;
    hipStream_t st = c->stream;
    int rc = [&]() -> int {
        ZK_HIP_TRY(hipMemsetAsync(d_flag, 0, 256, st));
        return body(d_flag, (void*)((char*)wk.base + 256));
    }();
    uint32_t flag = 0;
    if (!rc) rc = zk_d2h(c, &flag, d_flag, 4, st);                // the one read-back; also the wait before the buffer is freed
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    return flag ? ZK_ERR_BAD_ARG : ZK_OK;
}

// a deferred round (zk_kzg_round_begin_dev ...) holds the ctx's MSM buffer sets until zk_kzg_round_end.  ctx lock held.
inline bool round_open(const zk_ctx* c) { return c->round.n != 0; }

// ---- lookup_map.hip: the witness of a ZK_GADGET_LOOKUP_OUT segment -- one query of the table's (a, b, d) -> first-row map with the
// operands gathered from d_values by id and c written to d_values[var0 + k]; ZK_ERR_NOT_INDEXED on a miss.  ctx lock held.
int lookup_out_witness(zk_ctx* c, const zk_gadget_args& a, void* d_values);

// ---- srs.hip
// upload + convert; use_cache: look the content digest up first / publish the new handle.  Takes the ctx lock itself.
int srs_register_host(zk_ctx* c, int curve_id, const uint64_t* bases_xy, const uint8_t* inf_flags, size_t n, zk_srs** out, bool use_cache);

// ---- commit.hip: ctx lock and SRS read lock held, no round open (round.hip calls them for the jobs a round computes at submission)
typedef std::function<int(uint32_t)> BeforeJob;
// one commitment, no table / no batch: into_repr (unless canonical) + the per-window or single-job table MSM
int commit_one_locked(zk_ctx* c, zk_srs* s, const void* d_in, size_t n, bool canonical, uint64_t* out_xyz);
// the jobs of one PC call, no cache: fused window-table batch when every job qualifies, else one at a time.
// before_job(k) (optional) runs right before job k's kernels are queued (the host-pointer batch uploads job k there).
// Exactly one of out_xyz (Jacobian partials, 3L per job) / out_xy (affine, 2L per job) is non-null.
int batch_locked(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens, const uint8_t* kinds,
                 uint64_t* out_xyz, uint64_t* out_xy, uint8_t* out_inf, const BeforeJob* before_job);
// N3: the same with the ctx's content-addressed commitment cache in front (affine outputs only).
// Inputs must already be on the device (the digest is computed there).
int batch_cached_locked(zk_ctx* c, zk_srs* s, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens, const uint8_t* kinds,
                        uint64_t* out_xy, uint8_t* out_inf);

// ---- residency.hip: residency cache of the host-pointer entry points.  ctx lock held.
typedef zk_ctx::Residency::Entry ResEntry;
inline bool res_wants(const zk_ctx* c, size_t bytes) { return c->res.on && bytes >= 4096 && bytes <= c->res.max_vec; }
// the keyed digest of one host vector (on the ctx's host pool); res_lookup: ... and its entry if it is resident (counted as a hit,
// moved to the front) and, under option "cache_verify", its bytes equal the caller's; else nullptr (counted as a miss)
void res_digest(zk_ctx* c, const void* host, size_t bytes, uint64_t dig[4]);
ResEntry* res_lookup(zk_ctx* c, const void* host, size_t bytes, uint64_t dig[4]);
// a fresh entry of `bytes` at the front of the list (not yet valid), or nullptr when nothing may be evicted / allocated: the
// caller then takes the uncached path.  Evicted buffers are kept for reuse (hipFree synchronises the device).
ResEntry* res_new(zk_ctx* c, size_t bytes);
// a failed call: whatever it touched or created may hold bytes that never arrived
void res_fail_call(zk_ctx* c);
void res_clear(zk_ctx* c);

// Every host-pointer call that consults the cache runs inside one of these (a new epoch: what the call touches stays until it returns).
// An exit that was not marked ok() -- a failed allocation, a failed copy, a failed kernel launch, at ANY point of the call -- waits for
// both streams (uploads may still be in flight on the copy stream) and drops every entry the call touched or created: their digests
// may name bytes that never arrived (an early `return rc` used to leave such entries valid, and a retry with the same
// polynomials then committed over garbage).
struct ResCall {
    zk_ctx* c;
    bool active, good = false;
    explicit ResCall(zk_ctx* ctx) : c(ctx), active(ctx->res.on) {
        if (active) ++c->res.epoch;
    }
    int done(int rc) {
        good = rc == ZK_OK;
        return rc;
    }
    ~ResCall() {
        if (!active || good) return;
        (void)hipStreamSynchronize(c->stream);
        if (c->io.copy_stream) (void)hipStreamSynchronize(c->io.copy_stream);
        res_fail_call(c);
    }
};

// Inputs of one host-pointer call: for every vector the cache may hold (res_wants), its digest (all of them as ONE batch of work on
// the ctx's host pool) and, on a hit, the device copy.  On a miss a fresh entry takes the upload (the caller copies into *d_ptr and
// the vector is resident from then on); where the cache cannot take it, *d_ptr stays null and the caller uses its own staging buffer.
struct ResInput {
    const void* d_ptr = nullptr;   // device copy to use (hit, or the fresh entry a miss uploads into)
    bool upload = true;            // the bytes still have to go up
};
void res_resolve(zk_ctx* c, uint32_t n, const void* const* h_ptrs, const size_t* bytes, ResInput* out);
