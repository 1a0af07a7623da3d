/* ark_plonk_amd.h -- C ABI of the MI355X-native NTT + MSM prover hot path.
 *
 * Drop-in boundary for heliaxdev/ark-plonk's proof-generation inner loop.
 * Every entry point names the reference interface it replaces (file:line relative to the
 * reference tree) and, where the arithmetic lives in a crates.io dependency, the crate item the
 * reference calls there.  Plain pointers and sizes only; no torch / HIP types in signatures
 * (a HIP stream is passed as an opaque void*).
 *
 * Data formats (identical bytes to arkworks 0.3 in-memory values):
 *   Fr element  : 4 x uint64 little-endian limbs, Montgomery form (value * 2^256 mod r), < r.
 *   Fr scalar   : 4 x uint64 little-endian limbs, canonical integer (PrimeField::into_repr), < r.  No entry point checks
 *                 that: window tables whose scalars are folded (17 bits and wider) bring an integer in [r, 2^256) below r on the
 *                 way, a 16-bit table does not -- there such an integer with bits 240 .. 254 all set loses the carry out of its
 *                 top window and the sum is wrong, without an error.
 *   Fq element  : L x uint64 limbs (L = 6 BLS12-381, 4 BN254), Montgomery form (R = 2^(64L)).
 *   G1 affine   : x || y (2L limbs, packed) (arkworks' GroupAffine is not repr(C): the shim copies x, y, infinity).
 *                 The point at infinity is accepted in three encodings: inf_flags[i] != 0 (x, y ignored),
 *                 x = y = 0, and GroupAffine::zero() = (0, 1) with 1 in Montgomery form.  (0, 1) is on neither
 *                 supported curve, so no finite point is lost.
 *   Output point: affine x || y Montgomery; infinity is (0, 1) + flag 1, as GroupAffine::zero() -- an output may be
 *                 fed back as a base with or without its flag.
 *
 * Ownership: the caller owns every buffer; nothing is retained after return except the device
 * copy held by a zk_srs handle.  Errors: 0 = success, negative = failure (never aborts, never
 * throws).  Threading: calls on one ctx are serialised internally; one HIP stream per ctx, and the stream is ctx
 * state (zk_ctx_set_stream), so threads that want different streams use one ctx each -- ctxs are cheap and share
 * SRS handles.  One ctx drives one GPU: zk_ctx_create(int device) instead of SURVEY.md 8b's
 * (const int* devices, int n_dev) -- one process per GPU; multi-GPU MSM = one ctx per rank + an all-gather of
 * zk_msm_g1_*_partial outputs, see INTEGRATION.md.
 * Host-pointer entry points (zk_ntt, zk_kzg_commit(_batch), zk_kzg_open, zk_msm_g1(_srs), zk_srs_register) accept
 * ordinary pageable memory (zk_ctx_set_staging selects how it is moved); zk_io_stats reports the bytes moved.
 */
#ifndef ARK_PLONK_AMD_H
#define ARK_PLONK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_ctx zk_ctx;
typedef struct zk_srs zk_srs;

/* curve ids */
#define ZK_CURVE_BLS12_381 0
#define ZK_CURVE_BN254 1

/* transform kinds == ark_poly::EvaluationDomain methods */
#define ZK_NTT_FFT 0        /* EvaluationDomain::fft        (permutation/mod.rs:671-674)            */
#define ZK_NTT_IFFT 1       /* EvaluationDomain::ifft       (prover.rs:196-203,240-242,281-283,302-305) */
#define ZK_NTT_COSET_FFT 2  /* EvaluationDomain::coset_fft  (quotient_poly.rs:72-120,205,294)       */
#define ZK_NTT_COSET_IFFT 3 /* EvaluationDomain::coset_ifft (quotient_poly.rs:175-177)              */

/* error codes */
#define ZK_OK 0
#define ZK_ERR_BAD_ARG (-1)
#define ZK_ERR_DOMAIN_TOO_LARGE (-2) /* log_n > two-adicity: plonk-core/src/error.rs:14-21 InvalidEvalDomainSize */
#define ZK_ERR_HIP (-3)
#define ZK_ERR_OOM (-4)
#define ZK_ERR_NO_DEVICE (-5)
#define ZK_ERR_UNSUPPORTED (-6)
#define ZK_ERR_NOT_INVERTIBLE (-7) /* a grand-product denominator is zero (the reference panics: `inverse().unwrap()`) */
#define ZK_ERR_NOT_INDEXED (-8)    /* a lookup query value is not in the table (the reference's Error::ElementNotIndexed) */
#define ZK_ERR_PENDING (-9)        /* a deferred round (zk_kzg_round_begin_dev) is open on this ctx: close it with zk_kzg_round_end first */

const char* zk_strerror(int code);

/* ---- context -------------------------------------------------------------------------------- */
/* Create a context on HIP device `device` (one process per GPU). */
int zk_ctx_create(int device, zk_ctx** out);
void zk_ctx_destroy(zk_ctx* ctx);
/* Run all work of this ctx on an existing HIP stream (hipStream_t as void*).  NULL is HIP's
 * default (null) stream -- e.g. torch's default stream -- not "none". */
int zk_ctx_set_stream(zk_ctx* ctx, void* hip_stream);
/* Go back to the ctx's own non-blocking stream (the state after zk_ctx_create). */
int zk_ctx_use_own_stream(zk_ctx* ctx);
/* Block until all queued work of this ctx is complete. */
int zk_ctx_sync(zk_ctx* ctx);
/* Override the MSM window size c of the per-window path (0 = automatic, else 2..16). Test/tuning hook. */
int zk_ctx_set_msm_window(zk_ctx* ctx, int c);
/* Host<->device bytes moved by the host-pointer entry points of this ctx since creation / the last reset. */
int zk_io_stats(zk_ctx* ctx, uint64_t* h2d_bytes, uint64_t* d2h_bytes, int reset);
/* 0 (default): pageable host buffers are handed to hipMemcpyAsync as they are -- on the MI355X hosts that reaches the same
 * 56 GB/s as pinned memory; 1: through the ctx's pinned staging ring (49 GB/s there; for hosts whose runtime stages pageable
 * copies slowly).  Tuning hook, see tools/pcie_probe.py. */
int zk_ctx_set_staging(zk_ctx* ctx, int mode);
/* Tuning options of the MSM planner, per ctx, integers by name (SURVEY.md 5 "runtime ctx options"; until round 4 these were ZK_*
 * environment variables read inside the hot path).  Results are identical for every value; only launch shapes change.  Keys:
 *   "msm_merge"      1 (default): one sort / accumulation launch per round for all its deferred jobs; 0: per job at submission
 *   "pre_vw"         virtual windows of the shared-bucket reduction: 0 = default (64), else a power of two 8 .. 512
 *   "pre_logg"       log2 buckets per reduction segment: -1 = default, else 0 .. 5
 *   "chunk_l"        sorted references per accumulation lane: 0 = planned, else 8 .. 1024
 *   "long_rounds"    rounds of resident lanes given to a non-final job of a merged accumulation launch: 1 (default) .. 16
 *   "combine_sg"     lanes per small bucket in the combine kernel when a launch has more than two jobs: 0 = default (1), 2, 4
 *   "pre_max_log_n"  vectors longer than 2^value take the per-window path even over a table: 0 = built-in limit (2^26), 13 .. 25
 *                    (test hook; the ranks of a window-sharded MSM must agree on it, as on "pre_vw" / "pre_logg" for the
 *                    window-sum exchange below)
 *   "mem_reserve_mb"      device memory (MiB) the table path leaves alone when it decides whether another deferred job's buffer set
 *                         still fits (hipMemGetInfo): default 1024
 *   "round_mem_limit_mb"  test hook, 0 = off: the buffer sets of a round's QUEUED jobs may together hold at most this many MiB, so that
 *                         the early close described at zk_kzg_round_begin_dev can be exercised at small sizes
 *   "ntt_passes"     passes of an NTT: 0 (default) = by size (one to 2^9, two to 2^18, three to 2^27, four above); 1 .. 4: log_n is
 *                    split into that many passes by the same balanced rule (the first log_n % k passes get one bit more).  It exists
 *                    for tests and A/B runs: the four-pass plan is otherwise reached only from 2^28.  A transform whose split would
 *                    need a radix outside 2^3 .. 2^9 returns ZK_ERR_UNSUPPORTED and leaves its output untouched; transforms below 2^3
 *                    ignore the option.  Takes effect at the next transform; with profiling on, the counter "ntt_passes"
 *                    (zk_profile_get: launches) grows by one per pass launched
 *   "host_workers"        helper threads of the ctx's host pool (window-sum combine, affine normalisation, digests): default
 *                         min(15, hardware threads - 1); a launcher with several ranks per host passes cores / LOCAL_WORLD_SIZE - 1
 *   "cache_verify"        0 (default) | 1: every hit of the commitment cache is recomputed and every hit of the residency cache compared
 *                         byte for byte with the caller's vector before it is believed; mismatches are counted (zk_cache_verify_stats)
 *                         and the computed / uploaded value is used.  A diagnostic mode: it costs what the caches save
 * ZK_ERR_UNSUPPORTED: unknown key; ZK_ERR_BAD_ARG: value out of range; ZK_ERR_PENDING: a deferred round is open (a job's plan must
 * not change between its accumulation and its reduction).  The library reads NO environment variable on a compute path
 * (ZK_VERBOSE switches diagnostics on stderr only). */
/* Residency cache of the HOST-POINTER entry points (opt-in, per ctx; round 5).  The reference's call structure sends the same
 * vector across PCIe again and again: an `ifft` output goes straight back up as a `PC::commit` input (prover.rs:196-213), then as a
 * `coset_fft` input (quotient_poly.rs:72-120), then into the last round's commitments and openings (prover.rs:569-618) -- about 58 of
 * the 83 vectors an unchanged Prover::prove uploads per proof.  With the cache on, zk_ntt keeps the device copy of every output of at
 * most max_vector_bytes (named by a keyed 256-bit digest of the bytes the caller receives) and zk_ntt / zk_kzg_commit_batch / zk_kzg_open
 * digest every input of at most that size on the ctx's host pool and use the resident copy on a match; a miss uploads into a fresh
 * entry, so a second use of any vector hits too (the prover key's sigma polynomials, proof after proof).  A digest runs at ~190 GB/s
 * against PCIe's 56, so a hit costs a third of an upload and a miss a third more (profiles/r05/r05_notes.md).  WHAT IS GUARANTEED: results
 * are identical to the uncached calls UNLESS two different vectors of one length collide under the keyed 256-bit non-cryptographic
 * digest (per-process key from the operating system) -- a hit is taken on equality of (length, digest) of the caller's CURRENT bytes,
 * the contents are not compared: the trust model of zk_srs_register's registry below.  Option "cache_verify" = 1 compares them (and
 * recomputes every commitment-cache hit) and counts mismatches: zk_cache_verify_stats.  Without operating-system entropy behind the
 * key (getrandom and /dev/urandom both unavailable) enabling either cache returns ZK_ERR_UNSUPPORTED.  capacity_bytes = device memory the entries may hold (0 = leave unchanged; default 2 GiB, least recently used evicted;
 * entries of the running call are never evicted); max_vector_bytes: 0 = leave unchanged (default 64 MiB: at n = 2^20 the n-sized
 * vectors are cached, the 4n-sized coset evaluations -- consumed by host code, never sent back -- are not).  enable = 0 drops every entry. */
int zk_ctx_set_residency_cache(zk_ctx* ctx, int enable, size_t capacity_bytes, size_t max_vector_bytes);
int zk_residency_cache_stats(zk_ctx* ctx, uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* bytes);
int zk_ctx_set_option(zk_ctx* ctx, const char* key, int64_t value);
int zk_ctx_get_option(zk_ctx* ctx, const char* key, int64_t* value);
/* hits checked under option "cache_verify" and how many of them did not hold (either pointer may be NULL) */
int zk_cache_verify_stats(zk_ctx* ctx, uint64_t* checked, uint64_t* mismatches);

/* Per-kernel HIP-event timing (bench.py roofline leg). on = 1: every launch of the hot kernels is bracketed by
 * hipEventRecord on the ctx stream (≈ 200 scopes, ≈ 2 ms per 2^20 proof); on = 2: only the dominant kernel, msm_accumulate
 * (58 scopes per proof) -- what bench.py keeps on inside its timed region; 0: off. */
int zk_profile_enable(zk_ctx* ctx, int on);
int zk_profile_reset(zk_ctx* ctx);
/* name: "ntt_pass", "msm_accumulate", "msm_sort", "msm_reduce", ...; returns total ms and launch count */
int zk_profile_get(zk_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);

/* ---- a1: GeneralEvaluationDomain::new + EvaluationDomainExt (util.rs:24-88) ------------------- */
typedef struct zk_domain_info {
    uint64_t size;               /* 2^log_n                                   */
    uint32_t log_size_of_group;  /* EvaluationDomainExt::log_size_of_group    */
    uint32_t reserved;
    uint64_t size_inv[4];        /* ::size_inv        (Montgomery)            */
    uint64_t group_gen[4];       /* ::group_gen                               */
    uint64_t group_gen_inv[4];   /* ::group_gen_inv                           */
    uint64_t generator[4];       /* F::multiplicative_generator() (coset g)   */
    uint64_t generator_inv[4];   /* ::generator_inv                           */
} zk_domain_info;
/* Replaces GeneralEvaluationDomain::<F>::new(num_coeffs) (prover.rs:169-173,
 * quotient_poly.rs:64-69): size = next_power_of_two(num_coeffs). */
int zk_domain_new(int curve_id, uint64_t num_coeffs, zk_domain_info* out);

/* ---- a2-a5: NTT ------------------------------------------------------------------------------ */
/* Host-buffer transform.  in: in_len (<= 2^log_n) Montgomery Fr elements, zero-extended;
 * out: 2^log_n elements, natural order.  in == out allowed.
 * Replaces ark_poly Radix2EvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place.
 * Sizes: every log_n the reference admits (prover.rs:169-173, error.rs:14-21: up to the field's two-adicity, 32 for BLS12-381,
 * 28 for BN254; beyond it ZK_ERR_DOMAIN_TOO_LARGE, as Error::InvalidEvalDomainSize) -- one pass to 2^9, two to 2^18, three to 2^27,
 * four above.  What bounds the size in practice is memory: the vector, a work vector and the first pass boundary's twiddle table
 * are 2^log_n x 32 bytes each (8 GiB at 2^28); a size that does not fit the card returns ZK_ERR_OOM. */
int zk_ntt(zk_ctx* ctx, int curve_id, int kind, uint32_t log_n, const uint64_t* in, size_t in_len, uint64_t* out);
/* n_polys host-buffer transforms of one kind and size; ins[i] == outs[i] allowed. */
int zk_ntt_batch(zk_ctx* ctx, int curve_id, int kind, uint32_t log_n, uint32_t n_polys, const uint64_t* const* ins,
                 const size_t* in_lens, uint64_t* const* outs);
/* Same with device-resident buffers (async on the ctx stream).  d_in == d_out allowed. */
int zk_ntt_dev(zk_ctx* ctx, int curve_id, int kind, uint32_t log_n, const void* d_in, size_t in_len, void* d_out);
/* n_polys transforms of one kind/size sharing a plan (the 13 coset_fft of quotient_poly.rs:72-120). */
int zk_ntt_batch_dev(zk_ctx* ctx, int curve_id, int kind, uint32_t log_n, uint32_t n_polys,
                     const void* const* d_ins, const size_t* in_lens, void* const* d_outs);
/* Pre-build (and keep) the twiddle plan for (curve, log_n); otherwise built on first use. */
int zk_ntt_prepare(zk_ctx* ctx, int curve_id, uint32_t log_n);

/* Fr Montgomery <-> canonical on device (PrimeField::into_repr / from_repr; commitment.rs:37-40). */
int zk_fr_from_mont_dev(zk_ctx* ctx, int curve_id, const void* d_in, size_t n, void* d_out);
int zk_fr_to_mont_dev(zk_ctx* ctx, int curve_id, const void* d_in, size_t n, void* d_out);

/* ---- a6/a8: MSM ------------------------------------------------------------------------------ */
/* Replaces ark_ec::msm::VariableBaseMSM::multi_scalar_mul(bases, scalars) (commitment.rs:45,83)
 * followed by `.into()` affine.  n = min(len) pairs; inf_flags may be NULL. */
int zk_msm_g1(zk_ctx* ctx, int curve_id, const uint64_t* bases_xy, const uint8_t* inf_flags,
              const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf);

/* Device-resident SRS (CommitterKey::powers_of_g after PC::trim, circuit.rs:236,276).
 * A zk_srs belongs to the DEVICE of the registering ctx: every ctx of that device may use it (several proof streams
 * share one copy of the bases and of the window table).  It may outlive the ctx that registered it.
 * zk_srs_register is content-addressed: the reference trims on every gen_proof (circuit.rs:276), so registering
 * the same (curve, n, bases, flags) again returns the resident handle -- window table included -- after one pass of a
 * 256-bit digest over the host bytes, with no upload.  Handles are reference counted: call zk_srs_free once per
 * successful register.  An unreferenced cached SRS stays resident until zk_srs_cache_config's idle budget (default
 * 32 GiB) is exceeded, least recently used first.  zk_srs_register_dev (bases already on the device; d_inf_flags may
 * be NULL) is never cached.
 *
 * Trust model of the content-addressed caches (this one, zk_ctx_set_commit_cache, zk_ctx_set_residency_cache): a hit is accepted
 * on equality of a 256-bit digest, without comparing contents -- results are identical to the uncached call unless two inputs collide
 * under that digest.  The digests are KEYED with 256 bits drawn from the operating system once per process (the commitment cache
 * mixes in a per-ctx value); they are never exported, so a client that chooses the cached bytes cannot search for two inputs with
 * one digest offline; without operating-system entropy the registry shares nothing and the two ctx caches refuse to switch on.  The
 * mixing functions are fast NON-CRYPTOGRAPHIC ones (four xxhash-style lanes folded into each other every 256 bytes; a sum of
 * per-element keyed mixes on the device): a collision would return another SRS handle / another polynomial's
 * commitment -- an invalid proof that the verifier rejects, never an unsound one.  A service that must not even produce an
 * invalid proof for adversarial witnesses leaves the commitment cache off (the default) and registers its SRS from one
 * trusted source. */
int zk_srs_register(zk_ctx* ctx, int curve_id, const uint64_t* bases_xy, const uint8_t* inf_flags, size_t n, zk_srs** out);
int zk_srs_register_dev(zk_ctx* ctx, int curve_id, const void* d_bases_xy, const uint8_t* d_inf_flags, size_t n, zk_srs** out);
/* Optional: build the table of window multiples 2^(c w) * P_i (w = 1..W-1) for this SRS, W x its
 * size in HBM (1.9 GiB per 2^20 BLS12-381 points; the card has 288 GB).  MSMs over the SRS then use a
 * single bucket set: no per-window reduction and no host-side doublings.  Results are unchanged.  Idempotent.
 * Default window: c = 16 (16 rows) below 2^19 points, c = 17 from there on -- 15 rows for the 255-bit scalars of BLS12-381,
 * because a scalar k > (r - 1) / 2 is treated as -(r - k): one mixed addition per scalar fewer, 2^16 buckets instead of 2^15;
 * from 2^22 points on, c = 20 (13 rows, 2^19 buckets): two more additions per scalar saved outweigh the wider bucket reduction there
 * (the device-resident exchange below -- zk_kzg_round_end_winsums_dev -- needs window_bits <= 17: for an SRS or shard of 2^22 points
 * and more that is meant for it, call zk_srs_precompute_ex(ctx, srs, 17) instead; on a 20-bit table those calls return
 * ZK_ERR_UNSUPPORTED before anything is queued and the host form closes the round). */
int zk_srs_precompute(zk_ctx* ctx, zk_srs* srs);
/* Same with the table's window c chosen: 16 (default; 16 rows, 2^15 shared buckets) .. 21.  A larger window means fewer
 * rows (15 at c = 17, 13 at c = 20: mixed additions per scalar, table rows) but 2^(c-1) buckets to reduce.
 * 0 = default, or whatever table the SRS already holds.  The table belongs to the SRS, and a content-addressed
 * zk_srs_register hands every caller that registers the same bytes the SAME handle: the first precompute wins.  A later call
 * with window_bits = 0 (zk_srs_precompute) is a no-op; one that names a different window returns ZK_ERR_UNSUPPORTED and changes
 * nothing -- read the window in use with zk_srs_table_info.  Results never depend on the window. */
int zk_srs_precompute_ex(zk_ctx* ctx, zk_srs* srs, uint32_t window_bits);
/* window_bits / windows (= rows = mixed additions per scalar) of the SRS's table; both 0 without a table. */
int zk_srs_table_info(zk_srs* srs, uint32_t* window_bits, uint32_t* windows);
/* Multi-GPU, sharded by WINDOWS (BASELINE.json north_star: "the MSM shards its windows/buckets across GPUs"; SURVEY.md 8e's
 * alternative): rank g of G registers the WHOLE SRS and builds only the table rows of the windows first_window, first_window +
 * window_stride, ... (g, g + G, ...: ceil((W - g) / G) of the W rows), i.e. about 1/G of the table.  Every MSM entry point over such
 * an SRS then returns the rank's PARTIAL sum_i sum_{w owned} d_{i,w} 2^(c w) P_i -- all N scalars, the owned digits only, the rank's
 * own bucket set -- and the ranks' partials add up to the MSM (zk_g1_sum_partials*, after the same all-gather as the point-sharded
 * form: zk_kzg_round_end_partial, or the window-sum form on the device).  A vector too short for the table path is computed whole by the owner of window 0 and is
 * the point at infinity on the other ranks.  (first_window, window_stride) = (0, 1) is zk_srs_precompute_ex.  The first precompute
 * of an SRS wins, as above; a later call must name the same rows.  The plain SRS stays resident next to the rows. */
int zk_srs_precompute_rows(zk_ctx* ctx, zk_srs* srs, uint32_t window_bits, uint32_t first_window, uint32_t window_stride);
/* first_window / window_stride / rows held (0 / 1 / windows for a whole table; rows = 0 without a table). */
int zk_srs_table_rows(zk_srs* srs, uint32_t* first_window, uint32_t* window_stride, uint32_t* rows);
/* One more owner of a live handle (a second zk_ctx / thread that keeps using the SRS on its own): pairs with one more
 * zk_srs_free.  ZK_ERR_BAD_ARG for a handle whose last reference is gone. */
int zk_srs_retain(zk_srs* srs);
void zk_srs_free(zk_srs* srs);
size_t zk_srs_len(const zk_srs* srs);
/* SRS cache: bytes of unreferenced entries kept resident (0 = free on last zk_srs_free) / counters. */
int zk_srs_cache_config(size_t max_idle_bytes);
int zk_srs_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* resident_bytes);

/* MSM over srs[base_offset .. base_offset+n) with host / device canonical scalars.
 * Sizes: the window-table path takes 2^13 <= n <= 2^26 points per MSM (a sorted reference holds 26 bits of point index); shorter and
 * longer vectors run the per-window path over the same SRS inside the same call (identical result, no table rows read), which
 * takes n * windows < 2^32 references: about 2^27 points at its 16-bit window.  Beyond that ZK_ERR_UNSUPPORTED (a 2^28-point SRS
 * is 24 GiB in the ABI form; the reference's largest bench is 2^18, benches/plonk.rs:95-103). */
int zk_msm_g1_srs(zk_ctx* ctx, zk_srs* srs, size_t base_offset, const uint64_t* scalars, size_t n,
                  uint64_t* out_xy, uint8_t* out_inf);
int zk_msm_g1_srs_dev(zk_ctx* ctx, zk_srs* srs, size_t base_offset, const void* d_scalars, size_t n,
                      uint64_t* out_xy, uint8_t* out_inf);
/* Multi-GPU leg: this rank's partial sum as a projective (X, Y, Z) Jacobian triple, 3L limbs,
 * Montgomery (Z = 0 for infinity) -- the 144-byte message all-gathered over RCCL. */
int zk_msm_g1_srs_partial_dev(zk_ctx* ctx, zk_srs* srs, size_t base_offset, const void* d_scalars, size_t n,
                              uint64_t* out_xyz);
/* Host: sum `count` Jacobian partials (count x 3L limbs) and normalise to affine. */
int zk_g1_sum_partials(int curve_id, const uint64_t* partials_xyz, size_t count, uint64_t* out_xy, uint8_t* out_inf);
/* Host: the all-gathered partials of one prover round, laid out [rank][job][3L]; job k's sum -> out_xy[k], out_inf[k]. */
int zk_g1_sum_partials_batch(int curve_id, const uint64_t* partials_xyz, size_t ranks, uint32_t n_jobs, uint64_t* out_xy,
                             uint8_t* out_inf);

/* ---- a6: KZG10 commit (PC::commit, prover.rs:213,289-291,312-317,361-363,387-389,459-469) ----- */
/* d_coeffs_mont: n Montgomery Fr coefficients on device.  into_repr + MSM over
 * srs[0..n) (leading zero coefficients contribute nothing, as kzg10::commit's stripping). */
int zk_kzg_commit_dev(zk_ctx* ctx, zk_srs* srs, const void* d_coeffs_mont, size_t n, uint64_t* out_xy, uint8_t* out_inf);
int zk_kzg_commit(zk_ctx* ctx, zk_srs* srs, const uint64_t* coeffs_mont, size_t n, uint64_t* out_xy, uint8_t* out_inf);
/* PC::commit(ck, polys, None) with the caller's host slices -- the call GpuKZG10::commit forwards its whole
 * `polys` iterator to (prover.rs:213 passes 4 polynomials, :579 and :606 seven; n_polys <= 16).  Polynomial k+1 is
 * uploaded while polynomial k's MSM runs; results equal n_polys calls of zk_kzg_commit. */
int zk_kzg_commit_batch(zk_ctx* ctx, zk_srs* srs, uint32_t n_polys, const uint64_t* const* coeffs_mont, const size_t* lens,
                        uint64_t* out_xy, uint8_t* out_inf);

/* N3: opt-in, per-ctx, content-addressed commitment cache.  The reference commits twelve polynomials
 * a second time in its last round (prover.rs:569-607: aw_polys / saw_polys repeat sigma_1..3, f, h_2, table, z, w_l,
 * w_r, w_4, h_1, z_2).  With the cache on, every zk_kzg_commit* / zk_kzg_*_batch* call that returns affine points
 * first computes a 256-bit digest of each coefficient vector on the device and serves (srs, input kind, length,
 * digest) hits from the cache: an unchanged Prover::prove runs 17 MSMs per proof instead of 29 (20 on the first: the
 * prover key's sigma commitments then stay cached across proofs); outputs identical unless two coefficient vectors collide under the
 * keyed digest (trust model: at zk_srs_register above; option "cache_verify").  capacity = entries kept (0 = leave unchanged; default
 * 64, least recently used dropped).  ZK_ERR_UNSUPPORTED: no operating-system entropy behind the digest key. */
int zk_ctx_set_commit_cache(zk_ctx* ctx, int enable, uint32_t capacity);
int zk_commit_cache_stats(zk_ctx* ctx, uint64_t* hits, uint64_t* misses, uint64_t* entries);

/* The commitments of one prover round (e.g. the 4 wire commits of prover.rs:213, the 7 + 7 of
 * prover.rs:569-607): n_polys (<= 16) device-resident coefficient vectors over one precomputed SRS.
 * Results are identical to n_polys calls of zk_kzg_commit_dev; the batch queues all device work back to
 * back and the host blocks once per result instead of once per call.
 * out_xy: n_polys x 2L limbs, out_inf: n_polys flags. */
int zk_kzg_commit_batch_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_polys, const void* const* d_coeffs_mont, const size_t* lens,
                            uint64_t* out_xy, uint8_t* out_inf);

/* Same with a per-job input kind: kinds[k] = 0 Montgomery coefficients (a commit), 1 canonical scalars
 * (e.g. an opening witness from zk_kzg_witness_dev).  kinds == NULL means all 0.  Lets the 16 independent
 * MSMs of the last prover round (7 commits + opening, 7 commits + opening; prover.rs:569-618) be one batch. */
int zk_kzg_round_batch_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens,
                           const uint8_t* kinds, uint64_t* out_xy, uint8_t* out_inf);

/* Multi-GPU form of the batch: this rank's Jacobian partials (n_polys x 3L limbs) over ITS shard of the
 * SRS, for coefficient slices that already are the rank's [lo, hi) ranges; one all-gather per round. */
int zk_kzg_commit_batch_partial_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_polys, const void* const* d_coeffs_mont,
                                    const size_t* lens, uint64_t* out_xyz);

/* zk_kzg_round_batch_dev for a sharded SRS: per-job input kinds as above, Jacobian partials out
 * (n_jobs x 3L limbs); the opening witnesses of prover.rs:582-618 are passed as this rank's slice. */
int zk_kzg_round_batch_partial_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens,
                                   const uint8_t* kinds, uint64_t* out_xyz);

/* Deferred form of zk_kzg_round_batch_dev: a round OPENED by one or more calls and CLOSED by one.
 * The reference issues commitments whose inputs do not depend on each other's results as separate blocking calls:
 * f | h_1 | h_2 (prover.rs:289-317: no challenge is drawn between them), z | z_2 (prover.rs:361-389: delta and epsilon are
 * drawn before z is committed), and the four calls of the last round (prover.rs:579-618: both opening challenges are drawn
 * with no transcript append in between).  Every blocking call pays the latency of the bucket reduction's dependent-addition
 * chains and a host round trip while the GPU idles.  zk_kzg_round_begin_dev queues sort + bucket accumulation of its jobs on
 * the ctx stream and returns; other work (the next polynomial's NTT) and further begins may follow; zk_kzg_round_end reduces
 * every queued job with ONE launch per reduction kernel, waits once, and returns all results in submission order (n_jobs must
 * equal the number of jobs begun, else ZK_ERR_BAD_ARG and the round stays open).  Results are identical to the blocking
 * calls.  At most 16 jobs per round, one SRS per round; the caller keeps the inputs and the SRS alive until the round ends.
 * While a round is open the blocking MSM / commit / open entry points of the same ctx return ZK_ERR_PENDING (NTTs and the
 * other device builders may run).  Jobs that do not take the window-table path (no table, fewer than 2^13 elements) and,
 * with the commitment cache on, all jobs are computed at begin.  zk_kzg_open_begin_dev is zk_kzg_open_dev as a job of the
 * round (witness polynomial built at once, its MSM deferred).  zk_kzg_round_end_partial returns Jacobian partials (n_jobs x
 * 3L limbs) for a sharded SRS; zk_kzg_round_abort drops an open round (waits for the queued kernels).
 * zk_kzg_round_reduce (optional) queues the round's reduction kernels and returns: the round takes no further jobs, and
 * zk_kzg_round_end then waits for those kernels only -- whatever the caller queues on the stream in between (transforms that
 * do not depend on this round's results: prover.rs would have the sigma ffts of permutation/mod.rs:671-674 behind f | h_1 |
 * h_2, the coset ffts of quotient_poly.rs:72-120 behind z | z_2) runs while the host combines the window sums, normalises
 * and hashes the results into the transcript, instead of the GPU idling through that. */
int zk_kzg_round_begin_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_jobs, const void* const* d_inputs, const size_t* lens,
                           const uint8_t* kinds);
int zk_kzg_open_begin_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_polys, const void* const* d_polys, const size_t* lens,
                          const uint64_t* z_mont, const uint64_t* challenge_mont);
int zk_kzg_round_reduce(zk_ctx* ctx);
int zk_kzg_round_end(zk_ctx* ctx, uint32_t n_jobs, uint64_t* out_xy, uint8_t* out_inf);
int zk_kzg_round_end_partial(zk_ctx* ctx, uint32_t n_jobs, uint64_t* out_xyz);
int zk_kzg_round_pending(zk_ctx* ctx, uint32_t* n_jobs);
int zk_kzg_round_abort(zk_ctx* ctx);
/* Memory of a deferred round (round 6).  Every queued table-path job lives in a buffer set of its own until the round closes --
 * 4 B per (scalar, window) for its sorted references plus the chunk-edge partials and bucket arrays: 71 MB per job at n = 2^20, 2.5 GB at
 * 2^25 -- and sets are kept for the next round.  A begin that finds no room on the device for another set (hipMemGetInfo
 * minus option "mem_reserve_mb", or hipMalloc failing) CLOSES THE JOBS QUEUED SO FAR -- sort, accumulation, reduction, host combine, the
 * points parked in call order -- and reuses their sets; the round stays open and zk_kzg_round_end* returns exactly the points it would
 * have returned.  ZK_ERR_OOM is left for a size whose blocking form does not fit either (the reference itself has no size limit but
 * the field's two-adicity: plonk-core/src/error.rs:14-21).  zk_round_mem_stats: early closes so far, bytes held by the buffer sets, and
 * the device's free / total memory as the budget sees it (any pointer may be NULL). */
int zk_round_mem_stats(zk_ctx* ctx, uint64_t* early_closes, uint64_t* set_bytes, uint64_t* device_free, uint64_t* device_total);
/* Since round 4 a begin queues only the digit kernel of its jobs -- the one kernel that reads the caller's vectors, so the inputs are
 * consumed in stream order at the call, as before -- and zk_kzg_round_reduce / _end queue the rest for ALL jobs of the round as one
 * launch per kernel: the sort's placement passes, ONE accumulation launch (msm_accumulate_batch), the reductions.
 *
 * The multi-GPU exchange without a host hop (the reference is a single process).  A job's result is
 *   sum_v S_v + B_v * sum_v v * T_v
 * over the 2 VW virtual-window sums S_v | T_v its last reduction kernel writes (VW = 64 by default: 128 points in the library's internal
 * XYZZ limb form, opaque, 32 KiB for BLS12-381; every rank runs this library), and that expression is LINEAR in them.
 * zk_kzg_round_reduce_winsums_dev / zk_kzg_round_end_winsums_dev close the round with those sums -- not their combination -- left ON THE
 * DEVICE at d_out + k * zk_winsums_dev_bytes(ctx, srs), k = submission order, written by the reduction kernel the single-GPU path ends
 * with: no further dependent launch.  d_out is typically the send buffer of the collective (ncclAllGather / torch
 * all_gather_into_tensor on the same stream).  Neither call waits: d_out, the inputs and the SRS stay valid until the stream has passed
 * this point (zk_g1_sum_winsums_dev waits for it).  zk_kzg_round_reduce_winsums_dev is zk_kzg_round_reduce for this form (work queued
 * after it runs behind the reductions); zk_kzg_round_end_winsums_dev closes the round (queues the reductions itself unless reduce ran;
 * d_out must then be the same buffer).  All-zero sums are the point at infinity (a rank with an empty shard); a job computed at
 * submission or parked by the memory budget enters as S_0 = its point.  The ranks all-gather the buffers and zk_g1_sum_winsums_dev adds
 * the ranks' sums element-wise (one kernel of n_jobs * 2 VW independent quads, ranks - 1 additions each), waits once, and leaves the
 * one combine + inversion per job to the ctx's host pool exactly as zk_kzg_round_end does.  Same results.
 * ZK_ERR_UNSUPPORTED (returned before anything is queued: the round stays open, close it with zk_kzg_round_end_partial): no table, a
 * table with window_bits >= 18 -- the DEFAULT of zk_srs_precompute for whole tables of 2^22 points and more: pass window_bits = 17 to
 * zk_srs_precompute_ex / _rows for an SRS meant for this exchange -- and the commitment cache.  Every rank must run the same
 * table window and the same "pre_vw" / "pre_logg" options: zk_winsums_geometry returns {window_bits, windows of a full-width scalar, VW,
 * buckets per virtual window} for the caller to compare across ranks once (the Python schedule all-gathers it at construction and
 * refuses a mismatch); zk_winsums_dev_bytes is 0 where the form does not exist.
 * (Round 4's other device form -- ONE point per job, formed by a further dependent launch: zk_kzg_round_end_partial_dev /
 * zk_g1_sum_partials_dev -- measured last of the three exchanges and was retired in round 6: profiles/design_history_msm.md.) */
size_t zk_winsums_dev_bytes(zk_ctx* ctx, zk_srs* srs);
int zk_winsums_geometry(zk_ctx* ctx, zk_srs* srs, uint32_t out[4]);
int zk_kzg_round_reduce_winsums_dev(zk_ctx* ctx, void* d_out);
int zk_kzg_round_end_winsums_dev(zk_ctx* ctx, uint32_t n_jobs, void* d_out);
int zk_g1_sum_winsums_dev(zk_ctx* ctx, zk_srs* srs, const void* d_all, size_t ranks, uint32_t n_jobs, uint64_t* out_xy, uint8_t* out_inf);

/* ---- a7: KZG10 open (PC::open, prover.rs:582-591,609-618) ------------------------------------- */
/* p = sum_k challenge^k * polys[k]; witness = (p - p(z)) / (X - z); returns commit(witness).
 * polys: n_polys device pointers to Montgomery coefficient vectors of lens[k] elements. */
int zk_kzg_open_dev(zk_ctx* ctx, zk_srs* srs, uint32_t n_polys, const void* const* d_polys, const size_t* lens,
                    const uint64_t* z_mont, const uint64_t* challenge_mont, uint64_t* out_xy, uint8_t* out_inf);

/* Same with the caller's host slices (n_polys <= 16), as PC::open receives them. */
int zk_kzg_open(zk_ctx* ctx, zk_srs* srs, uint32_t n_polys, const uint64_t* const* polys_mont, const size_t* lens,
                const uint64_t* z_mont, const uint64_t* challenge_mont, uint64_t* out_xy, uint8_t* out_inf);

/* Only the CPU-side part of PC::open: writes the witness polynomial's max(len)-1 coefficients as
 * canonical scalars into d_out (device, max(len) x 4 limbs) and their count into *out_len; the caller
 * runs the opening MSM itself (e.g. sharded over GPUs with zk_msm_g1_srs_partial_dev). */
int zk_kzg_witness_dev(zk_ctx* ctx, int curve_id, uint32_t n_polys, const void* const* d_polys, const size_t* lens,
                       const uint64_t* z_mont, const uint64_t* challenge_mont, void* d_out, size_t* out_len);

/* ---- the O(n) work of the prover's last round (linearisation_poly.rs:164-350), device-resident ------------------ */
/* `DensePolynomial::evaluate(&point)` for a batch: out[k] = polys[k](points[k]), k < n_polys <= 32, one launch pair for
 * the batch.  The reference evaluates 16 polynomials at z and 7 at z*omega per proof (linearisation_poly.rs:203-261: the
 * ProofEvaluations of proof.rs:41-103).  polys: device pointers to Montgomery coefficient vectors of lens[k] elements
 * (lens[k] == 0 -> 0); points_mont: n_polys x 4 limbs (host), reduced; out_mont: n_polys x 4 limbs (host), Montgomery,
 * reduced.  Blocks until the values are in out_mont. */
int zk_poly_evaluate_dev(zk_ctx* ctx, int curve_id, uint32_t n_polys, const void* const* d_polys, const size_t* lens,
                         const uint64_t* points_mont, uint64_t* out_mont);

/* out[i] = sum_k coeffs[k] * polys[k][i] for i < out_len (a polynomial shorter than out_len counts as zero-extended, a longer
 * one is cut): the scalar-times-polynomial sums the reference builds with `&poly * scalar` and `+` -- the linearisation
 * polynomial (linearisation_poly.rs:288-336 with widget/arithmetic.rs:66-82, permutation.rs:156-291, widget/lookup.rs:154-203,
 * widget/mod.rs:96-104; 19 terms), the compressed lookup columns (sum zeta^k col_k).  n_terms <= 32; coeffs_mont: n_terms x
 * 4 limbs (host), reduced (pass the negated scalar for a subtracted term); d_out: device, out_len x 4 limbs, Montgomery,
 * reduced; may alias one of the inputs.  Queued on the ctx stream (no host synchronisation). */
int zk_poly_lincomb_dev(zk_ctx* ctx, int curve_id, uint32_t n_terms, const void* const* d_polys, const size_t* lens,
                        const uint64_t* coeffs_mont, void* d_out, size_t out_len);

/* ---- round 2 of the prover (prover.rs:228-317): the lookup query column and the sorted table/query halves ------------ */
/* prover.rs:244-279: out[i] = w_l[i] + zeta w_r[i] + zeta^2 w_o[i] + zeta^3 w_4[i] (`MultiSet::compress` of the four query
 * columns, util.rs `lc`) where q_lookup[i] != 0, and d_table_compressed[0] -- the first row of the compressed table, the
 * reference's dummy value -- where q_lookup[i] == 0 or i >= q_len (the reference pads q_lookup with zeros to n).
 * All vectors device-resident Montgomery, n rows; the compressed table itself is zk_poly_lincomb_dev over the four table
 * columns with coefficients 1, zeta, zeta^2, zeta^3 (prover.rs:229-237). */
int zk_lookup_query_dev(zk_ctx* ctx, int curve_id, size_t n, const void* d_q_lookup, size_t q_len, const void* const d_wires[4],
                        const uint64_t* zeta_mont, const void* d_table_compressed, void* d_out);

/* `MultiSet::combine_split` (lookup/multiset.rs:131-176), t.combine_split(&f): the values of t and f grouped by value in the
 * order of first appearance in t, every group written half to d_h1 ("evens") and half to d_h2 ("odds"), the odd element of
 * odd-sized groups alternately to h1 / h2 starting with h1.  d_t: n_t (< 2^24) elements, d_f: n_f elements; d_h1 / d_h2: room for
 * (n_t + n_f + 1) / 2 elements each; *len_h1 / *len_h2 receive the lengths (they differ by at most one).
 * ZK_ERR_NOT_INDEXED when f holds a value t does not (Error::ElementNotIndexed; nothing is written).  Values are compared as
 * 32-byte strings: pass reduced elements, as everywhere.  Blocks once (16-byte read-back of the lengths and the error flag). */
int zk_lookup_combine_split_dev(zk_ctx* ctx, int curve_id, const void* d_t, size_t n_t, const void* d_f, size_t n_f, void* d_h1, void* d_h2,
                                size_t* len_h1, size_t* len_h2);

/* ---- N2: grand-product builders, feeding the iNTT on device ------------------------ */
/* Evaluations of the permutation polynomial z over the size-2^log_n domain, i.e. everything
 * `Permutation::compute_permutation_poly` (permutation/mod.rs:652-752) does before its `domain.ifft`:
 *   out[0] = 1,  out[i+1] = out[i] * prod_k (w_k[i] + beta*K_k*omega^i + gamma) / prod_k (w_k[i] + beta*sigma_k[i] + gamma),
 * K = (1, 7, 13, 17) (permutation/constants.rs:12-22), the (n+1)-th value dropped as the reference does.
 * d_wires[k], d_sigmas[k] (k = 0..3): n Montgomery Fr evaluations each (sigma_k = domain.fft(sigma poly k),
 * mod.rs:671-676); beta, gamma: Montgomery Fr, 4 limbs, host.  d_out: n elements, may alias an input.
 * last_mont (optional, host, 4 limbs): the dropped value -- 1 for a satisfied permutation.
 * ZK_ERR_NOT_INVERTIBLE if a denominator is zero (the reference panics there). */
int zk_perm_product_dev(zk_ctx* ctx, int curve_id, uint32_t log_n, const void* const* d_wires, const void* const* d_sigmas,
                        const uint64_t* beta_mont, const uint64_t* gamma_mont, void* d_out, uint64_t* last_mont);
/* Same for the lookup product z2 (`compute_lookup_permutation_poly` + `lookup_ratio`, mod.rs:754-822):
 *   ratio_i = (1+d)(e + f_i)(e(1+d) + t_i + d t_{i+1}) / ((e(1+d) + h1_i + d h2_i)(e(1+d) + h2_i + d h1_{i+1})),
 * indices cyclic; d = delta, e = epsilon.  n need not be a power of two. */
int zk_lookup_product_dev(zk_ctx* ctx, int curve_id, size_t n, const void* d_f, const void* d_t, const void* d_h1, const void* d_h2,
                          const uint64_t* delta_mont, const uint64_t* epsilon_mont, void* d_out, uint64_t* last_mont);

/* ---- N1: pointwise quotient over the 4n coset ------------------------------------- */
/* Everything `quotient_poly::compute` (proof_system/quotient_poly.rs:34-178) does between its coset FFTs and
 * its final coset_ifft: out[i] = (gate_constraints[i] + permutation[i] + lookup[i]) / v_h_coset_4n[i] with all
 * widgets (arithmetic, range, logic, fixed-base scalar mul, curve addition), the permutation argument and the
 * lookup argument.  Every pointer is a device vector of 4n Montgomery Fr evaluations over the coset
 * g*<omega_4n> (the output of zk_ntt_dev kind 2); the "next row" of the reference (index i+4 of vectors it
 * extends by e[0..4], quotient_poly.rs:75-118) is taken cyclically.  Challenges / coefficients: Montgomery Fr. */
typedef struct zk_quotient_args {
    const void *w_l, *w_r, *w_o, *w_4;    /* wire polynomials */
    const void *z, *z2;                    /* permutation and lookup grand products */
    const void *f, *table, *h1, *h2;       /* lookup: query, compressed table, sorted halves */
    const void *pi;                        /* public inputs */
    const void *l1;                        /* first Lagrange polynomial (quotient_poly.rs:68-69) */
    /* prover key evaluations (preprocess.rs:144-212) */
    const void *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *q_arith;
    const void *q_range, *q_logic, *q_fixed_group_add, *q_variable_group_add, *q_lookup;
    const void* sigma[4];                  /* left, right, out, fourth */
    uint64_t alpha[4], beta[4], gamma[4], delta[4], epsilon[4], zeta[4];
    uint64_t range_challenge[4], logic_challenge[4], fixed_base_challenge[4], var_base_challenge[4], lookup_challenge[4];
    uint64_t coeff_a[4], coeff_d[4];       /* P::COEFF_A, P::COEFF_D of the embedded twisted Edwards curve */
} zk_quotient_args;
/* n = 2^log_n is the circuit domain size; vectors hold 4n elements.  d_out (4n elements) must not alias an input. */
int zk_quotient_evals_dev(zk_ctx* ctx, int curve_id, uint32_t log_n, const zk_quotient_args* args, void* d_out);

/* ---- N4: canonical wire formats and the transcript (host only, no GPU needed) ------------------ */
/* ark-serialize 0.3 CanonicalSerialize, as the reference applies it in transcript.rs:27-33 (`append`) and through the
 * derives on proof.rs:41-103 / linearisation_poly.rs:34-161 / widget/mod.rs:252-278:
 *   Fr        : zk_fr_serialized_size bytes (32), little-endian canonical (non-Montgomery) integer.
 *   G1Affine  : compressed = x as little-endian canonical integer in zk_g1_compressed_size bytes (48 BLS12-381,
 *               32 BN254) with SWFlags in the top bits of the LAST byte: 0x80 = y is the larger of (y, p - y),
 *               0x40 = infinity (x = 0).  Uncompressed = x then y (2 x that size), the infinity flag on y.
 * Deserialisation validates like ark: integer < modulus, point on the curve and in the prime-order subgroup, flag
 * combinations; any violation is ZK_ERR_BAD_ARG.  Field elements cross this API in Montgomery form as everywhere. */
size_t zk_fr_serialized_size(int curve_id);
size_t zk_g1_compressed_size(int curve_id);
int zk_fr_serialize(int curve_id, const uint64_t* fr_mont, uint8_t* out);
int zk_fr_deserialize(int curve_id, const uint8_t* in, uint64_t* fr_mont);
int zk_g1_serialize_compressed(int curve_id, const uint64_t* xy_mont, uint8_t inf, uint8_t* out);
int zk_g1_deserialize_compressed(int curve_id, const uint8_t* in, uint64_t* xy_mont, uint8_t* inf);
int zk_g1_serialize_uncompressed(int curve_id, const uint64_t* xy_mont, uint8_t inf, uint8_t* out);
int zk_g1_deserialize_uncompressed(int curve_id, const uint8_t* in, uint64_t* xy_mont, uint8_t* inf);

/* merlin 3.0 `Transcript` (STROBE-128 / Keccak-f[1600]) -- prover.rs:179 clones one and drives it through the proof. */
typedef struct zk_transcript zk_transcript;
zk_transcript* zk_transcript_new(const uint8_t* label, size_t label_len);            /* Transcript::new(label)   */
zk_transcript* zk_transcript_clone(const zk_transcript* t);                          /* prover.rs:179            */
void zk_transcript_free(zk_transcript* t);
int zk_transcript_append_message(zk_transcript* t, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len);
int zk_transcript_append_u64(zk_transcript* t, const uint8_t* label, size_t label_len, uint64_t v);
int zk_transcript_challenge_bytes(zk_transcript* t, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len);
/* plonk-core's TranscriptProtocol (transcript.rs:16-49): append(label, item) for the two item types the prover appends
 * (a commitment = compressed G1, prover.rs:217-220,294,320-321,366,472-475; a scalar, prover.rs:226,327-337,399-426,481,
 * 516-553), challenge_scalar (31 challenge bytes as a little-endian integer, transcript.rs:35-46) and
 * circuit_domain_sep (transcript.rs:45-48).  The order of labels over one proof is tabulated in INTEGRATION.md section 7
 * and replayed by ark_plonk_amd/transcript.py::ProverTranscript. */
int zk_transcript_append_fr(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* fr_mont);
int zk_transcript_append_g1(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* xy_mont, uint8_t inf);
int zk_transcript_challenge_scalar(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, uint64_t* fr_mont);
int zk_transcript_circuit_domain_sep(zk_transcript* t, uint64_t n);
/* prover.rs:182 `transcript.append(b"pi", self.cs.get_pi())`: PublicInputs = BTreeMap<usize, F> (pi.rs:28-36), i.e. u64 count,
 * then (u64 position, Fr) with strictly ascending positions (anything else is ZK_ERR_BAD_ARG). */
int zk_transcript_append_public_inputs(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* positions,
                                       const uint64_t* values_mont, size_t n);

/* `Proof<F, PC>` for PC = (Sonic)KZG10 (proof.rs:41-103): the serialised form is the fields in declaration order --
 * 13 commitments a b c d z f h_1 h_2 z_2 t_1 t_2 t_3 t_4 (compressed G1 each), aw_opening and saw_opening
 * (kzg10::Proof { w, random_v: None } = compressed G1 + one 0 byte), then ProofEvaluations (linearisation_poly.rs:34-161):
 * a b c d | left_sigma right_sigma out_sigma permutation | q_lookup z2_next h1 h1_next h2 f table table_next as Fr,
 * then custom_evals: u64 count, and per entry u64 label length + label bytes + Fr. */
#define ZK_PROOF_N_EVALS 16
typedef struct zk_proof {
    const uint64_t* commitments;     /* 13 x 2L limbs, Montgomery affine, the order above */
    const uint8_t* commitment_inf;   /* 13 flags */
    const uint64_t* openings;        /* 2 x 2L limbs: aw_opening.w, saw_opening.w */
    const uint8_t* opening_inf;      /* 2 flags */
    const uint64_t* evals;           /* ZK_PROOF_N_EVALS x 4 limbs, Montgomery, the order above */
    uint32_t n_custom_evals;
    const char* const* custom_labels; /* NUL-terminated */
    const uint64_t* custom_evals;    /* n_custom_evals x 4 limbs */
} zk_proof;
size_t zk_proof_serialized_size(int curve_id, uint32_t n_custom_evals, const uint32_t* label_lens);
int zk_proof_serialize(int curve_id, const zk_proof* proof, uint8_t* out, size_t cap, size_t* written);

/* ---- batch verification, the stages in front of the two pairing inputs ----------------------------------------- */
/* Stage 1, general (not tied to proofs): n compressed G1 encodings in device memory -> affine Montgomery points in the layout
 * zk_srs_register_dev takes (2L limbs each), one infinity flag and one status byte per point.  The rules are those of
 * zk_g1_deserialize_compressed (ark's GroupAffine::deserialize); where that returns ZK_ERR_BAD_ARG this reports which rule failed,
 * in the order they are applied.  Infinity is written as (0, 1) with flag 1; a rejected encoding as all-zero words, flag 0.
 * One lane per point, queued on the ctx stream, no working memory. */
#define ZK_G1_OK 0
#define ZK_G1_BAD_FLAGS 1        /* both flag bits set */
#define ZK_G1_X_NOT_REDUCED 2    /* x >= q (checked before the infinity flag is honoured, as ark does) */
#define ZK_G1_NOT_ON_CURVE 3     /* x^3 + b is no square */
#define ZK_G1_NOT_IN_SUBGROUP 4  /* r * P != O */
int zk_g1_decompress_batch_dev(zk_ctx* ctx, int curve_id, const void* d_in, size_t n, void* d_out_xy, void* d_out_inf, void* d_status);

/* Stage 2, host only: parse n_proofs serialised proofs (the layout of zk_proof above) and replay the verifier's transcript traffic
 * (proof.rs:128-300, 343-378) for each on a copy of `seeded` -- the transcript after VerifierKey::seed_transcript -- which is left
 * untouched.  Proof j has the public inputs pi_positions / pi_values_mont [pi_offsets[j], pi_offsets[j + 1]) (strictly ascending
 * positions; zero values are not part of the message, as in zk_transcript_append_public_inputs).
 *   out_challenges_mont  n_proofs x ZK_VERIFY_N_CHALLENGES x 4 limbs: zeta beta gamma delta epsilon alpha range logic fixed var lookup
 *                        z aw saw
 *   out_evals_mont       n_proofs x ZK_VERIFY_N_EVALS x 4 limbs: the 16 evaluations in the proof's order, then a_next b_next d_next
 *                        q_arith q_c q_l q_r (found by label among the custom evaluations; a repeated label: the last one)
 *   out_points           optional, n_proofs x 15 compressed encodings (13 commitments, aw and saw opening): the input of stage 1
 *   out_status           one ZK_PROOF_* per proof; a rejected proof has all-zero rows and infinity encodings
 * The transcript takes a commitment's own bytes (an infinity-flagged one in canonical form, as ark re-serialises it), so the replay
 * does not wait for the points to be decoded: whether they decode is stage 1's status.  Malformed bytes are a status, never a
 * return code: ZK_ERR_BAD_ARG is for null arguments, an unknown curve and descending pi_offsets. */
#define ZK_VERIFY_N_CHALLENGES 14
#define ZK_VERIFY_N_EVALS 23
#define ZK_PROOF_OK 0
#define ZK_PROOF_TRUNCATED 1          /* the bytes end inside a field */
#define ZK_PROOF_TRAILING 2           /* bytes are left after the last custom evaluation */
#define ZK_PROOF_BAD_OPTION 3         /* an opening's random_v is not None */
#define ZK_PROOF_FR_NOT_REDUCED 4     /* an evaluation >= r */
#define ZK_PROOF_MISSING_LABEL 5      /* one of the seven custom evaluations the verifier reads is absent */
#define ZK_PROOF_BAD_COUNT 6          /* the custom-evaluation count names more entries than the bytes hold */
#define ZK_PROOF_BAD_PUBLIC_INPUTS 7  /* positions not strictly ascending */
int zk_proof_replay_batch(const zk_transcript* seeded, int curve_id, size_t n_proofs, const uint8_t* const* proofs, const size_t* proof_lens,
                          const uint64_t* pi_offsets, const uint64_t* pi_positions, const uint64_t* pi_values_mont, uint64_t* out_challenges_mont,
                          uint64_t* out_evals_mont, uint8_t* out_points, uint8_t* out_status);
/* Stage 2 on the device: the same parse and replay, one proof per lane (64 per workgroup), every array in device memory.  The proofs
 * are one byte string d_proofs of proofs_bytes bytes, proof j being [d_proof_offsets[j], d_proof_offsets[j + 1]) of it (n_proofs + 1
 * uint64); the public inputs are the three arrays of zk_proof_replay_batch with n_pi_total entries behind d_pi_offsets.  The four
 * outputs have exactly the layout and content zk_proof_replay_batch writes (d_out_points may be NULL), so stages 1 and 3 take them where
 * they are.  `seeded` is a host handle, read when the call is made and left untouched.  Queued on the ctx stream, no working memory.
 * The offsets are data the host does not see, so where zk_proof_replay_batch returns ZK_ERR_BAD_ARG for them this call reports a
 * status and reads nothing outside the buffers: a proof range that descends or ends beyond proofs_bytes is ZK_PROOF_TRUNCATED; a
 * public-input range that descends or ends beyond n_pi_total is ZK_PROOF_BAD_PUBLIC_INPUTS (reported for a proof whose bytes parse: a
 * malformed proof keeps the status of its bytes).  ZK_ERR_BAD_ARG: a null ctx or `seeded`, an unknown curve, a null array with
 * n_proofs > 0 (the two public-input arrays only when n_pi_total > 0).  n_proofs == 0 is ZK_OK; n_proofs >= 2^31 ZK_ERR_UNSUPPORTED. */
int zk_proof_replay_batch_dev(zk_ctx* ctx, const zk_transcript* seeded, int curve_id, size_t n_proofs, const void* d_proofs, size_t proofs_bytes,
                              const void* d_proof_offsets, const void* d_pi_offsets, const void* d_pi_positions, const void* d_pi_values_mont,
                              size_t n_pi_total, void* d_out_challenges_mont, void* d_out_evals_mont, void* d_out_points, void* d_out_status);

/* Stage 3: the scalars of every proof's share of the two pairing inputs.  With u, u' the proof's two weights (d_weights: n_proofs x 2
 * canonical scalars), chi / chi' the aw / saw challenges and (C_k, v_k) the pairs of the two openings as Proof::verify forms them
 * (proof.rs:303-395: C_0 the linearisation commitment of :488-611, v_0 = -r_0 of :427-486),
 *   R_j = u (sum_k chi^k (C_k - v_k G) + z W_aw) + u' (sum_k chi'^k (C'_k - v'_k G) + z w W_saw),   L_j = u W_aw + u' W_saw,
 * expanded over the bases:
 *   d_key_rows    n_proofs x ZK_VERIFY_N_KEY_BASES: q_m q_l q_r q_o q_4 q_c q_range q_logic q_fixed_group_add q_variable_group_add
 *                 q_lookup | left right out fourth sigma | table_1..4 | G
 *   d_proof_rows  n_proofs x ZK_VERIFY_N_PROOF_BASES: the 13 commitments in the proof's order, aw_opening, saw_opening
 *   d_open_rows   n_proofs x 2: u, u' (the scalars of L over aw_opening, saw_opening)
 * all canonical (the form the MSM entry points take).  Inputs: the rows zk_proof_replay_batch wrote, copied to the device, the public
 * inputs in the same three arrays, the embedded curve's coefficients (host, 4 limbs each), and the statuses of stages 2 (one per proof;
 * may be NULL) and 1 (ZK_VERIFY_N_PROOF_BASES per proof; may be NULL).  d_status: one byte per proof -- 0, the stage-2 status, ZK_VERIFY_BAD_POINT + the
 * stage-1 status of its first rejected point, or ZK_VERIFY_Z_ON_DOMAIN (z = w^pos for a public input's position or z = 1: the
 * barycentric form has no value there).  Every row of a proof with a non-zero status is zero, so it drops out of any sum over the
 * batch.  One 64-lane workgroup per proof striding over its public inputs; one field inversion per 64 denominators.  Queued on the
 * ctx stream, no working memory.  ZK_ERR_DOMAIN_TOO_LARGE: log_n beyond the field's two-adicity. */
#define ZK_VERIFY_N_KEY_BASES 20
#define ZK_VERIFY_N_PROOF_BASES 15
#define ZK_VERIFY_OK 0
#define ZK_VERIFY_BAD_POINT 16
#define ZK_VERIFY_Z_ON_DOMAIN 32
int zk_verify_scalars_dev(zk_ctx* ctx, int curve_id, uint32_t log_n, size_t n_proofs, const void* d_challenges_mont, const void* d_evals_mont,
                          const void* d_pi_offsets, const void* d_pi_positions, const void* d_pi_values_mont, const uint64_t* coeff_a_mont,
                          const uint64_t* coeff_d_mont, const void* d_weights, const void* d_parse_status, const void* d_point_status,
                          void* d_key_rows, void* d_proof_rows, void* d_open_rows, void* d_status);
/* Stage 4's one kernel: d_out[c] = sum_r d_rows[r][c] over n_rows rows of n_cols Fr each (either form: a sum does not care), e.g. the
 * key-scalar rows of a range [lo, hi) of the batch -> 20 scalars.  The fold itself is the existing MSM over the decoded points
 * registered with zk_srs_register_dev (proof-major: base_offset = 15 lo, n = 15 (hi - lo)) and zk_g1_sum_partials. */
int zk_fr_column_sum_dev(zk_ctx* ctx, int curve_id, const void* d_rows, size_t n_rows, uint32_t n_cols, void* d_out);

/* ---- segmented MSM: many small MSMs, each as a point ------------------------------------------------------------- */
/* n_seg independent small MSMs over one set of bases: out[s] = sum over t in [off[s], off[s+1]) of scalar[t] * base[index[t]] -- the
 * batched form of HomomorphicCommitment::multi_scalar_mul (commitment.rs:8-91) and of the combined commitments an IPA check hashes.
 * d_bases_xy / d_bases_inf: n_bases affine Montgomery points and flags in the layout zk_srs_register_dev takes and
 * zk_g1_decompress_batch_dev writes (d_bases_inf may be NULL).  d_seg_offsets: n_seg + 1 uint64; d_base_index: n_terms uint32;
 * d_scalars: n_terms x 4 limbs, plain 256-bit integers (canonical Fr is the normal case; no reduction test: s * P is the
 * integer multiple).  d_out_xy / d_out_inf: n_seg affine Montgomery points, infinity written as (0, 1) with flag 1.
 * d_status: one byte per segment.  A term with a zero scalar or an infinity-flagged base contributes nothing and its coordinates are
 * not used (a base of all-zero words, what a rejected decoding leaves, contributes nothing either); other points are taken to be on the
 * curve.  A segment with a non-zero status yields infinity; an empty one yields infinity with ZK_SEG_OK.  Offsets and indices are data on
 * the device: a bad one is a status, never a fault, and nothing outside the buffers is read.  ZK_ERR_BAD_ARG: a null ctx, an unknown
 * curve, a null array with n_seg > 0 (the two term arrays only when n_terms > 0, the bases only when n_bases > 0); n_seg == 0 is ZK_OK;
 * n_seg > 2^31 ZK_ERR_UNSUPPORTED.  One 64-lane wavefront per segment, one double-and-add per term, the lane sums added in LDS with the
 * group law's full addition, one field inversion per workgroup of four segments.  Queued on the ctx stream, no working memory. */
#define ZK_SEG_OK 0
#define ZK_SEG_BAD_RANGE 1   /* offsets descend or end beyond n_terms: nothing of the segment is read */
#define ZK_SEG_BAD_INDEX 2   /* a term names a base >= n_bases: no base is read for it */
int zk_msm_g1_segments_dev(zk_ctx* ctx, int curve_id, size_t n_bases, const void* d_bases_xy, const void* d_bases_inf, size_t n_seg,
                           const void* d_seg_offsets, size_t n_terms, const void* d_base_index, const void* d_scalars,
                           void* d_out_xy, void* d_out_inf, void* d_status);

/* ---- inner-product-argument commitment (IPA) -------------------------------------------------------------------------------- */
/* The reference's second HomomorphicCommitment (plonk-core/src/commitment.rs:50-91: ark-poly-commit 0.3 ipa_pc::InnerProductArgPC),
 * without hiding and degree bounds, as ark-plonk uses it (prover.rs:582-618).  The committer key is a zk_srs of d1 = d + 1 = 2^k
 * points (comm_key; zk_ipa_* refuse another length with ZK_ERR_BAD_ARG); commit and the verifier's final-key MSM are the zk_msm_g1_srs*
 * calls over it.  An opening is driven round by round by the caller, who derives every challenge (the transcript is not part of this
 * ABI): for m = d1/2, d1/4, ..., 1
 *     zk_ipa_round_dev(first_round = (m == d1/2), m)  -> L, R      then    zk_ipa_fold_dev(first_round, m, xi)
 * The state lives in the caller's device buffers: a (the combined polynomial's Montgomery coefficients, zero-padded to d1), b (the
 * powers of the point, zk_ipa_powers_dev) and a workspace of zk_ipa_workspace_bytes (the folded key in the MSM's internal base layout,
 * the canonical copy of a the round MSMs read, the inner-product partial sums the fold leaves for the next round): a round that is not
 * the first reads what the fold before it left there.  Between these calls any other call on the ctx is allowed.  While a deferred KZG
 * round is open on the ctx (zk_kzg_round_pending) zk_ipa_round_dev -- which runs MSMs -- returns ZK_ERR_PENDING. */
/* device bytes one opening over d1 = 2^k points needs (0 for an unknown curve or a d1 that is not a power of two) */
size_t zk_ipa_workspace_bytes(int curve_id, size_t d1);
/* d_out[i] = point^i, i < n (Montgomery Fr, device); 0^0 = 1.  n = 0 writes nothing (d_out may be NULL); a point that is not below r
 * is ZK_ERR_BAD_ARG and writes nothing. */
int zk_ipa_powers_dev(zk_ctx* ctx, int curve_id, const uint64_t* point_mont, size_t n, void* d_out);
/* One round on vectors of length 2m: L = MSM(key_l, a_r) + <a_r, b_l> h', R = MSM(key_r, a_l) + <a_l, b_r> h', affine Montgomery
 * (out_lr_xy: L then R, 2 x 2L limbs; out_lr_inf: 2 flags, may be NULL).  The key is key[0 .. 2m) in the first round (the SRS
 * table path) and the folded key in d_work afterwards (first_round = 0: 2m <= d1 / 2).  h_prime_xy: affine Montgomery (2L limbs);
 * x = 0 with y = 0 (all-zero words) or y = 1 is the point at infinity, and the inner products then carry no weight.  An output at
 * infinity is written as the words of (0, 1), with or without out_lr_inf.  A first round may cover fewer points than the key holds
 * (2m < d1, a power of two): it and the folds after it read key[0 .. 2m) alone, in a workspace still sized for d1.  A key with a
 * window-sharded table (zk_srs_precompute_rows) is ZK_ERR_UNSUPPORTED in the first round; a, b and the key are left as they were. */
int zk_ipa_round_dev(zk_ctx* ctx, zk_srs* key, int first_round, size_t m, const void* d_a, const void* d_b, void* d_work,
                     const uint64_t* h_prime_xy, uint64_t* out_lr_xy, uint8_t* out_lr_inf);
/* a <- a_l + xi^-1 a_r, b <- b_l + xi b_r (in place, to length m); key <- key_l + xi key_r into d_work.  xi: Montgomery, non-zero.
 * A refused call (xi = 0, or words that are not below r: ZK_ERR_BAD_ARG) queues nothing: a, b, the folded key and the next round's
 * L and R are what they were.  A key point sent to infinity by the challenge (key_l[i] = -xi key_r[i]) is a null point of the folded
 * key, which the rounds and folds after it -- and zk_ipa_final_key_dev, as (0, 1) with flag 1 -- carry like any other.
 * Queued on the ctx stream. */
int zk_ipa_fold_dev(zk_ctx* ctx, zk_srs* key, int first_round, size_t m, const uint64_t* xi_mont, void* d_a, void* d_b, void* d_work);
/* after the last fold: final_comm_key = the one folded point in d_work (affine Montgomery); the caller reads c = a[0] itself */
int zk_ipa_final_key_dev(zk_ctx* ctx, int curve_id, const void* d_work, uint64_t* out_xy, uint8_t* out_inf);
/* one key fold on its own: out[i] = key[i] + xi key[i + m], i < m; ABI affine layout in and out (d_key_inf, d_out_inf: device flags,
 * may be NULL).  Blocks until the result is written. */
int zk_ipa_fold_key_dev(zk_ctx* ctx, int curve_id, size_t m, const void* d_key_xy, const uint8_t* d_key_inf, const uint64_t* xi_mont,
                        void* d_out_xy, uint8_t* d_out_inf);
/* s_k of the check polynomial s(X) = prod_j (1 + xi_j X^(2^(log_d - 1 - j))), k < 2^log_d: canonical Fr on the device, the scalars of
 * the verifier's final-key MSM (xis_mont: log_d Montgomery challenges, xi_0 first; log_d <= 32) */
int zk_ipa_check_coeffs_dev(zk_ctx* ctx, int curve_id, uint32_t log_d, const uint64_t* xis_mont, void* d_out);
/* The check vectors of n_open openings combined under weights, the scalars of ONE final-key MSM for the batch:
 *     d_out[i] = sum_j w_j prod_k xi_{j,k}^(bit (log_d - 1 - k) of i) mod r,   i < 2^log_d, canonical Fr
 * (the bit convention of zk_ipa_check_coeffs_dev: with n_open = 1 and w = 1 the two outputs are the same bytes).  d_xis_mont: n_open x
 * log_d Montgomery challenges, opening-major, xi_{j,0} first; d_weights_mont: n_open Montgomery weights; both on the device.  n_open = 0
 * writes zeros; log_d = 0 writes the sum of the weights; log_d <= 32, n_open <= 2^30.  A challenge or a weight that is not below r is
 * found on the device: ZK_ERR_BAD_ARG (d_out is then unspecified).  d_work: zk_ipa_check_combine_workspace_bytes(curve_id, log_d,
 * n_open) device bytes -- two tables per opening, of 2^ceil(log_d / 2) and 2^floor(log_d / 2) elements; the openings are not chunked and
 * the size is not capped (0 for an unknown curve or arguments out of range).  The call runs no MSM and is legal while a deferred KZG
 * round is open; it blocks until the device has answered. */
size_t zk_ipa_check_combine_workspace_bytes(int curve_id, uint32_t log_d, size_t n_open);
int zk_ipa_check_combine_dev(zk_ctx* ctx, int curve_id, uint32_t log_d, size_t n_open, const void* d_xis_mont, const void* d_weights_mont,
                             void* d_work, void* d_out);

/* ---- IPA key derivation: ipa_pc::setup's generators ---------------------------------------------------------- */
/* ark-poly-commit 0.3 `InnerProductArgPC::sample_generators`, AS RECALLED (the crate is not vendored; the encodings are stated once
 * for the device in csrc/h2c.cuh and once for the host in ark_plonk_amd/ipa.py, unpinned against the crate like the IPA transcript):
 * generator i is affine(cofactor * P) for the first P = from_random_bytes(D("PC-DL-2020" || u64_le(i) [|| u64_le(j)])) that is a
 * point, attempt 1 without j, attempt a >= 2 with j = a - 2.  D is unkeyed Blake2s-256 or Blake2b-512.  setup(max_degree) takes
 * d + 3 generators for d = next_power_of_two(max_degree + 1) - 1: comm_key = [0, d], s = d + 1, h = d + 2.
 *
 * zk_ipa_sample_generators_dev writes generators first_index .. first_index + n (ranks or chunks may each derive a range) in the
 * layout zk_srs_register_dev takes: d_out_xy n x 2L limbs affine Montgomery, d_out_inf n flags, d_status n bytes.  max_tries caps
 * the attempts per index (0: 1024; the worst per-attempt success probability is about 0.175, so 1024 fail with probability below
 * 1e-80): an index that runs out has status ZK_H2C_EXHAUSTED and an all-zero row, and is never a hang.  d_tries (optional, n uint32):
 * the attempts made.  d_wave_rounds (optional, zk_ipa_sample_generators_waves(n) uint32): the square-root rounds each wavefront ran,
 * a wavefront owning ZK_H2C_CHUNK consecutive indices.  n = 0 is a no-op.  Queued on the ctx stream, no working memory. */
#define ZK_H2C_BLAKE2S 0
#define ZK_H2C_BLAKE2B 1
#define ZK_H2C_CHUNK 512
#define ZK_G1_INF_FLAG_X_NONZERO 5  /* from_random_bytes: the infinity flag on an x that is not 0 */
#define ZK_H2C_EXHAUSTED 6          /* max_tries attempts and no point */
size_t zk_ipa_sample_generators_waves(size_t n);
int zk_ipa_sample_generators_dev(zk_ctx* ctx, int curve_id, int digest_id, uint64_t first_index, size_t n, uint32_t max_tries, void* d_out_xy,
                                 void* d_out_inf, void* d_tries, void* d_status, void* d_wave_rounds);
/* `GroupAffine::from_random_bytes` (over Fp::from_random_bytes_with_flags::<SWFlags>) of n strings of byte_len >= 0 bytes each, one
 * lane per string: min(byte_len, G) bytes into a zeroed buffer of G = zk_g1_compressed_size bytes; flags in the top two bits of byte
 * G - 1; x with every bit from MODULUS_BITS up cleared.  Status per string, in the order the rules apply: ZK_G1_X_NOT_REDUCED,
 * ZK_G1_BAD_FLAGS, ZK_G1_INF_FLAG_X_NONZERO (the flag with x = 0 is infinity, ZK_G1_OK), ZK_G1_NOT_ON_CURVE.  No subgroup check.
 * clear_cofactor != 0 multiplies every point by the cofactor of G1 (a point of the cofactor's torsion becomes infinity).  Rows as
 * zk_g1_decompress_batch_dev writes them: infinity (0, 1) with flag 1, a rejected string all-zero words. */
int zk_g1_from_random_bytes_batch_dev(zk_ctx* ctx, int curve_id, const void* d_bytes, size_t byte_len, size_t n, int clear_cofactor,
                                      void* d_out_xy, void* d_out_inf, void* d_status);

/* ---- circuit compilation (Circuit::compile, circuit.rs:226-259 -> preprocess.rs:126-423) ------------------------------------- */
/* The wire permutation: `Permutation::compute_sigma_permutations` + `compute_permutation_lagrange` (permutation/mod.rs:101-169).
 * n = 2^log_n.  A position is wire * n + row, wire 0..3 = Left, Right, Output, Fourth.  d_ins_var[k], d_ins_pos[k] (u32, device,
 * k < m <= 4n) are the k-th call of `add_variable_to_map(var, wire_data)` IN CALL ORDER (which is not row order: logic.rs:212-218
 * inserts Output(n - 1) after Left(n)); rows the composer pads and cells it never maps are not in the list.
 * For every variable with positions p_0 .. p_{c-1} in call order: sigma(p_i) = p_{(i+1) mod c}; a position never inserted maps to
 * itself.  d_sigma_pos (u32[4n] or NULL) receives sigma; d_sigma_evals (4 device pointers of n Montgomery Fr each, or NULL)
 * receive d_sigma_evals[w][row] = K_w' * omega^row' for sigma(w n + row) = w' n + row', K = (1, 7, 13, 17), omega the group_gen
 * zk_domain_new reports for n.  At least one of the two outputs is required.  The result is a pure function of the inputs.
 * ZK_ERR_BAD_ARG: m > 4n, a position >= 4n, a variable >= num_vars, a position inserted twice (found on the device, reported by one
 * flag word read back at the end; the outputs are then unspecified); ZK_ERR_DOMAIN_TOO_LARGE: log_n beyond the two-adicity;
 * ZK_ERR_UNSUPPORTED: log_n > 28 (positions are 32-bit).  m = 0 gives the identity.
 * Working memory: one device allocation per call, freed before return -- at most 16 m + m / 4 + 2 KiB bytes, + 16 n when
 * d_sigma_pos is NULL (<= 81 n bytes).  No buffer of the ctx is used: the call runs inside an open deferred round.  Blocks once. */
int zk_perm_sigma_dev(zk_ctx* ctx, int curve_id, uint32_t log_n, const void* d_ins_var, const void* d_ins_pos, size_t m, uint32_t num_vars,
                      void* d_sigma_pos, void* const* d_sigma_evals);
/* `to_scalars` (prover.rs:188-192): d_out[i] = d_values[d_index[i]], i < n; 32-byte elements, d_index u32 on the device.
 * ZK_ERR_BAD_ARG when an index is >= num_values (same flag mechanism; nothing is read out of range).  Uses no buffer of the ctx
 * (runs inside an open deferred round).  Blocks once. */
int zk_fr_gather_dev(zk_ctx* ctx, int curve_id, const void* d_values, size_t num_values, const void* d_index, size_t n, void* d_out);

/* ---- circuit check: which rows does a witness violate? ------------------------------------------------------------------------- */
/* The reference's `StandardComposer::check_circuit_satisfied` (constraint_system/composer.rs:661-814, feature `trace`) walks the gates
 * on the host and stops at the first failing one; it covers arithmetic, logic and range.  Here every row of the padded circuit is
 * tested on the device, BEFORE a proof is computed, against the summands of the identities the quotient enforces, one by one and with
 * no random challenge.  d_mask[i] (u32, n = 2^log_n rows) gets one bit per violated constraint of row i:
 *   bit 0       arith      q_arith (q_m ab + q_l a + q_r b + q_o c + q_4 d + q_c) + pi[i] != 0          (arithmetic.rs:51-63)
 *   bits 1-4    range0-3   q_range != 0 and delta(c-4d), delta(b-4c), delta(a-4b), delta(d_n-4a) != 0  (range.rs:47-63)
 *   bits 5-9    logic0-4   q_logic != 0 and delta(la), delta(lb), delta(ld), c - la lb,
 *                          q_c (9 ld - 3 (la+lb)) + 3 (la+lb+ld) - 2 F != 0                            (logic.rs:65-133)
 *   bits 10-13  fixed0-3   q_fixed_group_add != 0 and bit (bit-1) (bit+1), bit q_c - c, the x and the y equation of the step
 *                                                                                     (ecc/fixed_base_scalar_mul.rs:88-156)
 *   bits 14-16  curve0-2   q_variable_group_add != 0 and a d - d_n, the x and the y equation of the sum (ecc/curve_addition.rs:62-97)
 *   bit 17      lookup     q_lookup != 0 and (a, b, c, d) equals no row of the table (all four columns compared in full; a table of
 *                          0 rows fails every such row)
 *   bits 18-21  copy_l/r/o/4   the cell (wire k, row i) and the cell sigma[k][i] points to hold different values
 * a b c d: the wires at row i; a_n b_n d_n: w_l w_r w_4 at row (i + 1) mod n; delta(f) = f (f-1) (f-2) (f-3); la = a_n - 4a,
 * lb = b_n - 4b, ld = d_n - 4d, F as in logic.rs:104-133.  sigma[k][i] = K_w' * omega^row' (K = 1, 7, 13, 17) is decoded through a device
 * map of the 4n identity encodings, so any key works, compiled or written by hand; an entry that is no such encoding is
 * ZK_ERR_BAD_ARG (one flag word, read back with the summary), not a mask bit.
 * All columns: device vectors of n Montgomery Fr in canonical form (evaluations over the domain, not coefficients). */
typedef struct zk_circuit_check_args {
    const void *w_l, *w_r, *w_o, *w_4, *pi;          /* pi may be NULL (= zeros) */
    const void *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *q_arith, *q_range, *q_logic, *q_fixed_group_add, *q_variable_group_add, *q_lookup;
    const void* sigma[4];                            /* left, right, out, fourth: evaluations over the domain */
    const void* table[4];                            /* four columns of table_rows rows (may be NULL when table_rows = 0) */
    size_t table_rows;                               /* <= n; duplicates allowed (the padding repeats row 0) */
    uint64_t coeff_a[4], coeff_d[4];                 /* P::COEFF_A, P::COEFF_D of the embedded twisted Edwards curve */
} zk_circuit_check_args;
typedef struct zk_circuit_check_summary {
    uint64_t failing_rows;                           /* rows with a non-zero mask */
    uint64_t first_row;                              /* the smallest of them; n when there is none */
    uint32_t first_mask, reserved;                   /* its mask */
    uint64_t bit_count[32];                          /* rows that have bit b set */
} zk_circuit_check_summary;
/* args: a zk_circuit_check_args; out: a zk_circuit_check_summary (host); d_mask: u32[n] on the device, or NULL when the summary is
 * enough.  (Both structs cross as untyped pointers, like the column buffers: the bindings are generated and checked against a fixed
 * set of struct parameter types.)  Returns ZK_OK whether or not the circuit is satisfied -- the summary says which.
 * ZK_ERR_BAD_ARG: a null ctx / args / out (before anything else), a null column, table_rows > n, a sigma entry that is no identity
 * encoding; ZK_ERR_DOMAIN_TOO_LARGE: log_n beyond the two-adicity; ZK_ERR_UNSUPPORTED: log_n > 28 (positions are 32-bit).
 * Working memory: one device allocation per call, freed before return -- 160 n + 4 * (the power of two >= 2 table_rows) + 8 KiB bytes,
 * + 4 n when d_mask is NULL (<= 172 n + 8 KiB).  No buffer of the ctx is used: the call runs inside an open deferred round.
 * Blocks once. */
int zk_circuit_check_dev(zk_ctx* ctx, int curve_id, uint32_t log_n, const void* args, void* d_mask, void* out);

/* ---- gadget circuits and their witnesses (constraint_system/{arithmetic,boolean,range,logic,composer,lookup}.rs, ecc/) ----------- */
/* A SEGMENT is `calls` calls of one gadget with the same parameters: by definition what `StandardComposer` holds after the gadget is
 * called that many times in a row, call k with the k-th input variables -- rows, new variables in `add_input` order and
 * `add_variable_to_map` calls in call order, the cells the reference pushes without mapping (range.rs:185-187) and the logic gate's
 * Output(n - 1) after Left(n) included.  Every gadget has a fixed shape per call (R rows, V new variables, I insertions), so call k
 * owns rows row0 + k R .., variables var0 + k V .. and insertions k I ..; M = MODULUS_BITS of Fr (255 / 254):
 *   kind                  reference                                         R                  V            I
 *   ZK_GADGET_POLY        arithmetic_gate, poly_gate, constrain_to_constant,
 *                         assert_equal, boolean_gate                        1                  0 or 1       4
 *   ZK_GADGET_RANGE       range_gate(num_bits)                              ceil(bits/8) + 2   bits / 2     4 ceil(bits/8) + 5
 *   ZK_GADGET_LOGIC       xor_gate / and_gate(num_bits)                     bits / 2 + 1       2 bits       2 bits + 4
 *   ZK_GADGET_CURVE_ADD   point_addition_gate                               2                  3            8
 *   ZK_GADGET_FIXED_BASE  fixed_base_scalar_mul                             M + 5              4 M + 3      4 (M + 5)
 *   ZK_GADGET_CONST_WITNESS add_witness_to_circuit_description(value)       1                  1            4
 *   ZK_GADGET_IS_ZERO     is_zero_with_output(a)                            2                  2            8
 *   ZK_GADGET_IS_EQ       is_eq_with_output(a, b)                           3                  3            12
 *   ZK_GADGET_SELECT      conditional_select(bit, a, b)                     4                  4            16
 *   ZK_GADGET_POINT_SELECT conditional_point_select(p1, p0, bit)            8                  8            32
 *   ZK_GADGET_POINT_NEG   conditional_point_neg(bit, p)                     5                  5            20
 *   ZK_GADGET_VAR_BASE    variable_base_scalar_mul(scalar, point)           8 M + 2            9 M + 257    32 M + 8
 *   ZK_GADGET_LOOKUP      lookup_gate(a, b, c, d)                           1                  0            4
 *   ZK_GADGET_LOOKUP_OUT  lookup_gate(a, b, c, d) with
 *                         c = add_input(table.lookup(a, b, d)?)             1                  1            4
 *   ZK_GADGET_DUMMY       add_dummy_constraints()                           2                  4            8
 * The kinds from CONST_WITNESS on map every cell of every row, row by row (Left, Right, Output, Fourth).
 * Values (zk_gadget_witness_dev; canonical Montgomery Fr, what zk_fr_gather_dev and the circuit check take):
 *   POLY with ZK_GADGET_COMPUTE_OUT: (q_m a b + q_l a + q_r b + q_c + q_4 d + pi) (-q_o), as arithmetic.rs:144-155 writes it -- a
 *       product with -q_o, NOT a division by it;
 *   RANGE: accumulator j = (v mod 2^bits) >> (bits - 2 (j + 1)), v the canonical integer of the input -- the closing assert_equal row is
 *       satisfied iff v < 2^bits, as in the reference;
 *   LOGIC: per quad the two input prefixes (the same formula), the product of the two quads, the prefix of a ^ b or a & b;
 *   CURVE_ADD: x1 y2, then x3 = (x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), y3 = (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2);
 *   FIXED_BASE: the digit of weight 2^j of the width-2 NAF of the scalar e is bit j+1 of 3e minus bit j+1 of e (find_wnaf(2)); row i
 *       uses the digit of weight 2^(M-1-i) and holds the point and scalar accumulators before it and xy_alpha = x y of the addend
 *       +-2^(M-1-i) G, or 0;
 *   CONST_WITNESS: the new variable v holds the value, its row is (v, v, v, 0) with q_l = 1, q_c = -value (coeff[5] / coeff_const[20..24)
 *       is q_c, the value is its negative);
 *   IS_ZERO: new variables y = 1 / a (1 when a = 0) and b = 1 - a y; rows (a, b, 0, 0) q_m = 1 and (a, y, 0, b) q_m = q_4 = 1, q_c = -1, both
 *       with q_o = -1.  IS_EQ: the difference a - b on a row of its own (q_l = 1, q_r = -1), then IS_ZERO of it;
 *   SELECT: bit a; 1 - bit; (1 - bit) b; their sum -- four arithmetic rows, each value the product with -q_o of arithmetic.rs:144-155.
 *       POINT_SELECT: SELECT(bit, p1.x, p0.x) then SELECT(bit, p1.y, p0.y).  POINT_NEG: -x, then SELECT(bit, -x, x);
 *   VAR_BASE: variables 0 .. 255 the bits of the canonical scalar e (`to_bits_le` of four 64-bit words; bits M .. 255 appear on no row),
 *       256 + j (j < M) the accumulator e mod 2^(j+1), 256 + M the constant one of `Point::identity`, then for iteration i (bit M-1-i,
 *       from the identity (0, 1)) eight values: x1 y2, x3, y3 of the doubling; bit x; 1 - bit + bit y; x1 y2, x3, y3 of the addition, by
 *       the affine law above.  Rows: M x (boolean row, accumulator row with q_l = 2^j, q_r = 1), the assert_equal with the scalar, the
 *       row of the one, M x (2 rows of the doubling, select_zero, select_one, 2 rows of the addition).
 *   LOOKUP: no new variable; the row (a, b, c, d) has q_lookup = 1 alone.
 *   LOOKUP_OUT: the row (a, b, new, d) has q_lookup = 1 alone; the new variable holds c of the FIRST row of the lookup table whose
 *       (a, b, d) equals the values of the three inputs (`LookupTable::lookup`, lookup_table.rs:172-180: `.position` returns the first
 *       match, and rows with one key and different c are legal) -- one zk_lookup_map_query_dev over lut / lut_map.  The witness
 *       returns ZK_ERR_NOT_INDEXED when a call's key is in no row (Error::ElementNotIndexed); the calls that hit are still written;
 *   DUMMY (composer.rs:493-548): new variables 6, 1, 7, -20 in that order; row 0 is (six, seven, -20, one) with q_m q_l q_r q_o q_c q_4 =
 *       1, 2, 3, 4, 4, 1 and row 1 is (-20, six, seven, the zero variable) with 1, 1, 1, 1, 127, 0; both rows have q_arith = q_lookup = 1.
 * ZK_ERR_BAD_ARG, by one flag word read back once per call: an input id that is not smaller than var0 (an undefined variable); a
 * scalar whose NAF has more than M digits (3e >= 2^(M+1); the reference asserts); a zero denominator of the group law.  The outputs
 * of a refused call are unspecified; nothing is read or written outside the buffers. */
#define ZK_GADGET_POLY 0
#define ZK_GADGET_RANGE 1
#define ZK_GADGET_LOGIC 2
#define ZK_GADGET_CURVE_ADD 3
#define ZK_GADGET_FIXED_BASE 4
#define ZK_GADGET_CONST_WITNESS 5
#define ZK_GADGET_IS_ZERO 6
#define ZK_GADGET_IS_EQ 7
#define ZK_GADGET_SELECT 8
#define ZK_GADGET_POINT_SELECT 10                    /* 9 is no kind: it stays refused, as every unknown number is */
#define ZK_GADGET_POINT_NEG 11
#define ZK_GADGET_VAR_BASE 12
#define ZK_GADGET_LOOKUP 13
#define ZK_GADGET_LOOKUP_OUT 15                      /* 14 is no kind either: callers probe ZK_GADGET_LOOKUP + 1 for the end of the first table */
#define ZK_GADGET_DUMMY 16
#define ZK_GADGET_COMPUTE_OUT 1                      /* flags, POLY: the output wire is a new variable whose value is computed */
#define ZK_GADGET_XOR 2                              /* flags, LOGIC: q_c = q_logic = -1 (XOR); without it +1 (AND) */
typedef struct zk_gadget_args {
    uint32_t kind, num_bits, flags, reserved;
    uint64_t calls;                                  /* B >= 1 */
    uint64_t row0, var0;                             /* first row and first new variable of the segment (var0 >= 1) */
    const void* inputs[4];                           /* u32[calls] variable ids on the device -- POLY: a, b, c (unless computed), d (NULL:
                                                      * the zero variable); RANGE: the witness; LOGIC: a, b; CURVE_ADD: x1, y1, x2, y2;
                                                      * FIXED_BASE: the scalar */
    const void* coeff[6];                            /* POLY: q_m q_l q_r q_o q_4 q_c as columns of `calls` Montgomery Fr, or NULL ... */
    uint64_t coeff_const[24];                        /* ... for the constant coeff_const[4 j .. 4 j + 4) */
    const void* pi;                                  /* POLY: the public input of every call (Montgomery Fr, device), or NULL; read by
                                                      * the witness of a computed output only */
    uint64_t coeff_a[4], coeff_d[4];                 /* P::COEFF_A, P::COEFF_D of the embedded twisted Edwards curve (Montgomery) */
    const void* table;                               /* FIXED_BASE: 3 M Montgomery Fr on the device, row i: x, y, x y of 2^(M-1-i) G */
    const void* inputs_ext[4];                       /* inputs 4 .. 7, as `inputs`: the kinds from CONST_WITNESS on take, in order --
                                                      * IS_ZERO: a; IS_EQ: a, b; SELECT: bit, a, b; POINT_SELECT: bit, p1.x, p0.x, p1.y,
                                                      * p0.y (the fifth is inputs_ext[0]); POINT_NEG: bit, x; VAR_BASE: scalar, x, y of
                                                      * the point; LOOKUP: a, b, c, d (NULL: the zero variable); LOOKUP_OUT: a, b, d
                                                      * (each may be NULL: the zero variable) */
    const void* lut[4];                              /* LOOKUP_OUT, read by the witness only: the four columns of the lookup table ... */
    uint64_t lut_rows;                               /* ... of this many rows (Montgomery Fr, device), */
    const void* lut_map;                             /* its map (zk_lookup_map_build_dev over columns 0, 1, 3) */
    uint64_t lut_slots;                              /* and the map's slot count, zk_lookup_map_slots(lut_rows).  Other kinds ignore them */
} zk_gadget_args;
/* Host only: the shape of one call and the device bytes a witness of `calls` calls allocates (layout: 256). */
int zk_gadget_shape(int kind, int curve_id, uint32_t num_bits, uint32_t flags, size_t calls, uint32_t* rows, uint32_t* vars, uint32_t* insertions,
                    size_t* work_bytes);
/* args: a zk_gadget_args (crosses as an untyped pointer, like zk_circuit_check_args).  With N = calls * R and m = calls * I:
 * d_wire_ids u32[4][N] (Left, Right, Output, Fourth of every row of the segment); d_selectors: 12 device pointers of N Montgomery Fr
 * in the order q_m q_l q_r q_o q_4 q_c q_arith q_range q_logic q_fixed_group_add q_variable_group_add q_lookup; d_ins_var, d_ins_rec
 * u32[m]: the insertions in call order, a record being wire << 30 | row with the ABSOLUTE row (row0 included) -- independent of the
 * padded size; position = wire * n + row once n is known.  ZK_ERR_BAD_ARG: a null ctx / args (before anything else), a null buffer,
 * num_bits odd or outside 2 .. 256, an input id >= var0; ZK_ERR_UNSUPPORTED: rows beyond 2^28 or variables beyond 2^31.
 * Working memory: one device allocation of 256 bytes, freed before return.  Runs inside an open deferred round.  Blocks once. */
int zk_gadget_layout_dev(zk_ctx* ctx, int curve_id, const void* args, void* d_wire_ids, void* const* d_selectors, void* d_ins_var,
                         void* d_ins_rec);
/* The values of the segment's new variables into d_values[var0 .. var0 + calls * V) (num_vars rows of Montgomery Fr); the inputs'
 * values are read from the same vector, so segments are replayed in build order.  Working memory: one device allocation, freed on
 * every path -- 256 bytes, + 96 (M + 1) calls for FIXED_BASE and + 96 (2 M + 1) calls for VAR_BASE (the projective accumulators
 * between the two phases of a scalar multiplication: a walk of one lane per call, then a normalisation with one inversion per 256
 * lanes).  No buffer of the ctx is used: the call runs inside an open deferred round.  Blocks once.  LOOKUP_OUT: ZK_ERR_BAD_ARG for
 * a null table column or map (with lut_rows > 0) or a slot count that is not the table's; ZK_ERR_NOT_INDEXED for a key in no row. */
int zk_gadget_witness_dev(zk_ctx* ctx, int curve_id, const void* args, void* d_values, size_t num_vars);
/* One block of a lookup table (lookup/lookup_table.rs:94-152 insert_multi_add / _mul / _xor / _and(lower_bound, n_bits)) on the device:
 * with w = 2^n_bits - lower_bound, row r < w^2 holds a = lower_bound + r / w, b = lower_bound + r % w, c = op(a, b) mod 2^n_bits and the
 * tag of the operation -- op 0: add, tag 0; 1: mul, tag 1; 2: xor, tag -1; 3: and, tag 2 -- as Montgomery Fr into the four columns
 * d_a, d_b, d_c, d_d (w^2 elements each; a caller concatenates blocks by offsetting the pointers).  ZK_ERR_BAD_ARG: a null ctx or
 * column, an unknown op, n_bits > 12, lower_bound >= 2^n_bits.  Queued on the ctx stream; uses no buffer of the ctx. */
int zk_lookup_table_dev(zk_ctx* ctx, int curve_id, int op, uint32_t lower_bound, uint32_t n_bits, void* d_a, void* d_b, void* d_c, void* d_d);

/* ---- the output of a lookup: (a, b, d) -> c of the first matching row (lookup/lookup_table.rs:172-180 `LookupTable::lookup`) ------ */
/* An open-addressing map (linear probing) from the key (a, b, d) of a table row to the SMALLEST index of a row that holds it: the
 * reference's `.position(..)` returns the first match, and rows with one key and different c are legal.  Keys are compared as 32-byte
 * strings: pass reduced (canonical Montgomery) elements, as everywhere.  Memory: 4 * slots bytes per table, owned by the caller.
 * Host only: the slot count of a table of `rows` rows -- the power of two >= 2 * rows, at least 64; 0 for more than 2^30 rows. */
size_t zk_lookup_map_slots(size_t rows);
/* d_a, d_b, d_d: the three key columns, `rows` elements each (may be NULL when rows = 0); d_slots: u32[slots], slots =
 * zk_lookup_map_slots(rows), overwritten.  Afterwards every distinct key names its smallest row index, whatever order the lanes
 * arrive in (first claim of a slot by compare-and-swap, then a minimum).  rows = 0 gives an empty map.  ZK_ERR_BAD_ARG: a null ctx,
 * column or buffer, a slot count that is not the table's; ZK_ERR_UNSUPPORTED: more than 2^30 rows.  Queued on the ctx stream; uses no
 * buffer of the ctx. */
int zk_lookup_map_build_dev(zk_ctx* ctx, int curve_id, const void* d_a, const void* d_b, const void* d_d, size_t rows, void* d_slots,
                            size_t slots);
/* n queries (n < 2^32) against the table d_table (its four columns a, b, c, d of `rows` rows) and its map.  Operand w of query i
 * (w = 0, 1, 2: a, b, d; d_operands holds three pointers) is d_operands[w][i], or d_operands[w][d_operand_ids[w][i]] where d_operand_ids is not NULL and its entry w
 * is a u32[n] vector on the device; every operand vector holds operand_rows elements.  c of the first matching row goes to d_out[i], or
 * to d_out[d_out_ids[i]] when d_out_ids (u32[n]) is not NULL; d_out holds out_rows elements.  d_pos (u32[n], or NULL) receives the
 * matching row index, 0xFFFFFFFF for a miss.  ZK_ERR_NOT_INDEXED when a query matches no row (Error::ElementNotIndexed): *misses
 * (or NULL) receives how many do, *first_miss (or NULL) the smallest such i (n when there is none); the hits are written all the
 * same and a miss writes nothing but its d_pos.  ZK_ERR_BAD_ARG: a null ctx, table column (with rows > 0), map, operand vector or
 * d_out, a slot count that is not the table's, operand_rows < n or out_rows < n for a vector read or written directly, an index
 * that is not below operand_rows / out_rows (by one flag word; such a query reads and writes nothing); ZK_ERR_UNSUPPORTED: n >= 2^32.
 * Working memory: one device allocation of 256 bytes, freed before return; no buffer of the ctx is used: the call runs inside an
 * open deferred round.  Blocks once (one 12-byte read-back of the flag, the miss count and the first miss). */
int zk_lookup_map_query_dev(zk_ctx* ctx, int curve_id, const void* const d_table[4], size_t rows, const void* d_slots, size_t slots, size_t n,
                            const void* const* d_operands, const void* const* d_operand_ids, size_t operand_rows, void* d_out,
                            const void* d_out_ids, size_t out_rows, void* d_pos, uint64_t* misses, uint64_t* first_miss);

/* ---- the KZG pairing check (csrc/pairing.hip, csrc/pairing.cuh) --------------------------------------- */
/* Replaces ark_ec::PairingEngine::product_of_pairings as kzg10::KZG10::check calls it: ok = [ e(L, [tau]H) e(-R, H) == 1 ] for the two
 * G1 inputs (L, R) a batch of KZG proofs folds into (zk_verify_scalars_dev and the MSMs behind it), with both G2 points fixed by the
 * verifier key.  A key is prepared once: its two Miller loops are walked on the host into line tables, and a check is then line
 * evaluations at G1 points, sparse Fq12 products and the final exponentiation -- no G2 arithmetic where a check runs.
 *
 * The key is an opaque handle that crosses as an untyped pointer (`key` below; zk_pairing_key_new writes it to *out).
 * G2 points: affine, x.c0 x.c1 y.c0 y.c1, L limbs each (L = 6 / 4), Montgomery form, Fq2 = Fq[u]/(u^2 + 1).
 * G1 points: what the library writes -- x y, L limbs each, Montgomery; infinity by flag or as (0, 1) / (0, 0).  They are the
 * library's own outputs and are not tested for the curve or the subgroup.  Both coordinates must be reduced (below q): an unreduced
 * y changes a verdict, since its negation is not the negation of the residue.  The host entry points (zk_kzg_pairing_check,
 * zk_pairing_gt) return ZK_ERR_BAD_ARG, and write nothing, for a point without its infinity flag that has a coordinate >= q -- the
 * unreduced spellings (q, 1), (q, q) of infinity included; a point passed with its flag set is not inspected.  The device entry
 * points read arrays the library wrote on the device and do not look: unreduced coordinates are outside the contract there.
 * GT values: 12 Fq elements, Montgomery, in arkworks' tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... (Fq6 = Fq2[v]/(v^3 - xi),
 * Fq12 = Fq6[w]/(w^2 - v)).  The value is e(P, Q)^c for the reduced pairing e with the exponent (q^12 - 1) / r exactly and the small
 * constant c of the curve, coprime to r: c = 3 on BLS12-381 (the x-chain of the hard part), c = 1 on BN254
 * (ZK_PAIRING_GT_POWER_* in csrc/pairing.cuh). */
/* Validates h and tau_h (each coordinate reduced; on the twist y^2 = x^3 + 4(1 + u) / y^2 = x^3 + 3/(9 + u); not infinity; [r]Q =
 * infinity) and prepares both tables, on the host: no ctx, no GPU.  ZK_ERR_BAD_ARG: a null pointer, an unknown curve, a point
 * that fails a test. */
int zk_pairing_key_new(int curve_id, const uint64_t* h, const uint64_t* tau_h, void** out);
/* Frees the key and its device copies (one per device a batch call ran on; waits for that device).  NULL is a no-op. */
void zk_pairing_key_free(void* key);
/* *ok = [ e(L, tau_h) e(-R, h) == 1 ].  Host only: milliseconds, the form for one check per fold. */
int zk_kzg_pairing_check(const void* key, const uint64_t* L_xy, int L_inf, const uint64_t* R_xy, int R_inf, int* ok);
/* n independent checks, one per lane of one launch: d_ok[j] (n bytes) = the verdict of (d_L[j], d_R[j]).  d_L_inf / d_R_inf: n flag
 * bytes, or NULL (infinity by encoding only).  Queued on the ctx stream; nothing is read back.  The first call on a device uploads
 * the key's tables there (blocking, once).  n == 0 is a no-op. */
int zk_kzg_pairing_check_batch_dev(zk_ctx* ctx, void* key, const void* d_L, const uint8_t* d_L_inf, const void* d_R, const uint8_t* d_R_inf,
                                   size_t n, uint8_t* d_ok);
/* out = e(P, which ? tau_h : h)^c as 12 L limbs (the identity for P = infinity): what the tests pin to an independent pairing. */
int zk_pairing_gt(const void* key, int which, const uint64_t* P_xy, int P_inf, uint64_t* out);
/* ... for n points on the device, one per lane: d_out holds n GT values. */
int zk_pairing_gt_batch_dev(zk_ctx* ctx, void* key, int which, const void* d_P, const uint8_t* d_inf, size_t n, void* d_out);

/* ---- device self-test ------------------------------------------------------------------------------ */
/* Runs the quad-cooperative point arithmetic of the bucket-reduction kernels (csrc/ecq.cuh) against the
 * single-lane group law on n_quads point pairs incl. doubling, cancellation and infinity cases.
 * *mismatches = number of disagreeing pairs (0 expected); *case_mask (optional) = which cases failed. */
int zk_selftest_quad_dev(zk_ctx* ctx, int curve_id, uint32_t n_quads, uint32_t* mismatches, uint32_t* case_mask);

/* ---- utilities (a synthetic known-logarithm SRS for tests/bench; a real IPA key: zk_ipa_sample_generators_dev) --------- */
/* out[i] = scalars[i] * G1 generator, affine Montgomery, device buffers. */
int zk_g1_fixed_base_batch_dev(zk_ctx* ctx, int curve_id, const void* d_scalars, size_t n, void* d_out_xy);
/* out[i] = a[i] * b[i] (Montgomery Fr, device) -- pointwise helper for property tests. */
int zk_fr_mul_dev(zk_ctx* ctx, int curve_id, const void* d_a, const void* d_b, size_t n, void* d_out);

/* Device memory helpers so a non-torch host (the Rust shim, C++ host layer) needs no HIP headers. */
int zk_dev_alloc(zk_ctx* ctx, size_t bytes, void** d_ptr);
int zk_dev_free(zk_ctx* ctx, void* d_ptr);
int zk_dev_upload(zk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int zk_dev_download(zk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* device -> device on the ctx stream, queued in order with the kernels (no host wait): e.g. the four quarters of the quotient
 * polynomial as vectors of their own (prover.rs:107-123 split_tx_poly) for a caller whose vector type has no sub-ranges */
int zk_dev_copy(zk_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);

/* Library build info: returns "gfx950" etc. */
const char* zk_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* ARK_PLONK_AMD_H */
