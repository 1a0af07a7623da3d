// KZG10 opening helpers: random linear combination of polynomials and the
// witness polynomial (p(X) - p(z)) / (X - z), on the device -- and, with the same pieces, the two O(n) operations of the
// prover's last round (linearisation_poly.rs:164-350): `poly.evaluate(&point)` for the 23 evaluations of a proof
// (zk_poly_evaluate_dev) and the scalar-weighted sum of ~19 polynomials that is the linearisation polynomial
// (zk_poly_lincomb_dev).
//
// Replaces the CPU work ark-poly-commit 0.3 does inside `PolynomialCommitment::open` before its MSM
// (reference call sites: proof_system/prover.rs:582-591 -- 11 polynomials at z -- and :609-618 --
// 7 polynomials at z*w).  SonicKZG10::open without degree bounds or hiding:
//     p(X) = sum_k chi^k p_k(X);   w(X) = (p(X) - p(z)) / (X - z);   proof = commit(w).
// Synthetic division is the recurrence w[i-1] = p[i] + z*w[i]; here it runs as a three-phase
// Horner scan (chunk sums -> workgroup suffix scan with the operator (h,q)o(h',q') = (h+q h', q q')
// -> per-chunk replay), 3 field multiplications per coefficient, output already in canonical
// (into_repr) form for the opening MSM.
#include "ctx.h"
#include "zbound.cuh"

// Arithmetic: the 29-bit-limb Montgomery type of fieldu.cuh (as in the NTT), lazily reduced, with the bound carried in the type
// (zbound.cuh: Z<FU, B> is below B / 10 r, and a formula that could overflow does not compile).  Data stay in the arkworks
// Montgomery domain (R = 2^256): every constant multiplier (chi^k, z, z^CHUNK and the running powers of the
// scan) is held in the R' = 2^261 form, so data * multiplier / R' keeps the factor R; chunk sums and chunk
// carries are kept as lazily reduced limb vectors (48 B) between the phases, each buffer under one named type.

namespace {

constexpr int MAX_POLYS = 32;
struct RlcArgs {
    const void* poly[MAX_POLYS];
    uint64_t len[MAX_POLYS];
    Packed chi_pow[MAX_POLYS];   // chi^k in the R' form
    uint32_t n_polys;
};

// comb[i] = sum_k chi^k * p_k[i]
template <class FU>
__global__ void kzg_rlc(RlcArgs a, uint64_t m, void* comb) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    typedef ZRun<FU, 0, 20, MAX_POLYS> Sum;   // n_polys <= MAX_POLYS products: poly_lincomb and open_prepare refuse more
    typename Sum::T acc(FU::zero());
    for (uint32_t k = 0; k < a.n_polys; ++k) {
        if (i < a.len[k]) acc = Sum::step(acc, ld_c<FU>(a.poly[k], i) * unpack_c<FU>(a.chi_pow[k]));
    }
    st_c<FU>(comb, i, acc * z_one<FU>());
}

constexpr uint32_t CHUNK = 64;       // coefficients per lane in phases 1 and 3
constexpr uint32_t SCAN_T = 1024;    // lanes of the single scan workgroup
constexpr int SCAN_STEPS = 10;       // Hillis-Steele steps over them
static_assert(1u << SCAN_STEPS == SCAN_T, "the scan's step count is log2 of its lanes");

// the 48-byte buffers between the phases: what the writer stores and the reader loads
template <class FU> using ChunkSum = Z<FU, 30>;     // H: a Horner value c + acc * z
template <class FU> using LaneSum = Z<FU, 50>;      // HQ, even entries: a Horner value over chunk sums, H + h * zk
template <class FU> using LanePow = Z<FU, 20>;      // HQ, odd entries: a product of multipliers
template <class FU> using ScanRun = ZRun<FU, 50, 20, SCAN_STEPS>;      // a lane sum after up to SCAN_STEPS steps of h + q * h'
template <class FU> using Carry = typename ScanRun<FU>::T;           // the scan's carries and A, the value entering a chunk

// phase 1: H[t] = sum_{j < CHUNK} c[t*CHUNK + j] z^j
template <class FU>
__global__ void kzg_chunk_horner(const void* comb, uint64_t m, Packed zp, void* H, uint64_t n_chunks) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chunks) return;
    const Z<FU, 10> z = unpack_c<FU>(zp);
    const uint64_t lo = t * CHUNK;
    const uint64_t hi = lo + CHUNK < m ? lo + CHUNK : m;
    ChunkSum<FU> acc(FU::zero());
    for (uint64_t j = hi; j-- > lo;) acc = ld_c<FU>(comb, j) + acc * z;
    st_z<ChunkSum<FU>>(H, t, acc);
}

// phase 2: A[t] = sum_{t' > t} H[t'] (z^CHUNK)^(t'-t-1), the value flowing into chunk t.  SCAN_T lanes own n_chunks / SCAN_T
// consecutive chunks each.  Three launches: (a) every lane folds its chunks into (h, q), (b) ONE workgroup scans the SCAN_T
// pairs, (c) every lane replays its chunks from the value entering it.  (a) and (c) are the lanes' own loops and run as 16
// workgroups of one wavefront each -- alone on a SIMD a wavefront issues twice as often as it does sharing it with the three
// others of a 1024-lane workgroup on one CU, which is what the whole phase used to be (0.19 ms per opening with the rest of the
// chip idle).  Same operations on the same operands in the same order.
template <class FU>
ZK_D void scan_range(uint32_t u, uint64_t n_chunks, uint64_t& lo, uint64_t& hi) {
    const uint64_t per = (n_chunks + SCAN_T - 1) / SCAN_T;
    lo = (uint64_t)u * per < n_chunks ? (uint64_t)u * per : n_chunks;
    hi = lo + per < n_chunks ? lo + per : n_chunks;
}
template <class FU>
__global__ void __launch_bounds__(64) kzg_scan_local(const void* H, uint64_t n_chunks, Packed zkp /* z^CHUNK, R' form */, void* HQ) {
    const uint32_t u = blockIdx.x * 64 + threadIdx.x;
    const Z<FU, 10> zk = unpack_c<FU>(zkp);
    uint64_t lo, hi;
    scan_range<FU>(u, n_chunks, lo, hi);
    // local: h = sum_{t in [lo,hi)} H[t] zk^(t-lo) (data),  q = zk^(hi-lo) (multiplier, R' form)
    LaneSum<FU> h(FU::zero());
    LanePow<FU> q = z_one<FU>();
    for (uint64_t t = hi; t-- > lo;) {
        h = ld_z<ChunkSum<FU>>(H, t) + h * zk;
        q = q * zk;
    }
    st_z<LaneSum<FU>>(HQ, 2 * u, h);
    st_z<LanePow<FU>>(HQ, 2 * u + 1, q);
}
template <class FU>
__global__ void __launch_bounds__(SCAN_T) kzg_scan_cross(const void* HQ, void* carry_out) {
    extern __shared__ uint4 sh[];          // (h, q) per lane: 2 x 48 B
    const uint32_t u = threadIdx.x;
    Carry<FU> h = ld_z<LaneSum<FU>>(HQ, 2 * u);
    LanePow<FU> q = ld_z<LanePow<FU>>(HQ, 2 * u + 1);
    // exclusive suffix scan of (h, q) with (h1,q1) o (h2,q2) = (h1 + q1 h2, q1 q2): Hillis-Steele.  Every step adds one product to
    // h: h has the bound after the last of the SCAN_STEPS steps throughout, and q1 * h2 is checked against that.
    for (uint32_t d = 1; d < SCAN_T; d <<= 1) {
        st_z<Carry<FU>>(sh, 2 * u, h);
        st_z<LanePow<FU>>(sh, 2 * u + 1, q);
        __syncthreads();
        if (u + d < SCAN_T) {
            const Carry<FU> oh = ld_z<Carry<FU>>(sh, 2 * (u + d));
            const LanePow<FU> oq = ld_z<LanePow<FU>>(sh, 2 * (u + d) + 1);
            h = ScanRun<FU>::step(h, q * oh);
            q = q * oq;
        }
        __syncthreads();
    }
    // h = inclusive suffix value starting at this lane's first chunk; the value entering the lane
    // from above is the inclusive value of lane u+1
    st_z<Carry<FU>>(sh, 2 * u, h);
    __syncthreads();
    st_z<Carry<FU>>(carry_out, u, (u + 1 < SCAN_T) ? ld_z<Carry<FU>>(sh, 2 * (u + 1)) : Carry<FU>(FU::zero()));
}
template <class FU>
__global__ void __launch_bounds__(64) kzg_scan_replay(const void* H, uint64_t n_chunks, Packed zkp, const void* carry_in, void* A) {
    const uint32_t u = blockIdx.x * 64 + threadIdx.x;
    const Z<FU, 10> zk = unpack_c<FU>(zkp);
    uint64_t lo, hi;
    scan_range<FU>(u, n_chunks, lo, hi);
    Carry<FU> carry = ld_z<Carry<FU>>(carry_in, u);
    // replay the lane's chunks from the top to hand every chunk its incoming value (a LaneSum again after the first)
    for (uint64_t t = hi; t-- > lo;) {
        st_z<Carry<FU>>(A, t, carry);
        carry = ld_z<ChunkSum<FU>>(H, t) + carry * zk;
    }
}

// phase 3: replay each chunk with its incoming value; w[i-1] = c[i] + z*w[i], written canonical (into_repr)
template <class FU>
__global__ void kzg_witness(const void* comb, uint64_t m, Packed zp, const void* A, void* w_out, uint64_t n_chunks) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_chunks) return;
    const Z<FU, 10> z = unpack_c<FU>(zp);
    Z<FU, 10> unR(FU::zero());      // the plain integer R'/R = 2^5: (x R) * 2^5 / R' = x
    unR.v.v[0] = 32u;
    const uint64_t lo = t * CHUNK;
    const uint64_t hi = lo + CHUNK < m ? lo + CHUNK : m;
    Carry<FU> run = ld_z<Carry<FU>>(A, t);
    for (uint64_t j = hi; j-- > lo;) {
        run = ld_c<FU>(comb, j) + run * z;   // = w[j-1] (Montgomery, lazy: a ChunkSum)
        if (j >= 1) st_c<FU>(w_out, j - 1, run * unR);
    }
}

// ---- evaluations: out[y] = p_y(z_y) for n_polys polynomials in one launch pair ----------------------------------------
struct EvalArgs {
    const void* poly[MAX_POLYS];
    uint64_t len[MAX_POLYS];
    Packed z[MAX_POLYS];         // the point of polynomial y, R' form
    Packed zk[MAX_POLYS];        // z^CHUNK, R' form
    uint32_t n_polys;
    uint64_t max_chunks;
};
constexpr uint32_t FOLD_T = 256;

// phase 1 (grid: chunks x polys): H[y][t] = sum_{j < CHUNK} c_y[t*CHUNK + j] z_y^j
template <class FU>
__global__ void poly_chunk_horner(EvalArgs a, void* H) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t y = blockIdx.y;
    const uint64_t m = a.len[y];
    if (t * CHUNK >= m) return;
    const Z<FU, 10> z = unpack_c<FU>(a.z[y]);
    const uint64_t lo = t * CHUNK;
    const uint64_t hi = lo + CHUNK < m ? lo + CHUNK : m;
    ChunkSum<FU> acc(FU::zero());
    for (uint64_t j = hi; j-- > lo;) acc = ld_c<FU>(a.poly[y], j) + acc * z;
    st_z<ChunkSum<FU>>(H, (uint64_t)y * a.max_chunks + t, acc);
}

// phase 2 (one workgroup per polynomial): p(z) = sum_t H[t] (z^CHUNK)^t.  Lane u folds its `per` consecutive chunks by
// Horner, scales the result by (zk^per)^u (square and multiply on the lane index) and the workgroup adds the lanes up.
template <class FU>
__global__ void __launch_bounds__(FOLD_T) poly_chunk_fold(EvalArgs a, const void* H, void* out) {
    __shared__ uint4 sh[FOLD_T * 3];
    const uint32_t u = threadIdx.x, y = blockIdx.x;
    const uint64_t n_chunks = (a.len[y] + CHUNK - 1) / CHUNK;
    const uint64_t per = (n_chunks + FOLD_T - 1) / FOLD_T;
    const uint64_t lo = (uint64_t)u * per < n_chunks ? (uint64_t)u * per : n_chunks;
    const uint64_t hi = lo + per < n_chunks ? lo + per : n_chunks;
    const Z<FU, 10> zk = unpack_c<FU>(a.zk[y]);
    LaneSum<FU> h(FU::zero());
    for (uint64_t t = hi; t-- > lo;) h = ld_z<ChunkSum<FU>>(H, (uint64_t)y * a.max_chunks + t) + h * zk;
    // Q = zk^per (the same on every lane), then Q^u: products only
    LanePow<FU> Q = z_one<FU>(), b = zk;
    for (uint64_t e = per; e; e >>= 1) {
        if (e & 1) Q = Q * b;
        b = zmul_self(b);
    }
    LanePow<FU> s = z_one<FU>();
    b = Q;
    for (uint32_t e = u; e; e >>= 1) {
        if (e & 1) s = s * b;
        b = zmul_self(b);
    }
    // tree sum of the products h * s; every level re-normalises, so the shared array and the running sum stay below 2r
    Z<FU, 20> sum = h * s;
    st_z<Z<FU, 20>>(sh, u, sum);
    for (uint32_t d = FOLD_T / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (u < d) {
            sum = (sum + ld_z<Z<FU, 20>>(sh, u + d)) * z_one<FU>();
            st_z<Z<FU, 20>>(sh, u, sum);
        }
    }
    if (u == 0) st_c<FU>(out, y, sum);
}

template <class C>
int poly_evaluate(zk_ctx* c, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* points_mont, uint64_t* out_mont) {
    typedef typename C::Fr Fr;
    typedef typename C::FrU FU;
    if (n_polys > (uint32_t)MAX_POLYS) return ZK_ERR_UNSUPPORTED;
    if (n_polys == 0) return ZK_OK;
    EvalArgs a;
    memset(&a, 0, sizeof a);
    a.n_polys = n_polys;
    uint64_t m = 0;
    for (uint32_t k = 0; k < n_polys; ++k) {
        if (lens[k] && !d_polys[k]) return ZK_ERR_BAD_ARG;
        Fr z;
        if (!fr_reduced(points_mont + 4 * k, z)) return ZK_ERR_BAD_ARG;
        a.z[k] = pack_rp(z);
        a.zk[k] = pack_rp(Fr::pow_u64(z, CHUNK));
        a.poly[k] = d_polys[k];
        a.len[k] = lens[k];
        m = lens[k] > m ? lens[k] : m;
    }
    a.max_chunks = (m + CHUNK - 1) / CHUNK;
    int rc;
    if ((rc = c->io.b.ensure((size_t)n_polys * (a.max_chunks + 1) * 48 + (size_t)n_polys * 32))) return rc;
    void* H = c->io.b.p;
    void* d_out = (char*)c->io.b.p + (size_t)n_polys * (a.max_chunks + 1) * 48;
    hipStream_t st = c->stream;
    {
        ProfScope ps(c, "poly_evaluate");
        const int T = 128;
        if (a.max_chunks)
            hipLaunchKernelGGL(poly_chunk_horner<FU>, dim3((unsigned)((a.max_chunks + T - 1) / T), n_polys), dim3(T), 0, st, a, H);
        hipLaunchKernelGGL(poly_chunk_fold<FU>, dim3(n_polys), dim3(FOLD_T), 0, st, a, (const void*)H, d_out);
        ZK_HIP_TRY(hipGetLastError());
    }
    ZK_HIP_TRY(hipMemcpyAsync(out_mont, d_out, (size_t)n_polys * 32, hipMemcpyDeviceToHost, st));
    ZK_HIP_TRY(hipStreamSynchronize(st));
    c->io.d2h_bytes += (uint64_t)n_polys * 32;
    return ZK_OK;
}

template <class C>
int poly_lincomb(zk_ctx* c, uint32_t n_terms, const void* const* d_polys, const size_t* lens, const uint64_t* coeffs_mont, void* d_out, size_t out_len) {
    typedef typename C::Fr Fr;
    typedef typename C::FrU FU;
    if (n_terms > (uint32_t)MAX_POLYS) return ZK_ERR_UNSUPPORTED;
    if (out_len == 0) return ZK_OK;
    RlcArgs a;
    memset(&a, 0, sizeof a);
    a.n_polys = n_terms;
    for (uint32_t k = 0; k < n_terms; ++k) {
        if (lens[k] && !d_polys[k]) return ZK_ERR_BAD_ARG;
        Fr cf;
        if (!fr_reduced(coeffs_mont + 4 * k, cf)) return ZK_ERR_BAD_ARG;
        a.chi_pow[k] = pack_rp(cf);
        a.poly[k] = d_polys[k];
        a.len[k] = lens[k] < out_len ? lens[k] : out_len;
    }
    ProfScope ps(c, "poly_lincomb");
    const int T = 256;
    hipLaunchKernelGGL(kzg_rlc<FU>, dim3((unsigned)((out_len + T - 1) / T)), dim3(T), 0, c->stream, a, (uint64_t)out_len, d_out);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class C>
int open_prepare(zk_ctx* c, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* z_mont,
                 const uint64_t* chal_mont, void** d_w, size_t* wlen) {
    typedef typename C::Fr Fr;
    typedef typename C::FrU FU;
    if (n_polys > (uint32_t)MAX_POLYS) return ZK_ERR_UNSUPPORTED;
    uint64_t m = 0;
    for (uint32_t k = 0; k < n_polys; ++k) m = lens[k] > m ? lens[k] : m;
    *wlen = m > 0 ? m - 1 : 0;
    *d_w = nullptr;
    if (m <= 1) return ZK_OK;
    // z and chi are not validated here (the other entry points refuse an unreduced scalar: fr_reduced); an unreduced word stands for
    // its residue, as it always did: z * 1 is that residue, reduced, and chi enters through products only.
    const Fr z = Fr::mul(fr_arg<Fr>(z_mont), Fr::one()), chi = fr_arg<Fr>(chal_mont);
    RlcArgs a;
    memset(&a, 0, sizeof a);
    a.n_polys = n_polys;
    Fr pw = Fr::one();
    for (uint32_t k = 0; k < n_polys; ++k) {
        a.poly[k] = d_polys[k];
        a.len[k] = lens[k];
        a.chi_pow[k] = pack_rp(pw);
        pw = Fr::mul(pw, chi);
    }
    const uint64_t n_chunks = (m + CHUNK - 1) / CHUNK;
    int rc;
    if ((rc = c->io.a.ensure(m * 32))) return rc;                       // comb
    if ((rc = c->io.b.ensure((n_chunks * 2 + (size_t)SCAN_T * 3) * 48))) return rc;   // H | A | the scan's (h, q) pairs and carries (limb vectors)
    if ((rc = c->witness.ensure(m * 32))) return rc;                      // witness, canonical
    void* comb = c->io.a.p;
    void* H = c->io.b.p;
    void* A = (char*)c->io.b.p + n_chunks * 48;
    const Packed zp = pack_rp(z), zkp = pack_rp(Fr::pow_u64(z, CHUNK));
    hipStream_t st = c->stream;
    ProfScope ps(c, "kzg_open_prep");
    const int T = 256;
    hipLaunchKernelGGL(kzg_rlc<FU>, dim3((unsigned)((m + T - 1) / T)), dim3(T), 0, st, a, m, comb);
    hipLaunchKernelGGL(kzg_chunk_horner<FU>, dim3((unsigned)((n_chunks + T - 1) / T)), dim3(T), 0, st, comb, m, zp, H, n_chunks);
    void* HQ = (char*)c->io.b.p + n_chunks * 2 * 48;
    void* CR = (char*)HQ + (size_t)SCAN_T * 2 * 48;
    size_t shmem = (size_t)SCAN_T * 2 * 48;
    ZK_HIP_TRY(hipFuncSetAttribute((const void*)kzg_scan_cross<FU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(kzg_scan_local<FU>, dim3(SCAN_T / 64), dim3(64), 0, st, H, n_chunks, zkp, HQ);
    hipLaunchKernelGGL(kzg_scan_cross<FU>, dim3(1), dim3(SCAN_T), shmem, st, HQ, CR);
    hipLaunchKernelGGL(kzg_scan_replay<FU>, dim3(SCAN_T / 64), dim3(64), 0, st, H, n_chunks, zkp, CR, A);
    hipLaunchKernelGGL(kzg_witness<FU>, dim3((unsigned)((n_chunks + T - 1) / T)), dim3(T), 0, st, comb, m, zp, A, c->witness.p, n_chunks);
    ZK_HIP_TRY(hipGetLastError());
    *d_w = c->witness.p;
    return ZK_OK;
}

}  // namespace

int poly_evaluate_dev(zk_ctx* c, int curve, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* points_mont,
                      uint64_t* out_mont) {
    return zk_on_curve(curve, ZK_ERR_BAD_ARG, [&](auto cv) { return poly_evaluate<decltype(cv)>(c, n_polys, d_polys, lens, points_mont, out_mont); });
}

int poly_lincomb_dev(zk_ctx* c, int curve, uint32_t n_terms, const void* const* d_polys, const size_t* lens, const uint64_t* coeffs_mont,
                     void* d_out, size_t out_len) {
    return zk_on_curve(curve, ZK_ERR_BAD_ARG, [&](auto cv) { return poly_lincomb<decltype(cv)>(c, n_terms, d_polys, lens, coeffs_mont, d_out, out_len); });
}

int kzg_open_prepare_dev(zk_ctx* c, int curve, uint32_t n_polys, const void* const* d_polys, const size_t* lens,
                         const uint64_t* z_mont, const uint64_t* chal_mont, void** d_witness_canonical, size_t* wlen) {
    return zk_on_curve(curve, ZK_ERR_BAD_ARG, [&](auto cv) { return open_prepare<decltype(cv)>(c, n_polys, d_polys, lens, z_mont, chal_mont, d_witness_canonical, wlen); });
}
