// Many small MSMs over one set of bases, each as a point: out[s] = sum over t in [off[s], off[s + 1]) of scalar[t] * base[index[t]].
//
// The batched form of `HomomorphicCommitment::multi_scalar_mul` (plonk-core/src/commitment.rs:8-91: at most 19 points per call) and
// of the combined commitment C = sum_k chi^k C_k that ipa_pc's check hashes into its transcript: a batch of proofs needs thousands of
// them, each of a few dozen terms, and each as an affine point -- the MSM entry points give ONE sum of many terms.
//
// One 64-lane wavefront per segment, SEG_PER_BLOCK segments per workgroup.  The lanes stride over the segment's terms; a lane runs
// one double-and-add per term on the XYZZ law of ecu.cuh (256 steps for every lane: the scalar's top bit only selects whether the
// base is added, so the wavefront walks one loop; a lane with nothing to do holds infinity, which dbl returns as it is), adds the
// term into its own sum, and the 64 sums are added up in LDS with the law's full addition (equal points, opposite points and
// infinity are its branches).  The workgroup's results are normalised with ONE field inversion (block_inverse.cuh) and the law's
// to_affine_given, as the key fold of ipa.hip does.  Offsets and indices are data: a bad one is a status, and nothing outside the
// buffers is read.
//
// Built once for both curves; with -DZK_CURVE_SEL=<0|1> only that curve's kernel is instantiated (the register test compiles each
// on its own: tests/test_g1_segments_build.py).
#include "api_internal.h"
#include "block_inverse.cuh"

namespace {

constexpr uint32_t SEG_W = 64;                            // lanes per segment
constexpr uint32_t SEG_PER_BLOCK = 4;                     // segments per workgroup = points per batched inversion
constexpr uint32_t SEG_T = SEG_W * SEG_PER_BLOCK;

#if defined(ZK_CURVE_SEL)
template <class Cv>
constexpr bool seg_built = std::is_same<Cv, CurveBls>::value == (ZK_CURVE_SEL == 0);
#else
template <class Cv>
constexpr bool seg_built = true;
#endif

// the lane sums of the reduction, then (after a barrier) the products of the inversion
template <class F>
union SegLds {
    XYZZu<F> sum[SEG_T];
    BlockInverseLds<F, SEG_T> inv;
};

template <class Cv>
__global__ void __launch_bounds__(SEG_T) g1_segments(uint64_t n_bases, const uint32_t* bases_xy, const uint8_t* bases_inf, uint64_t n_seg,
                                                     const uint64_t* seg_offsets, uint64_t n_terms, const uint32_t* base_index,
                                                     const uint32_t* scalars, uint32_t* out_xy, uint8_t* out_inf, uint8_t* status) {
    typedef typename Cv::FqU F;
    typedef XYZZu<F> P;
    constexpr int SAT = F::SAT;
    __shared__ SegLds<F> lds;
    const uint32_t t = threadIdx.x, lane = t % SEG_W;
    const uint64_t s = (uint64_t)blockIdx.x * SEG_PER_BLOCK + t / SEG_W;
    const bool have = s < n_seg;
    uint64_t lo = 0, hi = 0;
    uint32_t st = ZK_SEG_OK;
    if (have) {
        lo = seg_offsets[s];
        hi = seg_offsets[s + 1];
        if (lo > hi || hi > n_terms) {
            st = ZK_SEG_BAD_RANGE;
            lo = hi = 0;
        }
    }
    lds.sum[t] = P::infinity();                                      // the lane's own sum: in LDS while a term is computed
    bool bad = false;
    for (uint64_t first = lo; first < hi; first += SEG_W) {          // the same trip count for the 64 lanes of a segment
        const uint64_t k = first + lane;
        uint32_t sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        AffineU<F> q;
        q.x = F::zero();
        q.y = F::zero();
        if (k < hi) {
            const uint64_t idx = base_index[k];
            if (idx >= n_bases) {
                bad = true;
            } else if (!(bases_inf && bases_inf[idx])) {
                uint32_t any = 0;
#pragma unroll
                for (int w = 0; w < 8; ++w) any |= sc[w] = scalars[8 * k + w];
                if (any) {                                          // a zero scalar: the base's words are not used
                    q.x = F::from_sat(bases_xy + idx * 2 * SAT);
                    q.y = F::from_sat(bases_xy + idx * 2 * SAT + SAT);
                }
            }
        }
        const bool on = !q.is_null();
        P acc = P::infinity();
        for (int step = 0; step < 256; ++step) {
            acc = P::dbl(acc);
            const bool bit = on && (sc[7] >> 31);
#pragma unroll
            for (int w = 7; w > 0; --w) sc[w] = (sc[w] << 1) | (sc[w - 1] >> 31);
            sc[0] <<= 1;
            if (bit) acc = P::madd(acc, q);
        }
        lds.sum[t] = P::add(lds.sum[t], acc);
    }
    // the 64 lane sums of every segment -> its lane 0
    P total = lds.sum[t];
    for (uint32_t d = SEG_W / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (lane < d) {
            total = P::add(total, lds.sum[t + d]);
            lds.sum[t] = total;
        }
    }
    if (__any(bad)) st = ZK_SEG_BAD_INDEX;
    __syncthreads();                                                 // the sums are read: the same LDS now takes the products
    const bool fin = have && lane == 0 && st == ZK_SEG_OK && !total.is_inf();
    if (!fin) total.zzz = F::one();                                  // a lane with no finite result enters the product as 1
    const F zi3 = block_inverse(total.zzz, lds.inv);                 // 1 / ZZZ
    if (!have || lane != 0) return;
    uint32_t* w = out_xy + s * 2 * SAT;
    if (fin) {
        AffineU<F> a;
        total.to_affine_given(zi3, a);
        a.x.to_sat(w);
        a.y.to_sat(w + SAT);
    } else {                                                         // GroupAffine::zero() = (0, 1)
        for (int k = 0; k < SAT; ++k) {
            w[k] = 0;
            w[SAT + k] = Cv::FqP::R(k);
        }
    }
    out_inf[s] = fin ? 0 : 1;
    status[s] = (uint8_t)st;
}

template <class Cv>
int segments_impl(zk_ctx* c, size_t n_bases, const void* d_bases_xy, const void* d_bases_inf, size_t n_seg, const void* d_seg_offsets,
                  size_t n_terms, const void* d_base_index, const void* d_scalars, void* d_out_xy, void* d_out_inf, void* d_status) {
    if constexpr (!seg_built<Cv>) {
        return ZK_ERR_UNSUPPORTED;
    } else {
        ProfScope ps(c, "g1_segments");
        hipLaunchKernelGGL(g1_segments<Cv>, dim3(blocks_of(n_seg, SEG_PER_BLOCK)), dim3(SEG_T), 0, c->stream, (uint64_t)n_bases,
                           (const uint32_t*)d_bases_xy, (const uint8_t*)d_bases_inf, (uint64_t)n_seg, (const uint64_t*)d_seg_offsets,
                           (uint64_t)n_terms, (const uint32_t*)d_base_index, (const uint32_t*)d_scalars, (uint32_t*)d_out_xy, (uint8_t*)d_out_inf,
                           (uint8_t*)d_status);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    }
}

}  // namespace

int zk_msm_g1_segments_dev(zk_ctx* c, int curve_id, size_t n_bases, const void* d_bases_xy, const void* d_bases_inf, size_t n_seg,
                           const void* d_seg_offsets, size_t n_terms, const void* d_base_index, const void* d_scalars, void* d_out_xy,
                           void* d_out_inf, void* d_status) {
    if (!c || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (n_seg == 0) return ZK_OK;
    if (!d_seg_offsets || !d_out_xy || !d_out_inf || !d_status) return ZK_ERR_BAD_ARG;
    if ((n_terms && (!d_base_index || !d_scalars)) || (n_bases && !d_bases_xy)) return ZK_ERR_BAD_ARG;
    if (n_seg > ((size_t)1 << 31)) return ZK_ERR_UNSUPPORTED;      // one workgroup per SEG_PER_BLOCK segments in one grid
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return segments_impl<decltype(cv)>(c, n_bases, d_bases_xy, d_bases_inf, n_seg, d_seg_offsets, n_terms, d_base_index, d_scalars,
                                           d_out_xy, d_out_inf, d_status);
    });
}
