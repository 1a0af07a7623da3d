// MSM unit 3 of 4 (msm_common.cuh): from the accumulation's buckets and chunk-edge partials to window sums.
//   msm_combine*      joins the chunk-edge partials of each bucket: lane(s) / wavefront (shuffle tree) / workgroup per bucket by size class
//   msm_seg_reduce    segmented running-sum reduction (sum_j j * B_j), level 1
//   msm_win_finish    LDS suffix-scan + tree reduction per (virtual) window -> window sums: arkworks layout straight into pinned host
//                     memory, or -- the multi-GPU exchange -- the internal form into a device buffer (the collective's send buffer)
//   *_q               quad-cooperative forms (ecq.cuh): four lanes per dependent chain where the launch is latency-shaped
//   g1_sum_winsums_q  the ranks' window sums added element-wise after the all-gather
// Steps the kernels share are defined once, in front of them: the per-job views of RJobs (CombineJob, SegJob), the size class of a
// bucket and its queue (classify_bucket), the shuffle tree over a group of lanes (lane_group_sum) and the writer of a window sum
// that leaves the device (put_winsum / put_winsum_q).  Host side: launch_combine, seg_reduce_finish_q and level_geom (msm_common.cuh)
// are what queue_reduce and queue_reduce_wide are put together from.
// host: the few window sums are combined (table path: sum of 64 virtual windows; per-window path: Horner with W * c doublings) and
// normalised to affine in msm_plan.hip.
#include "msm_common.cuh"
#include "ecq.cuh"

namespace {

// one job (blockIdx.y) of a launch as the combine kernels see it; L = references per lane the accumulation really used
struct CombineJob {
    const void* part_pt;
    const uint32_t* offsets;
    void* buckets;
    uint32_t* q;
    uint32_t L;
    ZK_D CombineJob(const RJobs& jobs, uint32_t k)
        : part_pt(jobs.part_pt[k]), offsets(jobs.offsets[k]), buckets(jobs.buckets[k]), q(jobs.q[k]),
          L(chunk_len(offsets[jobs.nbk[k]], jobs.lanes[k], jobs.L[k])) {}
};
// ... and as the levels of the segmented reduction see it
struct SegJob {
    void* buckets;
    const uint32_t* offsets;
    void *seg_run, *seg_acc;
    uint32_t *win_s, *win_t;
    ZK_D SegJob(const RJobs& jobs, uint32_t k)
        : buckets(jobs.buckets[k]), offsets(jobs.offsets[k]), seg_run(jobs.seg_run[k]), seg_acc(jobs.seg_acc[k]), win_s(jobs.win_s[k]), win_t(jobs.win_t[k]) {}
};

ZK_D uint64_t partial_slot(uint32_t t, uint32_t ta, uint32_t s, uint32_t L) {
    return (t == ta && (s % L) != 0) ? 2ull * t + 1 : 2ull * t;
}

// shuffle tree over groups of LANES neighbouring lanes (a power of two <= 64): the first lane of a group ends with the group's sum
// (order irrelevant: abelian group).  LANES = 64 is the wave reduction: lane 0 ends with the sum of all 64 lanes
template <class F, int LANES>
ZK_D XYZZu<F> lane_group_sum(XYZZu<F> acc) {
#pragma unroll 1
    for (int d = LANES / 2; d >= 1; d >>= 1) {
        XYZZu<F> o;
#pragma unroll
        for (int i = 0; i < F::NL; ++i) {
            o.x.v[i] = __shfl_down(acc.x.v[i], d, 64);
            o.y.v[i] = __shfl_down(acc.y.v[i], d, 64);
            o.zz.v[i] = __shfl_down(acc.zz.v[i], d, 64);
            o.zzz.v[i] = __shfl_down(acc.zzz.v[i], d, 64);
        }
        acc = XYZZu<F>::add(acc, o);
    }
    return acc;
}

// A bucket whose entries span p >= 2 chunks has exactly p partials at slots known from the offsets (see msm_accumulate).  Small p
// is summed by the kernel that classifies: small(s, ta, p) gets the bucket's first reference, its chunk and p; larger p is queued
// by the lane with `push`.
// queues: q[0] = medium count, q[1] = large count, q[2 ..] medium ids (grow up), q[.. 2+nb) large ids (grow down)
template <class Small>
ZK_D void classify_bucket(const CombineJob& job, uint32_t nb, uint32_t b, bool push, Small small) {
    const uint32_t s = job.offsets[b], e = job.offsets[b + 1];
    if (e == s) return;
    const uint32_t ta = s / job.L;
    const uint32_t p = (e - 1) / job.L - ta + 1;   // p == 1: whole bucket inside one chunk, already complete
    if (p > COMBINE_MEDIUM) {
        if (push) job.q[2 + nb - 1 - atomicAdd(&job.q[1], 1u)] = b;
    } else if (p > COMBINE_SMALL) {
        if (push) job.q[2 + atomicAdd(&job.q[0], 1u)] = b;
    } else if (p > 1) {
        small(s, ta, p);
    }
}

// A window sum leaves the device: words of zero for infinity, the arkworks layout (XYZZ of 4 x SAT words, canonical) otherwise.
// Lane form: the whole point.
template <class F>
ZK_D void put_winsum(uint32_t* out, uint32_t w, const XYZZu<F>& p) {
    uint32_t* o = out + (size_t)w * 4 * F::SAT;
    if (p.is_inf()) {
        for (int i = 0; i < 4 * F::SAT; ++i) o[i] = 0;
    } else {
        p.x.to_sat(o);
        p.y.to_sat(o + F::SAT);
        p.zz.to_sat(o + 2 * F::SAT);
        p.zzz.to_sat(o + 3 * F::SAT);
    }
}
// Quad form: the coordinate of one role.  raw != 0: the internal point form (zero limbs for infinity) instead of SAT words.
template <class F>
ZK_D void put_winsum_q(uint32_t* out, uint32_t w, uint32_t role, const F& v, bool inf, uint32_t raw) {
    if (raw) {
        st_coord<F>(out, w, role, inf ? F::zero() : v);
    } else {
        uint32_t* o = out + (size_t)w * 4 * F::SAT + role * F::SAT;
        if (inf) {
            for (int i = 0; i < F::SAT; ++i) o[i] = 0;
        } else {
            v.to_sat(o);
        }
    }
}

// One lane per bucket (or COMBINE_SG lanes): small buckets are summed here.
// COMBINE_SG lanes cooperate on one small bucket: 4 shortens the dependent chain when the launch is
// latency-bound (1-2 jobs: 0.25 -> 0.19 ms); with more jobs the launch is throughput-bound and the idle
// lanes of the shuffle tree cost more than they save (7 jobs: 1.0 ms at 4 lanes), so 1 is used there.
template <class F, uint32_t COMBINE_SG>
__global__ void __launch_bounds__(128) msm_combine(RJobs jobs, uint32_t nb) {
    const CombineJob job(jobs, blockIdx.y);
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = id / COMBINE_SG, sub = id % COMBINE_SG;
    // every lane stays to the end: the sub-group sums below are wave shuffles
    XYZZu<F> acc = XYZZu<F>::infinity();
    bool mine = false;
    if (b < nb)
        classify_bucket(job, nb, b, sub == 0, [&](uint32_t s, uint32_t ta, uint32_t p) __attribute__((always_inline)) {
            mine = true;
#pragma unroll 1
            for (uint32_t t = ta + sub; t <= ta + p - 1; t += COMBINE_SG)
                acc = XYZZu<F>::add(acc, ld_xyzz<F>(job.part_pt, partial_slot(t, ta, s, job.L)));
        });
    acc = lane_group_sum<F, COMBINE_SG>(acc);
    if (mine && sub == 0) st_xyzz<F>(job.buckets, b, acc);
}

// medium buckets: one wavefront per bucket, lanes stride over its partials, shuffle tree
template <class F>
__global__ void __launch_bounds__(256) msm_combine_wave(RJobs jobs) {
    const CombineJob job(jobs, blockIdx.y);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t nm = job.q[0];
    for (uint32_t h = wave; h < nm; h += n_waves) {
        const uint32_t b = job.q[2 + h];
        const uint32_t s = job.offsets[b], e = job.offsets[b + 1];
        const uint32_t ta = s / job.L, tb = (e - 1) / job.L;
        XYZZu<F> acc = XYZZu<F>::infinity();
        for (uint32_t t = ta + lane; t <= tb; t += 64) acc = XYZZu<F>::add(acc, ld_xyzz<F>(job.part_pt, partial_slot(t, ta, s, job.L)));
        acc = lane_group_sum<F, 64>(acc);
        if (lane == 0) st_xyzz<F>(job.buckets, b, acc);
    }
}

// large buckets (heavily skewed scalars): one 256-lane workgroup per bucket
template <class F>
__global__ void __launch_bounds__(256) msm_combine_block(RJobs jobs, uint32_t nb) {
    extern __shared__ uint4 sh[];
    const CombineJob job(jobs, blockIdx.y);
    const uint32_t u = threadIdx.x;
    const uint32_t nl = job.q[1];
    for (uint32_t h = blockIdx.x; h < nl; h += gridDim.x) {
        const uint32_t b = job.q[2 + nb - 1 - h];
        const uint32_t s = job.offsets[b], e = job.offsets[b + 1];
        const uint32_t ta = s / job.L, tb = (e - 1) / job.L;
        XYZZu<F> acc = XYZZu<F>::infinity();
        for (uint32_t t = ta + u; t <= tb; t += 256) acc = XYZZu<F>::add(acc, ld_xyzz<F>(job.part_pt, partial_slot(t, ta, s, job.L)));
        acc = lane_group_sum<F, 64>(acc);
        __syncthreads();
        if ((u & 63) == 0) st_xyzz<F>(sh, u >> 6, acc);
        __syncthreads();
        if (u == 0) {
            for (uint32_t w = 1; w < 4; ++w) acc = XYZZu<F>::add(acc, ld_xyzz<F>(sh, w));
            st_xyzz<F>(job.buckets, b, acc);
        }
    }
}

// level 1 of the per-window reduction: segment s of window w covers buckets [s*G, (s+1)*G)
//   run = sum B_i ; acc = sum (i+1) * B_i   (i local index)
template <class F>
__global__ void __launch_bounds__(128) msm_seg_reduce(RJobs jobs, MsmGeom g) {
    const SegJob job(jobs, blockIdx.y);
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= g.W * g.ns) return;
    const uint32_t w = id / g.ns, s = id % g.ns;
    const uint32_t G = 1u << g.logG;
    XYZZu<F> run = XYZZu<F>::infinity(), acc = XYZZu<F>::infinity();
    for (int i = (int)G - 1; i >= 0; --i) {
        const uint32_t bi = w * g.B + s * G + (uint32_t)i;
        if (!job.offsets || job.offsets[bi + 1] != job.offsets[bi]) run = XYZZu<F>::add(run, ld_xyzz<F>(job.buckets, bi));
        acc = XYZZu<F>::add(acc, run);
    }
    st_xyzz<F>(job.seg_run, id, run);
    st_xyzz<F>(job.seg_acc, id, acc);
}

// level 2: one 256-lane workgroup per window.
//   S_w = sum_s acc_s + G * sum_s s * run_s
// The window sum leaves the device in the arkworks layout (put_winsum).
// win_t (optional): sum of all buckets of the window, same layout (used when one real window is
// reduced as several "virtual" windows to shorten the dependent-addition chain).
template <class F>
__global__ void __launch_bounds__(256) msm_win_finish(RJobs jobs, MsmGeom g) {
    extern __shared__ uint4 sh[];
    const SegJob job(jobs, blockIdx.y);
    const uint32_t w = blockIdx.x, u = threadIdx.x;
    const uint32_t q = 1u << g.logq;
    typedef XYZZu<F> P;
    P A = P::infinity(), V = P::infinity(), tsum = P::infinity(), R = P::infinity();
    for (int v = (int)q - 1; v >= 0; --v) {
        const uint32_t s = u * q + (uint32_t)v;
        P x = P::infinity();
        if (s < g.ns) {
            x = ld_xyzz<F>(job.seg_run, (uint64_t)w * g.ns + s);
            A = P::add(A, ld_xyzz<F>(job.seg_acc, (uint64_t)w * g.ns + s));
        }
        if (v >= 1) {
            tsum = P::add(tsum, x);
            V = P::add(V, tsum);
        } else {
            R = P::add(tsum, x);
        }
    }
    // Y = A + G * V
    for (uint32_t k = 0; k < g.logG; ++k) V = P::dbl(V);
    P Y = P::add(A, V);
    // suffix sums Q_u = sum_{u' >= u} R_u'  (Hillis-Steele in LDS)
    st_xyzz<F>(sh, u, R);
    for (uint32_t d = 1; d < 256; d <<= 1) {
        __syncthreads();
        P o = P::infinity();
        if (u + d < 256) o = ld_xyzz<F>(sh, u + d);
        __syncthreads();
        R = P::add(R, o);
        st_xyzz<F>(sh, u, R);
    }
    if (job.win_t && u == 0) put_winsum<F>(job.win_t, w, R);
    // Z = Y + (G*q) * Q_u   (u >= 1)
    P Z = Y;
    if (u >= 1) {
        P Qm = R;
        for (uint32_t k = 0; k < g.logG + g.logq; ++k) Qm = P::dbl(Qm);
        Z = P::add(Z, Qm);
    }
    __syncthreads();
    st_xyzz<F>(sh, u, Z);
    for (uint32_t d = 128; d >= 1; d >>= 1) {
        __syncthreads();
        if (u < d) {
            Z = P::add(Z, ld_xyzz<F>(sh, u + d));
            st_xyzz<F>(sh, u, Z);
        }
    }
    if (u == 0) put_winsum<F>(job.win_s, w, Z);
}

// ---- quad-cooperative forms of the three reduction kernels (ecq.cuh): four lanes per dependent chain,
// an addition in 4.5 product-times instead of 13.5.  Same inputs, outputs and arithmetic results.
template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) msm_combine_q(RJobs jobs, uint32_t nb) {
    const CombineJob job(jobs, blockIdx.y);
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = id >> 2, role = id & 3;
    uint32_t s = 0, ta = 0, np = 0;     // np = partials this quad sums itself (0: nothing to do)
    if (b < nb)
        classify_bucket(job, nb, b, role == 0, [&](uint32_t s_, uint32_t ta_, uint32_t p) __attribute__((always_inline)) {
            s = s_;
            ta = ta_;
            np = p;
        });
    // the quads of a wavefront run in lock step to the longest bucket among them; shorter ones add infinity
    uint32_t steps = np;
#pragma unroll
    for (int d = 32; d >= 4; d >>= 1) {
        const uint32_t o = __shfl_xor(steps, d, 64);
        steps = o > steps ? o : steps;
    }
    F acc = F::zero();
#pragma unroll 1
    for (uint32_t k = 0; k < steps; ++k) {
        F v = F::zero();
        if (k < np) v = ld_coord<F>(job.part_pt, partial_slot(ta + k, ta, s, job.L), role);
        acc = qadd<F>(acc, v, role);
    }
    if (np) st_coord<F>(job.buckets, b, role, acc);
}

template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) msm_seg_reduce_q(RJobs jobs, MsmGeom g) {
    const SegJob job(jobs, blockIdx.y);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t id = tid >> 2, role = tid & 3;
    const bool live = id < g.W * g.ns;              // no early exit: wave shuffles inside qadd
    const uint32_t w = live ? id / g.ns : 0, sg = live ? id % g.ns : 0;
    const uint32_t G = 1u << g.logG;
    F run = F::zero(), acc = F::zero();
    // the bucket of the NEXT step (its two offsets, then its coordinate: two dependent round trips) is requested before the two
    // additions of the current one; at one to two wavefronts per SIMD nothing else would hide them
    auto bucket = [&](int i) -> F {
        const uint32_t bi = w * g.B + sg * G + (uint32_t)i;
        F v = F::zero();
        if (live && (!job.offsets || job.offsets[bi + 1] != job.offsets[bi])) v = ld_coord<F>(job.buckets, bi, role);
        return v;
    };
    F nv = bucket((int)G - 1);
#pragma unroll 1
    for (int i = (int)G - 1; i >= 0; --i) {
        const F v = nv;
        if (i > 0) nv = bucket(i - 1);
        run = qadd<F>(run, v, role);
        acc = qadd<F>(acc, run, role);
    }
    if (live) {
        st_coord<F>(job.seg_run, id, role, run);
        st_coord<F>(job.seg_acc, id, role, acc);
    }
}

// msm_win_finish for logq == 0 (one segment per chain): 4 * ns lanes per workgroup, ns <= 256
// raw != 0: the two sums stay on the device in the internal point form (the "buckets" of the next reduction level);
// raw == 0: arkworks layout for the host, as msm_win_finish.
// MAXT = lanes per workgroup the instance is built for.  512 (up to 128 chains: every launch of the window-table path) leaves the
// register file to two wavefronts per SIMD and nothing spills; built for 1024 lanes -- four wavefronts per SIMD, 128 registers --
// the same code spilled 162 registers to 332 bytes of scratch per lane (the form every launch used before round 4; only the
// per-window path's 256-chain geometry still needs it).
template <class F, int MAXT>
__global__ void __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(MAXT / 256, MAXT / 256))) msm_win_finish_q(RJobs jobs, MsmGeom g, uint32_t raw) {
    extern __shared__ uint4 sh[];
    const SegJob job(jobs, blockIdx.y);
    const uint32_t w = blockIdx.x, u = threadIdx.x >> 2, role = threadIdx.x & 3;
    const uint32_t T = blockDim.x >> 2;             // chains = power of two >= ns
    F R = F::zero(), Y = F::zero();
    if (u < g.ns) {
        R = ld_coord<F>(job.seg_run, (uint64_t)w * g.ns + u, role);
        Y = ld_coord<F>(job.seg_acc, (uint64_t)w * g.ns + u, role);
    }
    // suffix sums Q_u = sum_{u' >= u} R_u'  (Hillis-Steele in LDS)
    st_coord<F>(sh, u, role, R);
    for (uint32_t d = 1; d < T; d <<= 1) {
        __syncthreads();
        F o = F::zero();
        if (u + d < T) o = ld_coord<F>(sh, u + d, role);
        __syncthreads();
        R = qadd<F>(R, o, role);
        st_coord<F>(sh, u, role, R);
    }
    const bool r_inf = quad_is_inf(R, role);
    if (job.win_t && u == 0) put_winsum_q<F>(job.win_t, w, role, R, r_inf, raw);
    // Z = Y + G * Q_u   (u >= 1)
    F Qm = R;
    for (uint32_t k = 0; k < g.logG; ++k) Qm = qdbl<F>(Qm, role);
    F Z = qadd<F>(Y, u >= 1 ? Qm : F::zero(), role);
    __syncthreads();
    st_coord<F>(sh, u, role, Z);
    for (uint32_t d = T / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (u < d) {                                 // quad-uniform: all four lanes of a chain agree
            Z = qadd<F>(Z, ld_coord<F>(sh, u + d, role), role);
            st_coord<F>(sh, u, role, Z);
        }
    }
    const bool z_inf = quad_is_inf(Z, role);
    if (u == 0) put_winsum_q<F>(job.win_s, w, role, Z, z_inf, raw);
}

// Work-efficient level of the wide reduction: a node (run, acc) stands for m = 2^logm consecutive buckets,
//   run = sum B_i,  acc = sum (i + 1) B_i   (i local to the node);
// K = 2^logk neighbouring nodes make one node of K*m buckets:  run' = sum_j run_j,  acc' = sum_j acc_j + m * sum_j j * run_j
// -- 3 additions per child instead of the log2(chains) of the Hillis-Steele scan in msm_win_finish_q, which is what made
// 2^17 level-1 nodes per job (window tables with c = 20) cost more than the level below them.  One quad per output node.
// in: jobs.seg_run / seg_acc (n_out * K nodes);  out: jobs.win_s (run') / jobs.win_t (acc'), internal point form.
template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) msm_node_reduce_q(RJobs jobs, uint32_t n_out, uint32_t logk, uint32_t logm) {
    const SegJob job(jobs, blockIdx.y);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t id = tid >> 2, role = tid & 3;
    const bool live = id < n_out;                  // no early exit: wave shuffles inside qadd
    const uint32_t K = 1u << logk;
    const uint64_t first = (uint64_t)(live ? id : 0) * K;
    F run = F::zero(), wsum = F::zero(), asum = F::zero();
#pragma unroll 1
    for (int j = (int)K - 1; j >= 1; --j) {
        run = qadd<F>(run, live ? ld_coord<F>(job.seg_run, first + (uint32_t)j, role) : F::zero(), role);
        wsum = qadd<F>(wsum, run, role);           // after the loop: sum_j j * run_j
        asum = qadd<F>(asum, live ? ld_coord<F>(job.seg_acc, first + (uint32_t)j, role) : F::zero(), role);
    }
    run = qadd<F>(run, live ? ld_coord<F>(job.seg_run, first, role) : F::zero(), role);
    asum = qadd<F>(asum, live ? ld_coord<F>(job.seg_acc, first, role) : F::zero(), role);
    for (uint32_t t = 0; t < logm; ++t) wsum = qdbl<F>(wsum, role);
    asum = qadd<F>(asum, wsum, role);
    if (live) {
        st_coord<F>(job.win_s, id, role, run);
        st_coord<F>(job.win_t, id, role, asum);
    }
}

// element-wise sum over the ranks of every job's 2 VW virtual-window sums (ranks x n_jobs x 2 VW points as the all-gather leaves
// them) -> n_jobs x 2 VW points in the arkworks layout in pinned host memory, where the single-GPU path's last reduction kernel
// puts them.  Q = 2^logq quads share one sum: quad j adds the ranks j, j + Q, ... (ranks / Q - 1 dependent additions), an LDS tree
// adds the Q partial sums (logq more): 3 dependent additions for 8 ranks instead of 7 -- the launch is latency-shaped (2 VW n_jobs
// points, at most a few thousand quads), so the chain is what it costs.
template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) g1_sum_winsums_q(const void* all, uint32_t ranks, uint32_t n_pts /* n_jobs * 2 VW */,
                                                                                                     uint32_t logq, uint32_t* out_sat) {
    extern __shared__ uint4 sh[];
    const uint32_t Q = 1u << logq;
    const uint32_t quad = threadIdx.x >> 2, role = threadIdx.x & 3;
    const uint32_t per_block = (blockDim.x >> 2) >> logq;                      // points per workgroup
    const uint32_t k = blockIdx.x * per_block + (quad >> logq), j = quad & (Q - 1);
    const bool live = k < n_pts;                   // no early exit: wave shuffles inside qadd, barriers below
    F acc = F::zero();
#pragma unroll 1
    for (uint32_t r = j; r < ranks; r += Q) acc = qadd<F>(acc, live ? ld_coord<F>(all, (uint64_t)r * n_pts + k, role) : F::zero(), role);
    for (uint32_t d = Q >> 1; d >= 1; d >>= 1) {
        st_coord<F>(sh, quad, role, acc);
        __syncthreads();
        const F o = j < d ? ld_coord<F>(sh, quad + d, role) : F::zero();
        __syncthreads();
        acc = qadd<F>(acc, o, role);               // quads with j >= d add the point at infinity: uniform control flow
    }
    const bool inf = quad_is_inf(acc, role);
    if (live && j == 0) put_winsum_q<F>(out_sat, k, role, acc, inf, 0u);
}

// ---------------------------------------------------------------------------------------- host side
// msm_win_finish_q with `chains` (a power of two <= 256) chains of four lanes per workgroup
template <class F>
int launch_win_finish_q(dim3 grid, uint32_t chains, hipStream_t st, const RJobs& jobs, const MsmGeom& g, uint32_t raw) {
    const size_t shmem = (size_t)chains * Store<F>::POINT_BYTES;
    if (chains <= 128) {
        if (shmem > 48 * 1024)
            ZK_HIP_TRY(hipFuncSetAttribute((const void*)msm_win_finish_q<F, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL((msm_win_finish_q<F, 512>), grid, dim3(4 * chains), shmem, st, jobs, g, raw);
    } else if (chains <= 256) {
        if (shmem > 48 * 1024)
            ZK_HIP_TRY(hipFuncSetAttribute((const void*)msm_win_finish_q<F, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL((msm_win_finish_q<F, 1024>), grid, dim3(4 * chains), shmem, st, jobs, g, raw);
    } else {
        return ZK_ERR_UNSUPPORTED;
    }
    return ZK_OK;
}

constexpr int LANE_T = 128;       // lanes per workgroup of the one-lane-per-item kernels (msm_combine, msm_seg_reduce)

template <class F, uint32_t SG>
void launch_combine_lanes(const RJobs& jobs, uint32_t n_jobs, uint32_t nb, hipStream_t st) {
    unsigned blocks = (unsigned)(((uint64_t)nb * SG + LANE_T - 1) / LANE_T);
    hipLaunchKernelGGL((msm_combine<F, SG>), dim3(blocks, n_jobs), dim3(LANE_T), 0, st, jobs, nb);
}
// chunk-edge partials -> buckets: the small buckets and the two queues, then the queued medium and large ones.  The two callers
// choose differently and say so: `quad` lets a launch of one or two jobs take msm_combine_q (without it: four lanes per bucket);
// `sg_many` is the lanes per small bucket when the launch has more jobs.
template <class F>
void launch_combine(const RJobs& jobs, uint32_t n_jobs, uint32_t nb, bool quad, int sg_many, hipStream_t st) {
    if (n_jobs <= 2 && quad) {
        unsigned blocks = (unsigned)(((uint64_t)nb * 4 + 255) / 256);
        hipLaunchKernelGGL(msm_combine_q<F>, dim3(blocks, n_jobs), dim3(256), 0, st, jobs, nb);
    } else if (n_jobs <= 2 || sg_many == 4) {
        launch_combine_lanes<F, 4>(jobs, n_jobs, nb, st);
    } else if (sg_many == 2) {
        launch_combine_lanes<F, 2>(jobs, n_jobs, nb, st);
    } else {
        launch_combine_lanes<F, 1>(jobs, n_jobs, nb, st);
    }
    hipLaunchKernelGGL(msm_combine_wave<F>, dim3(256, n_jobs), dim3(256), 0, st, jobs);
    hipLaunchKernelGGL(msm_combine_block<F>, dim3(64, n_jobs), dim3(256), 4 * Store<F>::POINT_BYTES, st, jobs, nb);
}

// the quad forms of a level: msm_seg_reduce_q, then msm_win_finish_q with the segments of a window rounded up to a power of two chains
template <class F>
int seg_reduce_finish_q(const RJobs& jobs, uint32_t n_jobs, const MsmGeom& g, uint32_t raw, hipStream_t st) {
    unsigned sblocks = (unsigned)(((uint64_t)g.W * g.ns * 4 + 255) / 256);
    hipLaunchKernelGGL(msm_seg_reduce_q<F>, dim3(sblocks, n_jobs), dim3(256), 0, st, jobs, g);
    uint32_t chains = 1;
    while (chains < g.ns) chains <<= 1;
    return launch_win_finish_q<F>(dim3(g.W, n_jobs), chains, st, jobs, g, raw);
}

// combine + segmented reduction of n_jobs MSMs that share the geometry (nb buckets, reduction geometry gr)
template <class F>
int queue_reduce(zk_ctx* c, const RJobs& jobs, uint32_t n_jobs, uint32_t nb, const MsmGeom& gr, hipStream_t st, bool queues_cleared = false,
                 uint32_t raw = 0 /* 1: the window sums stay in the internal point form (device buffers), quad geometry only */) {
    ProfScope ps(c, "msm_reduce", st);
    int rc;
    if (!queues_cleared)
        for (uint32_t k = 0; k < n_jobs; ++k) ZK_HIP_TRY(hipMemsetAsync(jobs.q[k], 0, 8, st));
    // quad-cooperative kernels where the geometry allows (one segment per chain, <= 256 chains per window)
    const bool quad = gr.logq == 0 && gr.ns <= 256;
    // lanes per small bucket when the launch has many jobs.  Option "combine_sg": tuning hook (profiles/r03/r03_notes.md)
    launch_combine<F>(jobs, n_jobs, nb, quad, c->tune.combine_sg ? c->tune.combine_sg : 1, st);
    if (quad) {
        if ((rc = seg_reduce_finish_q<F>(jobs, n_jobs, gr, raw, st))) return rc;
    } else {
        if (raw) return ZK_ERR_UNSUPPORTED;
        unsigned sblocks = (gr.W * gr.ns + LANE_T - 1) / LANE_T;
        hipLaunchKernelGGL(msm_seg_reduce<F>, dim3(sblocks, n_jobs), dim3(LANE_T), 0, st, jobs, gr);
        const size_t shmem = 256 * Store<F>::POINT_BYTES;
        if (shmem > 48 * 1024)
            ZK_HIP_TRY(hipFuncSetAttribute((const void*)msm_win_finish<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(msm_win_finish<F>, dim3(gr.W, n_jobs), dim3(256), shmem, st, jobs, gr);
    }
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// Reduction for window tables with c > 16 (nb = 2^(c-1) >= 2^16 shared buckets), all on the device:
//   level 1  msm_seg_reduce      one LANE per node of 4 buckets: with >= 16 Ki nodes per job the launch is throughput-bound,
//                                where the single-lane group law costs 13.5 product-times per addition against the quad form's 18
//   level 2  msm_node_reduce_q   4 nodes -> one node of 16 buckets, 3 additions per child (quads)
//   level 3  msm_win_finish_q    VW = nb / 2048 virtual windows of 128 nodes -> S_v = sum_l (l+1) B_{v,l},  T_v = sum_l B_{v,l}, kept on
//                                the device in the internal point form
//   level 4  msm_seg_reduce_q + msm_win_finish_q over the two arrays S and T of every job (2 n_jobs "jobs", every element present):
//                                sum_v S_v,  K = sum_v (v+1) T_v,  sum_v T_v  -> pinned host memory, arkworks layout
//   host     total = sum_v S_v + 2048 * (K - sum_v T_v)      (bucket j = 2048 v + l has weight j + 1)
template <class F>
int queue_reduce_wide(zk_ctx* c, const RJobs& jobs, uint32_t n_jobs, uint32_t nb, void* const* d_vw, void* const* d_seg3, void* const* d_seg2,
                      char* h_out, size_t h_stride, hipStream_t st) {
    constexpr size_t PT = Store<F>::POINT_BYTES;
    ProfScope ps(c, "msm_reduce", st);
    int rc;
    const uint32_t VW = nb / WIDE_VB;
    if (VW == 0 || VW > 2048) return ZK_ERR_UNSUPPORTED;
    // chunk-edge partials -> buckets (queues cleared by the job's sort).  Whatever the level geometries below say, one or two jobs
    // take the quad form, and "combine_sg" is not consulted: one lane per small bucket with more jobs
    launch_combine<F>(jobs, n_jobs, nb, true, 1, st);
    const uint32_t n1 = nb >> WIDE_LOGG1, n2 = n1 >> WIDE_LOGK2;
    {   // level 1: flat over all buckets (one "window" of nb buckets, nodes of 4)
        const MsmGeom g1 = level_geom(1, nb, WIDE_LOGG1);
        unsigned sblocks = (unsigned)(((uint64_t)n1 + LANE_T - 1) / LANE_T);
        hipLaunchKernelGGL(msm_seg_reduce<F>, dim3(sblocks, n_jobs), dim3(LANE_T), 0, st, jobs, g1);
    }
    RJobs j2 = jobs;      // level 2: seg_run / seg_acc (n1 nodes) -> d_seg2 (n2 nodes: run | acc)
    for (uint32_t k = 0; k < n_jobs; ++k) {
        j2.win_s[k] = (uint32_t*)d_seg2[k];
        j2.win_t[k] = (uint32_t*)((char*)d_seg2[k] + (size_t)n2 * PT);
    }
    {
        unsigned blocks = (unsigned)(((uint64_t)n2 * 4 + 255) / 256);
        hipLaunchKernelGGL(msm_node_reduce_q<F>, dim3(blocks, n_jobs), dim3(256), 0, st, j2, n2, WIDE_LOGK2, WIDE_LOGG1);
    }
    RJobs j3 = jobs;      // level 3: virtual windows of 128 level-2 nodes (16 buckets each)
    const MsmGeom gv = level_geom(VW, WIDE_VB, WIDE_LOGG1 + WIDE_LOGK2);
    for (uint32_t k = 0; k < n_jobs; ++k) {
        j3.seg_run[k] = d_seg2[k];
        j3.seg_acc[k] = (char*)d_seg2[k] + (size_t)n2 * PT;
        j3.win_s[k] = (uint32_t*)d_vw[k];
        j3.win_t[k] = (uint32_t*)((char*)d_vw[k] + (size_t)VW * PT);
    }
    if ((rc = launch_win_finish_q<F>(dim3(VW, n_jobs), WIDE_CHAINS, st, j3, gv, 1u))) return rc;
    // level 4: the VW pairs (S_v, T_v) of every job
    const MsmGeom g4 = level_geom(1, VW, VW <= 4 ? 0 : VW <= 1024 ? 2 : 3);
    if (g4.ns == 0 || g4.ns > 256) return ZK_ERR_UNSUPPORTED;
    RJobs j4;
    memset(&j4, 0, sizeof j4);
    const size_t PHB = h_stride / 4;      // bytes of one host point
    for (uint32_t k = 0; k < n_jobs; ++k)
        for (uint32_t a = 0; a < 2; ++a) {
            const uint32_t j = 2 * k + a;
            j4.buckets[j] = (char*)d_vw[k] + (size_t)a * VW * PT;
            j4.offsets[j] = nullptr;
            j4.seg_run[j] = (char*)d_seg3[k] + (size_t)a * 2 * g4.ns * PT;
            j4.seg_acc[j] = (char*)d_seg3[k] + ((size_t)a * 2 + 1) * g4.ns * PT;
            j4.win_s[j] = (uint32_t*)(h_out + (size_t)k * h_stride + (size_t)a * 2 * PHB);
            j4.win_t[j] = (uint32_t*)(h_out + (size_t)k * h_stride + ((size_t)a * 2 + 1) * PHB);
        }
    if ((rc = seg_reduce_finish_q<F>(j4, 2 * n_jobs, g4, 0u, st))) return rc;
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// fused reduction of the jobs mbs[0..n_jobs) (same geometry); their virtual-window sums land in h_win (n_jobs x win_bytes, pinned host
// memory, arkworks layout) or, with d_winsums, stay on the device in the internal form at d_winsums[k]
template <class Cv>
int pre_queue_reduce(zk_ctx* c, const PrePlan* pls, MsmBufs* const* mbs, uint32_t n_jobs, void* h_win, hipStream_t st, void* const* d_winsums) {
    typedef typename Cv::FqU F;
    constexpr size_t PT = Store<F>::POINT_BYTES;
    RJobs jobs;
    memset(&jobs, 0, sizeof jobs);
    const PrePlan& p0 = pls[0];
    if (d_winsums && !pre_partial_dev_ok(p0)) return ZK_ERR_UNSUPPORTED;     // checked by the callers before anything is queued
    const size_t n_seg = p0.wide_red ? (size_t)(p0.g.B >> WIDE_LOGG1) : (size_t)p0.gv.W * p0.gv.ns;
    for (uint32_t k = 0; k < n_jobs; ++k) {
        const MsmBufs& mb = *mbs[k];
        // the window sums (a few KiB per job) are written by the last kernel straight into the pinned host
        // buffer (hipHostMalloc memory is device-visible): no copy launches at the tail of the call
        uint32_t* win_s = (uint32_t*)((char*)h_win + (size_t)k * p0.win_bytes);
        uint32_t* win_t = win_s + (size_t)p0.gv.W * 4 * F::SAT;
        if (d_winsums) {
            win_s = (uint32_t*)d_winsums[k];                                        // S_v | T_v, internal form, straight into the
            win_t = (uint32_t*)((char*)d_winsums[k] + (size_t)p0.gv.W * PT);        // caller's buffer (the collective's send buffer)
        }
        // L, lanes: the plan the accumulation really ran with (pre_queue_accumulate), not a re-derived one
        set_rjob<F>(jobs, k, mb, PRE_Q_OFF, n_seg, win_s, win_t, mb.acc_chunk_l, mb.acc_n_lanes, p0.g1.nb);
    }
    // the queue counters were cleared by the job's sort (its digit kernel: reset_job_counters / the memset of the fallback sort)
    if (p0.wide_red) {
        void* d_vw[MAX_JOBS];
        void* d_seg3[MAX_JOBS];
        void* d_seg2[MAX_JOBS];
        for (uint32_t k = 0; k < n_jobs; ++k) {
            d_vw[k] = mbs[k]->win.p;
            d_seg3[k] = mbs[k]->seg3.p;
            d_seg2[k] = mbs[k]->seg2.p;
        }
        return queue_reduce_wide<F>(c, jobs, n_jobs, p0.g1.nb, d_vw, d_seg3, d_seg2, (char*)h_win, p0.win_bytes, st);
    }
    // on the device the window sums ARE the result: zk_g1_sum_winsums_dev adds the ranks' and the host combines
    return queue_reduce<F>(c, jobs, n_jobs, p0.g1.nb, p0.gv, st, true, d_winsums ? 1u : 0u);
}

}  // namespace

int ZK_SYM(queue_reduce)(zk_ctx* c, const RJobs& jobs, uint32_t n_jobs, uint32_t nb, const MsmGeom& gr, hipStream_t st, bool queues_cleared, uint32_t raw) {
    return queue_reduce<CurveSel::FqU>(c, jobs, n_jobs, nb, gr, st, queues_cleared, raw);
}
int ZK_SYM(pre_queue_reduce)(zk_ctx* c, const PrePlan* pls, MsmBufs* const* mbs, uint32_t n_jobs, void* h_win, hipStream_t st, void* const* d_winsums) {
    return pre_queue_reduce<CurveSel>(c, pls, mbs, n_jobs, h_win, st, d_winsums);
}
int ZK_SYM(queue_sum_winsums)(zk_ctx* c, const void* d_all, uint32_t ranks, uint32_t n_pts, void* h_out, hipStream_t st) {
    typedef CurveSel::FqU F;
    ProfScope ps(c, "msm_sum_winsums", st);
    uint32_t logq = 0;                                    // quads per sum: half the ranks (rounded up to a power of two), at most 16
    while (logq < 4 && (2u << logq) < ranks) ++logq;
    const uint32_t per_block = 64u >> logq;
    hipLaunchKernelGGL(g1_sum_winsums_q<F>, dim3((n_pts + per_block - 1) / per_block), dim3(256), 64 * Store<F>::POINT_BYTES, st, d_all, ranks, n_pts, logq, (uint32_t*)h_out);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}
