// ipa_pc::setup on the device: the committer key's generators, hashed to the curve.  The rule is h2c.cuh's (its host
// statement: ark_plonk_amd/ipa.py); the field is the device form of the MSM base field (fields.cuh); the lift of an x to a point --
// conversion, x^3 + b, square root, sign rule -- is g1_lift.cuh's, shared with g1_decompress (verify.hip); the group law is ecu.cuh's
// and the normalisation block_inverse.cuh + to_affine_given: nothing of the arithmetic is restated here.
//
// h2c_search: a wavefront owns a contiguous chunk of H2C_CHUNK indices and a wave-uniform counter `next`.  A lane without an index
// takes the next one of the chunk (ballot of the lanes that need work, the lane's rank in that mask, next += popcount: no atomics, no
// LDS) and hashes until a digest passes the checks that need no field arithmetic.  Then the WHOLE wavefront runs one square-root round
// -- x^3 + b to the power (q + 1) / 4, a constant of the curve, so every lane takes the same branches -- and a lane whose candidate
// is a residue writes its affine point to the row of its index and is free again.  Lanes leave the lock-step only in the hash loop.
// A per-lane `while` would make a wavefront run as many roots as its unluckiest index needs (about 7 for 64 lanes at p = 1/2) where
// the indices need about 2 each; here the excess is the tail of a chunk alone, when fewer than 64 indices are left in flight.
//
// g1_clear_cofactor: the second kernel, in place over the candidates: one uniform double-and-add by the curve's cofactor per lane, one
// field inversion per workgroup.  Not launched on BN254 (cofactor 1).
//
// g1_from_random_bytes: the same rule applied to caller-supplied byte strings, one lane per string, a status per string: what makes the
// rule's corner cases testable without hash preimages.
//
// Built once for both curves; with -DZK_CURVE_SEL=<0|1> only that curve's kernels are instantiated (tests/test_ipa_setup_build.py
// compiles each on its own).
#include "api_internal.h"
#include "block_inverse.cuh"
#include "g1_lift.cuh"
#include "h2c.cuh"

namespace {

static_assert(H2C_BLAKE2S == ZK_H2C_BLAKE2S && H2C_BLAKE2B == ZK_H2C_BLAKE2B, "h2c.cuh numbers the digests as the C ABI does");
constexpr uint32_t H2C_WAVE = 64;
constexpr uint32_t H2C_CHUNK = ZK_H2C_CHUNK;               // indices per wavefront (why 512)
constexpr uint32_t CLR_T = 128;                            // lanes = points per batched inversion of the cofactor kernel
constexpr uint32_t FRB_T = 128;

#if defined(ZK_CURVE_SEL)
template <class Cv>
constexpr bool h2c_built = std::is_same<Cv, CurveBls>::value == (ZK_CURVE_SEL == 0);
#else
template <class Cv>
constexpr bool h2c_built = true;
#endif

// GroupAffine::zero() = (0, 1); a row without a point: all-zero words
template <class Cv>
ZK_D void h2c_write_infinity(uint32_t* dst) {
    constexpr int SAT = Cv::FqU::SAT;
    for (int k = 0; k < SAT; ++k) {
        dst[k] = 0;
        dst[SAT + k] = Cv::FqP::R(k);
    }
}
template <class Cv>
ZK_D void h2c_write_null(uint32_t* dst) {
    for (int k = 0; k < 2 * Cv::FqU::SAT; ++k) dst[k] = 0;
}

ZK_D uint8_t h2c_status_of(int cls) {
    return cls == H2C_X_NOT_REDUCED ? ZK_G1_X_NOT_REDUCED : cls == H2C_BAD_FLAGS ? ZK_G1_BAD_FLAGS : ZK_G1_INF_FLAG_X_NONZERO;
}

// ------------------------------------------------------------------------------------------------------------ candidate search
template <class Cv, int DIGEST>
__global__ void __launch_bounds__(H2C_WAVE) h2c_search(uint64_t first_index, uint64_t n, uint32_t max_tries, uint32_t* out_xy, uint8_t* out_inf,
                                                       uint32_t* tries_out, uint8_t* status, uint32_t* wave_rounds) {
    typedef typename Cv::FqU F;
    typedef typename Cv::FqP FqP;
    constexpr int SAT = F::SAT;
    const uint32_t lane = threadIdx.x;
    uint64_t next = (uint64_t)blockIdx.x * H2C_CHUNK;                    // wave-uniform: the first index of the chunk nobody has taken
    const uint64_t end = next + H2C_CHUNK < n ? next + H2C_CHUNK : n;    // next <= end <= n: every row written below is a row of the call
    uint64_t idx = 0;                     // the lane's index, relative to first_index
    uint32_t tries = 0, flags = 0, rounds = 0;
    bool active = false, have = false;    // active: holds an unresolved index; have: w is a candidate x that awaits its square root
    uint32_t w[SAT];
#pragma unroll
    for (int k = 0; k < SAT; ++k) w[k] = 0;

    auto resolve = [&](uint8_t st, uint8_t inf) {
        out_inf[idx] = inf;
        status[idx] = st;
        if (tries_out) tries_out[idx] = tries;
        active = false;
    };
    for (;;) {
        // ---- every lane that can have a candidate gets one
        for (;;) {
            const uint64_t need = __ballot(!active);
            if (!active) {
                const uint64_t cand = next + __popcll(need & (((uint64_t)1 << lane) - 1));
                if (cand < end) {
                    idx = cand;
                    tries = 0;
                    active = true;
                }
            }
            next += __popcll(need);
            if (next > end) next = end;
            if (active && !have) {
                while (tries < max_tries) {
                    h2c_generator_digest<DIGEST>(first_index + idx, tries, w);
                    ++tries;
                    const int cls = h2c_classify<FqP>(w, flags);
                    if (cls == H2C_X_ON_CURVE_PENDING) {
                        have = true;
                        break;
                    }
                    if (cls == H2C_INFINITY) {                           // its generator is infinity too
                        h2c_write_infinity<Cv>(out_xy + idx * 2 * SAT);
                        resolve(ZK_G1_OK, 1);
                        break;
                    }
                }
                if (active && !have) {                                   // out of attempts: a null row, never a hang
                    h2c_write_null<Cv>(out_xy + idx * 2 * SAT);
                    resolve(ZK_H2C_EXHAUSTED, 0);
                }
            }
            if (!(__any(!active) && next < end)) break;                  // a lane is free and the chunk has indices left: again
        }
        if (!__any(have)) break;                                         // nothing in flight: the chunk is done
        // ---- ONE square-root round for the wavefront (a lane without a candidate computes on x = 0 and drops the result)
        ++rounds;
        F x, rhs, y;
        g1_curve_rhs<Cv>(w, x, rhs);
        const bool square = g1_sqrt<Cv>(rhs, y);
        if (have && square) {
            g1_write_lifted<Cv>(x, g1_pick_root<Cv>(y, (flags & 2u) != 0), out_xy + idx * 2 * SAT);
            resolve(ZK_G1_OK, 0);
        }
        have = false;
#pragma unroll
        for (int k = 0; k < SAT; ++k) w[k] = 0;
    }
    if (wave_rounds && lane == 0) wave_rounds[blockIdx.x] = rounds;
}

// ------------------------------------------------------------------------------------------------------------ cofactor clearing
template <class Cv>
__global__ void __launch_bounds__(CLR_T) g1_clear_cofactor(uint64_t n, uint32_t* xy, uint8_t* inf, const uint8_t* status) {
    typedef typename Cv::FqU F;
    typedef XYZZu<F> P;
    constexpr int SAT = F::SAT;
    __shared__ BlockInverseLds<F, CLR_T> lds;
    const uint64_t i = (uint64_t)blockIdx.x * CLR_T + threadIdx.x;
    const bool have = i < n && status[i] == ZK_G1_OK && !inf[i];
    uint32_t* row = xy + i * 2 * SAT;                                     // used under `have` only
    AffineU<F> q;
    q.x = F::zero();
    q.y = F::zero();
    if (have) {
        q.x = F::from_sat(row);
        q.y = F::from_sat(row + SAT);
    }
    // double-and-add from the top bit, as G1Host::scalar_mul: the cofactor is a constant, so every lane walks one loop
    P acc = P::infinity();
    for (int limb = 3; limb >= 0; --limb) {
        const uint32_t word = h2c_bls12_381_cofactor_word(limb);
        for (int bit = 31; bit >= 0; --bit) {
            acc = P::dbl(acc);
            if (have && ((word >> bit) & 1u)) acc = P::madd(acc, q);
        }
    }
    const bool fin = have && !acc.is_inf();
    if (!fin) acc.zzz = F::one();                                        // a lane with no finite result enters the product as 1
    const F zi3 = block_inverse(acc.zzz, lds);                           // 1 / ZZZ
    if (!have) return;
    if (fin) {
        AffineU<F> a;
        acc.to_affine_given(zi3, a);
        a.x.to_sat(row);
        a.y.to_sat(row + SAT);
    } else {                                                             // a point of the cofactor's torsion
        h2c_write_infinity<Cv>(row);
        inf[i] = 1;
    }
}

// ------------------------------------------------------------------------------------------------------------ from_random_bytes
template <class Cv>
__global__ void __launch_bounds__(FRB_T) g1_from_random_bytes(const uint8_t* bytes, uint32_t byte_len, uint64_t n, uint32_t* out_xy,
                                                              uint8_t* out_inf, uint8_t* status) {
    typedef typename Cv::FqU F;
    typedef typename Cv::FqP FqP;
    constexpr int SAT = F::SAT;
    constexpr uint32_t G = 4 * SAT;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* src = bytes + i * byte_len;
    uint32_t* dst = out_xy + i * 2 * SAT;
    uint32_t w[SAT], flags;
#pragma unroll
    for (int k = 0; k < SAT; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if ((uint32_t)(4 * k + b) < byte_len) v |= (uint32_t)src[4 * k + b] << (8 * b);     // min(len, G) bytes, the rest of the buffer zero
        w[k] = v;
    }
    static_assert(G == 4 * SAT, "the buffer of from_random_bytes fills the words of a base-field element");
    const int cls = h2c_classify<FqP>(w, flags);
    if (cls == H2C_INFINITY) {
        h2c_write_infinity<Cv>(dst);
        out_inf[i] = 1;
        status[i] = ZK_G1_OK;
        return;
    }
    out_inf[i] = 0;
    if (cls != H2C_X_ON_CURVE_PENDING) {
        h2c_write_null<Cv>(dst);
        status[i] = h2c_status_of(cls);
        return;
    }
    F x, rhs, y;
    g1_curve_rhs<Cv>(w, x, rhs);
    if (!g1_sqrt<Cv>(rhs, y)) {
        h2c_write_null<Cv>(dst);
        status[i] = ZK_G1_NOT_ON_CURVE;
        return;
    }
    g1_write_lifted<Cv>(x, g1_pick_root<Cv>(y, (flags & 2u) != 0), dst);
    status[i] = ZK_G1_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ host
template <class Cv>
int clear_cofactor_impl(zk_ctx* c, size_t n, void* d_xy, void* d_inf, const void* d_status) {
    if constexpr (!h2c_built<Cv>) {
        return ZK_ERR_UNSUPPORTED;
    } else if constexpr (std::is_same<Cv, CurveBn>::value) {
        return ZK_OK;                                                    // cofactor 1
    } else {
        ProfScope ps(c, "g1_clear_cofactor");
        hipLaunchKernelGGL(g1_clear_cofactor<Cv>, dim3(blocks_of(n, CLR_T)), dim3(CLR_T), 0, c->stream, (uint64_t)n, (uint32_t*)d_xy, (uint8_t*)d_inf,
                           (const uint8_t*)d_status);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    }
}

template <class Cv>
int sample_impl(zk_ctx* c, int digest_id, uint64_t first_index, size_t n, uint32_t max_tries, void* d_out_xy, void* d_out_inf, void* d_tries,
                void* d_status, void* d_wave_rounds) {
    if constexpr (!h2c_built<Cv>) {
        return ZK_ERR_UNSUPPORTED;
    } else {
        {
            ProfScope ps(c, "h2c_search");
            const dim3 grid(blocks_of(n, H2C_CHUNK)), block(H2C_WAVE);
            if (digest_id == ZK_H2C_BLAKE2S)
                hipLaunchKernelGGL((h2c_search<Cv, ZK_H2C_BLAKE2S>), grid, block, 0, c->stream, first_index, (uint64_t)n, max_tries, (uint32_t*)d_out_xy,
                                   (uint8_t*)d_out_inf, (uint32_t*)d_tries, (uint8_t*)d_status, (uint32_t*)d_wave_rounds);
            else
                hipLaunchKernelGGL((h2c_search<Cv, ZK_H2C_BLAKE2B>), grid, block, 0, c->stream, first_index, (uint64_t)n, max_tries, (uint32_t*)d_out_xy,
                                   (uint8_t*)d_out_inf, (uint32_t*)d_tries, (uint8_t*)d_status, (uint32_t*)d_wave_rounds);
            ZK_HIP_TRY(hipGetLastError());
        }
        return clear_cofactor_impl<Cv>(c, n, d_out_xy, d_out_inf, d_status);
    }
}

template <class Cv>
int from_random_bytes_impl(zk_ctx* c, const void* d_bytes, size_t byte_len, size_t n, int clear_cofactor, void* d_out_xy, void* d_out_inf,
                           void* d_status) {
    if constexpr (!h2c_built<Cv>) {
        return ZK_ERR_UNSUPPORTED;
    } else {
        {
            ProfScope ps(c, "g1_from_random_bytes");
            hipLaunchKernelGGL(g1_from_random_bytes<Cv>, dim3(blocks_of(n, FRB_T)), dim3(FRB_T), 0, c->stream, (const uint8_t*)d_bytes, (uint32_t)byte_len,
                               (uint64_t)n, (uint32_t*)d_out_xy, (uint8_t*)d_out_inf, (uint8_t*)d_status);
            ZK_HIP_TRY(hipGetLastError());
        }
        return clear_cofactor ? clear_cofactor_impl<Cv>(c, n, d_out_xy, d_out_inf, d_status) : ZK_OK;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
size_t zk_ipa_sample_generators_waves(size_t n) { return (n + H2C_CHUNK - 1) / H2C_CHUNK; }

int zk_ipa_sample_generators_dev(zk_ctx* c, int curve_id, int digest_id, uint64_t first_index, size_t n, uint32_t max_tries, void* d_out_xy,
                                 void* d_out_inf, void* d_tries, void* d_status, void* d_wave_rounds) {
    if (!c || !zk_curve_ok(curve_id) || (digest_id != ZK_H2C_BLAKE2S && digest_id != ZK_H2C_BLAKE2B)) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    if (!d_out_xy || !d_out_inf || !d_status) return ZK_ERR_BAD_ARG;
    if (first_index + (uint64_t)n < first_index) return ZK_ERR_BAD_ARG;             // the indices are u64
    if (n > ((size_t)1 << 31) * H2C_CHUNK - H2C_CHUNK) return ZK_ERR_UNSUPPORTED;   // the grid of one launch
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return sample_impl<decltype(cv)>(c, digest_id, first_index, n, max_tries ? max_tries : 1024u, d_out_xy, d_out_inf, d_tries, d_status,
                                         d_wave_rounds);
    });
}

int zk_g1_from_random_bytes_batch_dev(zk_ctx* c, int curve_id, const void* d_bytes, size_t byte_len, size_t n, int clear_cofactor, void* d_out_xy,
                                      void* d_out_inf, void* d_status) {
    if (!c || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    if (!d_out_xy || !d_out_inf || !d_status || (byte_len && !d_bytes)) return ZK_ERR_BAD_ARG;
    if (byte_len > ((size_t)1 << 20) || n > ((size_t)1 << 31) * FRB_T - FRB_T) return ZK_ERR_UNSUPPORTED;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        return from_random_bytes_impl<decltype(cv)>(c, d_bytes, byte_len, n, clear_cofactor, d_out_xy, d_out_inf, d_status);
    });
}
