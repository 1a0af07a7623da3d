// Inner-product-argument polynomial commitment (ark-poly-commit 0.3 `ipa_pc::InnerProductArgPC`, the reference's second
// `HomomorphicCommitment`: plonk-core/src/commitment.rs:50-91): the device side of `open` and of the verifier's final-key check.
//
// The library keeps no IPA state: the vectors a, b and a workspace (the folded key in the MSM's internal base layout, the canonical copy
// of a the round MSMs read, the inner-product partial sums of the next round) live in buffers the caller owns, and every challenge is
// derived by the caller (the transcript rules are not part of the C ABI).  One opening over a key of d1 = d + 1 = 2^k points is
//   round(first) fold(first) round fold ... round fold          k rounds, m = d1/2, d1/4, ..., 1
// where round j computes L = MSM(key_l, a_r) + <a_r, b_l> h', R = MSM(key_r, a_l) + <a_l, b_r> h' and fold j applies the challenge:
//   key'_i = key_l[i] + xi key_r[i]   (ipa_fold_key: one variable-base scalar multiplication per point, xi shared by every lane)
//   a' = a_l + xi^-1 a_r, b' = b_l + xi b_r   (ipa_scalar_pass: also the canonical copy of a' and the next round's inner products)
// Round 0 reads the registered key itself (SRS window-table path); later rounds run the per-window MSM over the folded key.
// The verifier's side: the check vector of one opening (check_coeffs_impl), and the check vectors of a batch of openings combined
// under weights into the scalars of one key MSM (check_combine_impl).
#include "api_internal.h"
#include "g1_host.h"
#include "block_inverse.cuh"
#include "fr_io.cuh"
#include "point_io.cuh"

#include <shared_mutex>

namespace {

// The folded key keeps the layout of the MSM's internal bases (point_io.cuh: NL limbs padded to whole uint4, x then y; "no point"
// -- infinity -- is all-zero limbs); a and b are Fr elements as the saturated type of field.cuh (fr_io.cuh).
using namespace zkmsm;

// The challenge of a key fold in non-adjacent form: digit i is +1 where bit i of pos is set, -1 where bit i of neg is set; `top` is the
// index of the highest digit (always +1), -1 for xi = 0.  A kernel argument: every lane walks the same digits.
constexpr int NAF_WORDS = 9;     // 288 bits: a NAF has at most one digit more than the 255-bit scalar
struct Naf {
    uint32_t pos[NAF_WORDS];
    uint32_t neg[NAF_WORDS];
    int32_t top;
};
// word w of a kernel-argument array with a run-time (uniform) index, as a chain of selects: no copy of the array to scratch memory
ZK_D uint32_t pick(const uint32_t (&a)[NAF_WORDS], int w) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < NAF_WORDS; ++k) r = (k == w) ? a[k] : r;
    return r;
}

constexpr uint32_t FOLD_T = 128;   // lanes per block of the key fold = points per batched inversion

// dst[i] = src[i] + xi * src[i + m] for i < m, affine, internal layout.  dst may alias src (lane i alone reads src[i] and src[i + m]
// and writes dst[i]).  Per lane: the NAF of xi as doublings and mixed additions of +-src[i + m] on the XYZZ law of ecu.cuh, one mixed
// addition of src[i]; then the block normalises its 128 results with ONE field inversion of the ZZZ (block_inverse.cuh) and the
// law's own normalisation from a known 1/ZZZ (XYZZu::to_affine_given).
template <class Cv>
__global__ void __launch_bounds__(FOLD_T) ipa_fold_key(const void* src, void* dst, uint64_t m, Naf nf) {
    typedef typename Cv::FqU F;
    typedef XYZZu<F> P;
    __shared__ BlockInverseLds<F, FOLD_T> lds;
    const uint32_t t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * FOLD_T + t;
    const bool active = i < m;
    P acc = P::infinity();
    if (active) {
        const AffineU<F> q = ld_affine<F>(src, i + m);
        if (!q.is_null() && nf.top >= 0) {
            acc = P::from_affine(q);
            for (int b = nf.top - 1; b >= 0; --b) {
                acc = P::dbl(acc);
                const uint32_t sh = (uint32_t)b & 31u;
                const bool dp = (pick(nf.pos, b >> 5) >> sh) & 1u;
                const bool dn = (pick(nf.neg, b >> 5) >> sh) & 1u;
                if (dp || dn) {
                    AffineU<F> qq;
                    qq.x = q.x;
                    qq.y = dn ? F::neg(q.y) : q.y;
                    acc = P::madd(acc, qq);
                }
            }
        }
        const AffineU<F> kl = ld_affine<F>(src, i);
        if (!kl.is_null()) acc = P::madd(acc, kl);
    }
    const bool fin = active && !acc.is_inf();
    if (!fin) acc.zzz = F::one();                        // a lane with no finite result enters the product as 1
    const F zi3 = block_inverse(acc.zzz, lds);           // 1 / ZZZ_i
    if (!active) return;
    uint4* out = reinterpret_cast<uint4*>(dst) + i * (2 * Store<F>::U4);
    if (!fin) {
        st_fu<F>(out, F::zero());
        st_fu<F>(out + Store<F>::U4, F::zero());
        return;
    }
    AffineU<F> a;
    acc.to_affine_given(zi3, a);
    st_fu<F>(out, F::canonical_lt2p(a.x));
    st_fu<F>(out + Store<F>::U4, F::canonical_lt2p(a.y));
}

constexpr uint32_t SP_T = 256;     // lanes per block of the scalar pass

// The scalar side of a round, one pass.  The vectors after the pass have length mo; lane j < mo/2 owns elements j and j + mo/2 of them
// (the low and high halves of the NEXT round).  FOLD: a' = a_l + xi^-1 a_r, b' = b_l + xi b_r from the vectors of length 2 mo, in place;
// otherwise a, b are read as they are (the first round).  Writes a_can = canonical a' (the round MSMs' scalars) and, per block, the
// partial sums of <a'_r, b'_l> and <a'_l, b'_r> (Montgomery) to partials[block][2].
template <class Cv, bool FOLD>
__global__ void __launch_bounds__(SP_T) ipa_scalar_pass(void* a, void* b, uint64_t mo, typename Cv::Fr xi, typename Cv::Fr xi_inv, void* a_can,
                                                        void* partials) {
    typedef typename Cv::Fr Fr;
    __shared__ Fr s1[SP_T];
    __shared__ Fr s2[SP_T];
    const uint32_t t = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * SP_T + t;
    if (mo == 1) {                                       // the last fold: one element, no inner product follows
        if (j == 0) {
            Fr al = ld_fr<Fr>(a, 0);
            if (FOLD) {
                al = Fr::add(al, Fr::mul(xi_inv, ld_fr<Fr>(a, 1)));
                const Fr bl = Fr::add(ld_fr<Fr>(b, 0), Fr::mul(xi, ld_fr<Fr>(b, 1)));
                st_fr<Fr>(a, 0, al);
                st_fr<Fr>(b, 0, bl);
            }
            st_fr<Fr>(a_can, 0, Fr::from_mont(al));
        }
        return;
    }
    const uint64_t h = mo >> 1;
    Fr ip1 = Fr::zero(), ip2 = Fr::zero();
    if (j < h) {
        Fr al = ld_fr<Fr>(a, j), ah = ld_fr<Fr>(a, j + h), bl = ld_fr<Fr>(b, j), bh = ld_fr<Fr>(b, j + h);
        if (FOLD) {
            al = Fr::add(al, Fr::mul(xi_inv, ld_fr<Fr>(a, j + mo)));
            ah = Fr::add(ah, Fr::mul(xi_inv, ld_fr<Fr>(a, j + h + mo)));
            bl = Fr::add(bl, Fr::mul(xi, ld_fr<Fr>(b, j + mo)));
            bh = Fr::add(bh, Fr::mul(xi, ld_fr<Fr>(b, j + h + mo)));
            st_fr<Fr>(a, j, al);
            st_fr<Fr>(a, j + h, ah);
            st_fr<Fr>(b, j, bl);
            st_fr<Fr>(b, j + h, bh);
        }
        st_fr<Fr>(a_can, j, Fr::from_mont(al));
        st_fr<Fr>(a_can, j + h, Fr::from_mont(ah));
        ip1 = Fr::mul(ah, bl);
        ip2 = Fr::mul(al, bh);
    }
    s1[t] = ip1;
    s2[t] = ip2;
    for (uint32_t d = SP_T / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (t < d) {
            ip1 = Fr::add(ip1, s1[t + d]);
            ip2 = Fr::add(ip2, s2[t + d]);
            s1[t] = ip1;
            s2[t] = ip2;
        }
    }
    if (t == 0) {
        st_fr<Fr>(partials, 2 * (uint64_t)blockIdx.x, ip1);
        st_fr<Fr>(partials, 2 * (uint64_t)blockIdx.x + 1, ip2);
    }
}

constexpr uint32_t POW_K = 16;     // consecutive powers per lane

// out[i] = z^i, i < n (Montgomery): each lane raises z to its first index, then steps by one multiplication
template <class Cv>
__global__ void __launch_bounds__(256) ipa_powers(typename Cv::Fr z, uint64_t n, void* out) {
    typedef typename Cv::Fr Fr;
    const uint64_t start = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * POW_K;
    if (start >= n) return;
    Fr p = Fr::pow_u64(z, start);
    const uint64_t end = start + POW_K < n ? start + POW_K : n;
    for (uint64_t i = start; i < end; ++i) {
        st_fr<Fr>(out, i, p);
        p = Fr::mul(p, z);
    }
}

// s[k + half] = s[k] * xi for k < half (Montgomery): one bit of the check polynomial's coefficient vector
template <class Cv>
__global__ void __launch_bounds__(256) ipa_check_expand(void* s, uint64_t half, typename Cv::Fr xi) {
    typedef typename Cv::Fr Fr;
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (half == 0) {
        if (k == 0) st_fr<Fr>(s, 0, Fr::one());
        return;
    }
    if (k < half) st_fr<Fr>(s, k + half, Fr::mul(ld_fr<Fr>(s, k), xi));
}

// ---- the combined check vector of a batch of openings: t[i] = sum_j w_j s_j[i], s_j the check vector of opening j.
// The index splits into lo_bits = ceil(log_d / 2) low bits and log_d - lo_bits high bits: s_j[hi << lo_bits | lo] = LO_j[lo] HI_j[hi],
// so each opening costs two tables of about sqrt(d1) entries and ONE product per coefficient instead of log_d.
constexpr uint32_t CT_T = 256;     // lanes per block of both combine kernels
constexpr uint32_t FLAG_UNREDUCED = 1;
constexpr size_t COMBINE_MAX_OPEN = (size_t)1 << 30;    // two table blocks per opening in one grid

// Block 2j fills LO_j (from the last lo_bits challenges of opening j), block 2j + 1 fills W_HI_j = w_j HI_j (from the first
// log_d - lo_bits): ipa_check_expand's doubling, tab[k + 2^b] = tab[k] xi, one step per bit with a barrier between steps (a block
// strides over a table wider than itself).  Montgomery.  Each block tests what it reads: a challenge or weight that is not below r
// sets the flag (the tables of that opening are then meaningless, and the call fails).
template <class Cv>
__global__ void __launch_bounds__(CT_T) ipa_combine_tables(const void* xis, const void* weights, uint32_t log_d, uint32_t lo_bits, void* lo_tab,
                                                           void* hi_tab, uint32_t* flag) {
    typedef typename Cv::Fr Fr;
    const uint32_t t = threadIdx.x;
    const uint64_t j = blockIdx.x >> 1;
    const bool high = blockIdx.x & 1;
    const uint32_t bits = high ? log_d - lo_bits : lo_bits;
    const uint32_t top = high ? log_d - lo_bits : log_d;         // bit b of the table index selects challenge top - 1 - b
    void* tab = high ? hi_tab : lo_tab;
    const uint64_t base = j << bits;
    if (t == 0) {
        Fr first = Fr::one();
        if (high) {
            first = ld_fr<Fr>(weights, j);
            if (Fr::reduce_once(first) != first) atomicOr(flag, FLAG_UNREDUCED);
        }
        st_fr<Fr>(tab, base, first);
    }
    for (uint32_t b = 0; b < bits; ++b) {
        const Fr xi = ld_fr<Fr>(xis, j * log_d + (top - 1 - b));
        if (t == 0 && Fr::reduce_once(xi) != xi) atomicOr(flag, FLAG_UNREDUCED);
        __syncthreads();
        const uint64_t half = (uint64_t)1 << b;
        for (uint64_t k = t; k < half; k += CT_T) st_fr<Fr>(tab, base + half + k, Fr::mul(ld_fr<Fr>(tab, base + k), xi));
    }
}

// out[i] = sum_j LO_j[lo] W_HI_j[hi], canonical: one lane per coefficient, one product and one addition per opening, one store.
// Lanes of a wave share hi wherever a low table spans a wave, so W_HI_j[hi] is one broadcast load and LO_j[lo] a contiguous one.
template <class Cv>
__global__ void __launch_bounds__(CT_T) ipa_combine_sum(const void* lo_tab, const void* hi_tab, uint32_t log_d, uint32_t lo_bits, uint64_t n_open,
                                                        void* out) {
    typedef typename Cv::Fr Fr;
    const uint64_t i = (uint64_t)blockIdx.x * CT_T + threadIdx.x;
    if (i >> log_d) return;
    const uint32_t hi_bits = log_d - lo_bits;
    const uint64_t lo = i & (((uint64_t)1 << lo_bits) - 1), hi = i >> lo_bits;
    Fr acc = Fr::zero();
    for (uint64_t j = 0; j < n_open; ++j)
        acc = Fr::add(acc, Fr::mul(ld_fr<Fr>(lo_tab, (j << lo_bits) + lo), ld_fr<Fr>(hi_tab, (j << hi_bits) + hi)));
    st_fr<Fr>(out, i, Fr::from_mont(acc));
}

// internal layout -> ABI affine (x || y Montgomery, infinity = (0, 1) with flag 1, as GroupAffine::zero())
template <class Cv>
__global__ void __launch_bounds__(256) ipa_to_abi(const void* src, uint64_t n, uint32_t* out_xy, uint8_t* out_inf) {
    typedef typename Cv::FqU F;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const AffineU<F> p = ld_affine<F>(src, i);
    uint32_t* w = out_xy + i * 2 * F::SAT;
    const bool inf = p.is_null();
    if (inf) {
        for (int k = 0; k < F::SAT; ++k) {
            w[k] = 0;
            w[F::SAT + k] = Cv::FqP::R(k);
        }
    } else {
        p.x.to_sat(w);
        p.y.to_sat(w + F::SAT);
    }
    if (out_inf) out_inf[i] = inf ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline bool pow2(size_t x) { return x && !(x & (x - 1)); }

// workspace of one opening over d1 points: [folded key: d1/2 points][a_can: d1 scalars][partials: 2 Fr per scalar-pass block]
struct Layout {
    size_t key = 0, a_can = 0, partials = 0, total = 0;
};
inline Layout layout(int curve, size_t d1) {
    Layout l;
    const size_t pb = msm_ops(curve)->point_bytes();
    const size_t half = d1 / 2 ? d1 / 2 : 1;
    const size_t n_part = blocks_of(d1 / 2 ? d1 / 2 : 1, SP_T) + 1;
    l.key = 0;
    l.a_can = up256(half * pb);
    l.partials = l.a_can + up256(d1 * 32);
    l.total = l.partials + up256(n_part * 64);
    return l;
}

// the NAF of a canonical scalar (8 little-endian 32-bit words)
inline Naf make_naf(const uint32_t* k8) {
    Naf nf;
    memset(&nf, 0, sizeof nf);
    nf.top = -1;
    uint64_t k[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < 8; ++w) k[w / 2] |= (uint64_t)k8[w] << (32 * (w & 1));
    for (int i = 0; i < 32 * NAF_WORDS; ++i) {
        if (!(k[0] | k[1] | k[2] | k[3] | k[4])) break;
        if (k[0] & 1) {
            if ((k[0] & 3) == 1) {                        // digit +1: k -= 1
                k[0] -= 1;
                nf.pos[i >> 5] |= 1u << (i & 31);
            } else {                                      // digit -1: k += 1
                for (int w = 0; w < 5; ++w)
                    if (++k[w] != 0) break;
                nf.neg[i >> 5] |= 1u << (i & 31);
            }
            nf.top = i;
        }
        for (int w = 0; w < 5; ++w) k[w] = (k[w] >> 1) | (w + 1 < 5 ? k[w + 1] << 63 : 0);
    }
    return nf;
}

template <class Cv>
int launch_fold_key(zk_ctx* c, const void* src, void* dst, size_t m, const uint64_t* xi_mont) {
    typedef typename Cv::Fr Fr;
    Fr xi;
    if (!fr_reduced<Fr>(xi_mont, xi)) return ZK_ERR_BAD_ARG;
    const Fr k = Fr::from_mont(xi);
    const Naf nf = make_naf(k.v);
    ProfScope ps(c, "ipa_fold_key");
    hipLaunchKernelGGL(ipa_fold_key<Cv>, dim3(blocks_of(m, FOLD_T)), dim3(FOLD_T), 0, c->stream, src, dst, (uint64_t)m, nf);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class Cv, bool FOLD>
int launch_scalar_pass(zk_ctx* c, void* a, void* b, size_t mo, const typename Cv::Fr& xi, const typename Cv::Fr& xi_inv, void* a_can,
                       void* partials) {
    const uint64_t lanes = mo > 1 ? mo / 2 : 1;
    ProfScope ps(c, "ipa_scalar_pass");
    hipLaunchKernelGGL((ipa_scalar_pass<Cv, FOLD>), dim3(blocks_of(lanes, SP_T)), dim3(SP_T), 0, c->stream, a, b, (uint64_t)mo, xi,
                       xi_inv, a_can, partials);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

// host: affine out = P + k * Q (P Jacobian as the MSM returns it, Q affine Montgomery, k Montgomery Fr)
template <class Cv>
void add_scaled(const uint64_t* xyz, const uint64_t* q_xy, const typename Cv::Fr& k_mont, uint64_t* out_xy, uint8_t* out_inf) {
    typedef G1Host<typename Cv::Fq> H;
    typedef typename Cv::Fr Fr;
    typename H::P p = H::ld_jacobian(xyz);
    const typename H::A q = H::ld_affine(q_xy);
    if (!H::affine_is_inf(q)) p = H::P::add(p, H::scalar_mul(q, Fr::from_mont(k_mont).v, Fr::N));
    H::st_normalised(out_xy, out_inf, p);
}

// NULL handles, a key of another device, a key length that is not a power of two: ZK_ERR_BAD_ARG
inline int check_key(zk_ctx* c, zk_srs* s) {
    if (!c || !s) return ZK_ERR_BAD_ARG;
    if (s->device != c->device || !zk_curve_ok(s->curve) || !pow2(s->n)) return ZK_ERR_BAD_ARG;
    return ZK_OK;
}
// m fits the key: round / fold j works on vectors of 2m <= d1 (first round: 2m = d1 exactly at the top, or any smaller power of two)
inline bool m_fits(const zk_srs* s, int first_round, size_t m) {
    if (!pow2(m)) return false;
    return first_round ? 2 * m <= s->n : 2 * m <= s->n / 2;
}

template <class Cv>
int round_impl(zk_ctx* c, zk_srs* s, int first_round, size_t m, void* d_a, void* d_b, void* d_work, const uint64_t* h_prime_xy,
               uint64_t* out_lr_xy, uint8_t* out_lr_inf) {
    typedef typename Cv::Fr Fr;
    constexpr int L64 = G1Host<typename Cv::Fq>::L;
    const Layout ly = layout(s->curve, s->n);
    char* w = (char*)d_work;
    void* a_can = w + ly.a_can;
    void* partials = w + ly.partials;
    int rc;
    if (first_round && (rc = launch_scalar_pass<Cv, false>(c, d_a, d_b, 2 * m, Fr::zero(), Fr::zero(), a_can, partials))) return rc;
    // the inner products: the scalar pass's per-block partial sums (the fold before this round, or the pass above), added up here
    const size_t nb = blocks_of(m, SP_T);
    std::vector<uint64_t> part(nb * 8);
    if ((rc = zk_d2h(c, part.data(), partials, nb * 64, c->stream))) return rc;
    Fr ip1 = Fr::zero(), ip2 = Fr::zero();
    for (size_t k = 0; k < nb; ++k) {
        Fr x, y;
        memcpy(x.v, &part[8 * k], 32);
        memcpy(y.v, &part[8 * k + 4], 32);
        ip1 = Fr::add(ip1, x);
        ip2 = Fr::add(ip2, y);
    }
    uint64_t xyz_l[ZK_MAX_JACOBIAN64], xyz_r[ZK_MAX_JACOBIAN64];
    const char* ac = (const char*)a_can;
    if (first_round) {
        if (s->pre_wstep > 1) return ZK_ERR_UNSUPPORTED;    // a window-sharded key returns partials: not an opening's MSM
        if ((rc = zk_msm_g1_srs_partial_dev(c, s, 0, ac + 32 * m, m, xyz_l))) return rc;
        if ((rc = zk_msm_g1_srs_partial_dev(c, s, m, ac, m, xyz_r))) return rc;
    } else {
        const size_t pb = msm_ops(s->curve)->point_bytes();
        if ((rc = msm_ops(s->curve)->run(c, w + ly.key, ac + 32 * m, m, xyz_l))) return rc;
        if ((rc = msm_ops(s->curve)->run(c, w + ly.key + m * pb, ac, m, xyz_r))) return rc;
    }
    add_scaled<Cv>(xyz_l, h_prime_xy, ip1, out_lr_xy, out_lr_inf);
    add_scaled<Cv>(xyz_r, h_prime_xy, ip2, out_lr_xy + 2 * L64, out_lr_inf ? out_lr_inf + 1 : nullptr);
    return ZK_OK;
}

template <class Cv>
int fold_impl(zk_ctx* c, zk_srs* s, int first_round, size_t m, const uint64_t* xi_mont, void* d_a, void* d_b, void* d_work) {
    typedef typename Cv::Fr Fr;
    Fr xi;
    if (!fr_reduced<Fr>(xi_mont, xi) || xi.is_zero()) return ZK_ERR_BAD_ARG;
    const Fr xi_inv = Fr::inverse(xi);
    const Layout ly = layout(s->curve, s->n);
    char* w = (char*)d_work;
    int rc;
    if (first_round) {
        std::shared_lock<std::shared_mutex> rl(s->mu);       // the registered key is read by the kernel below (queued under the lock)
        if ((rc = launch_fold_key<Cv>(c, s->d_xy, w + ly.key, m, xi_mont))) return rc;
    } else if ((rc = launch_fold_key<Cv>(c, w + ly.key, w + ly.key, m, xi_mont))) {
        return rc;
    }
    return launch_scalar_pass<Cv, true>(c, d_a, d_b, m, xi, xi_inv, w + ly.a_can, w + ly.partials);
}

template <class Cv>
int powers_impl(zk_ctx* c, const uint64_t* point_mont, size_t n, void* d_out) {
    typedef typename Cv::Fr Fr;
    Fr z;
    if (!fr_reduced<Fr>(point_mont, z)) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    const uint64_t lanes = blocks_of(n, POW_K);
    ProfScope ps(c, "ipa_powers");
    hipLaunchKernelGGL(ipa_powers<Cv>, dim3(blocks_of(lanes, 256)), dim3(256), 0, c->stream, z, (uint64_t)n, d_out);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class Cv>
int check_coeffs_impl(zk_ctx* c, int curve, uint32_t log_d, const uint64_t* xis_mont, void* d_out) {
    typedef typename Cv::Fr Fr;
    std::vector<Fr> xi(log_d);
    for (uint32_t j = 0; j < log_d; ++j)
        if (!fr_reduced<Fr>(xis_mont + 4 * j, xi[j])) return ZK_ERR_BAD_ARG;
    ProfScope ps(c, "ipa_check_coeffs");
    hipLaunchKernelGGL(ipa_check_expand<Cv>, dim3(1), dim3(1), 0, c->stream, d_out, (uint64_t)0, Fr::one());
    // bit (log_d - 1 - j) of k selects xi_j: xi_{log_d-1} doubles the vector first (bit 0), xi_0 last (the top bit)
    for (uint32_t b = 0; b < log_d; ++b) {
        const uint64_t half = (uint64_t)1 << b;
        hipLaunchKernelGGL(ipa_check_expand<Cv>, dim3(blocks_of(half, 256)), dim3(256), 0, c->stream, d_out, half, xi[log_d - 1 - b]);
    }
    ZK_HIP_TRY(hipGetLastError());
    return fr_convert_dev(c, curve, 0, d_out, (size_t)1 << log_d, d_out);     // canonical: the MSM's scalars
}

// the combine's workspace: [LO: n_open tables of 2^lo_bits Fr][W_HI: n_open tables of 2^(log_d - lo_bits) Fr]
inline uint32_t combine_lo_bits(uint32_t log_d) { return (log_d + 1) / 2; }
inline size_t combine_lo_bytes(uint32_t log_d, size_t n_open) { return up256(n_open * (((size_t)32) << combine_lo_bits(log_d))); }
inline size_t combine_hi_bytes(uint32_t log_d, size_t n_open) {
    return up256(n_open * (((size_t)32) << (log_d - combine_lo_bits(log_d))));
}

template <class Cv>
int check_combine_impl(zk_ctx* c, uint32_t log_d, size_t n_open, const void* d_xis, const void* d_weights, void* d_work, void* d_out) {
    const uint32_t lo_bits = combine_lo_bits(log_d);
    void* lo_tab = d_work;
    void* hi_tab = (char*)d_work + combine_lo_bytes(log_d, n_open);
    const unsigned sum_blocks = blocks_of((uint64_t)1 << log_d, CT_T);
    ProfScope ps(c, "ipa_check_combine");
    if (n_open == 0) {                                           // the empty sum: no tables, nothing to test
        hipLaunchKernelGGL(ipa_combine_sum<Cv>, dim3(sum_blocks), dim3(CT_T), 0, c->stream, lo_tab, hi_tab, log_d, lo_bits, (uint64_t)0, d_out);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    }
    return run_flagged(c, 0, [&](uint32_t* d_flag, void*) -> int {
        hipLaunchKernelGGL(ipa_combine_tables<Cv>, dim3((unsigned)(2 * n_open)), dim3(CT_T), 0, c->stream, d_xis, d_weights, log_d, lo_bits,
                           lo_tab, hi_tab, d_flag);
        ZK_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ipa_combine_sum<Cv>, dim3(sum_blocks), dim3(CT_T), 0, c->stream, lo_tab, hi_tab, log_d, lo_bits, (uint64_t)n_open,
                           d_out);
        ZK_HIP_TRY(hipGetLastError());
        return ZK_OK;
    });
}

template <class Cv>
int to_abi(zk_ctx* c, const void* src, size_t n, void* d_out_xy, uint8_t* d_out_inf) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(ipa_to_abi<Cv>, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, src, (uint64_t)n, (uint32_t*)d_out_xy, d_out_inf);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

template <class Cv>
void internal_to_abi_host(const void* pt, uint64_t* out_xy, uint8_t* out_inf) {
    typedef typename Cv::FqU F;
    typedef G1Host<typename Cv::Fq> H;
    const uint32_t* w = (const uint32_t*)pt;
    AffineU<F> p;
    for (int k = 0; k < F::NL; ++k) {
        p.x.v[k] = w[k];
        p.y.v[k] = w[4 * Store<F>::U4 + k];
    }
    if (p.is_null()) return H::st_affine_inf(out_xy, out_inf);
    p.x.to_sat((uint32_t*)out_xy);
    p.y.to_sat((uint32_t*)(out_xy + H::L));
    if (out_inf) *out_inf = 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
size_t zk_ipa_workspace_bytes(int curve_id, size_t d1) {
    if (!zk_curve_ok(curve_id) || !pow2(d1)) return 0;
    return layout(curve_id, d1).total;
}

int zk_ipa_powers_dev(zk_ctx* c, int curve_id, const uint64_t* point_mont, size_t n, void* d_out) {
    if (!c || !zk_curve_ok(curve_id) || !point_mont || (n && !d_out)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return powers_impl<decltype(cv)>(c, point_mont, n, d_out); });
}

int zk_ipa_round_dev(zk_ctx* c, zk_srs* key, int first_round, size_t m, const void* d_a, const void* d_b, void* d_work,
                     const uint64_t* h_prime_xy, uint64_t* out_lr_xy, uint8_t* out_lr_inf) {
    int rc = check_key(c, key);
    if (rc) return rc;
    if (!m_fits(key, first_round, m) || !d_a || !d_b || !d_work || !h_prime_xy || !out_lr_xy) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (round_open(c)) return ZK_ERR_PENDING;
    void* a = const_cast<void*>(d_a);    // the first round's scalar pass reads a, b (FOLD = false writes neither)
    void* b = const_cast<void*>(d_b);
    return zk_on_curve(key->curve, ZK_ERR_BAD_ARG,
                       [&](auto cv) { return round_impl<decltype(cv)>(c, key, first_round, m, a, b, d_work, h_prime_xy, out_lr_xy, out_lr_inf); });
}

int zk_ipa_fold_dev(zk_ctx* c, zk_srs* key, int first_round, size_t m, const uint64_t* xi_mont, void* d_a, void* d_b, void* d_work) {
    int rc = check_key(c, key);
    if (rc) return rc;
    if (!m_fits(key, first_round, m) || !xi_mont || !d_a || !d_b || !d_work) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return zk_on_curve(key->curve, ZK_ERR_BAD_ARG, [&](auto cv) { return fold_impl<decltype(cv)>(c, key, first_round, m, xi_mont, d_a, d_b, d_work); });
}

int zk_ipa_final_key_dev(zk_ctx* c, int curve_id, const void* d_work, uint64_t* out_xy, uint8_t* out_inf) {
    if (!c || !zk_curve_ok(curve_id) || !d_work || !out_xy) return ZK_ERR_BAD_ARG;
    Guard g(c);
    uint64_t pt[32];
    const size_t pb = msm_ops(curve_id)->point_bytes();
    if (pb > sizeof pt) return ZK_ERR_UNSUPPORTED;
    int rc = zk_d2h(c, pt, d_work, pb, c->stream);
    if (rc) return rc;
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        internal_to_abi_host<decltype(cv)>(pt, out_xy, out_inf);
        return ZK_OK;
    });
}

int zk_ipa_fold_key_dev(zk_ctx* c, int curve_id, size_t m, const void* d_key_xy, const uint8_t* d_key_inf, const uint64_t* xi_mont,
                        void* d_out_xy, uint8_t* d_out_inf) {
    if (!c || !zk_curve_ok(curve_id) || !xi_mont || (m && (!d_key_xy || !d_out_xy))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    if (m == 0) return ZK_OK;
    const size_t pb = msm_ops(curve_id)->point_bytes();
    void* tmp = nullptr;
    if (hipMalloc(&tmp, 3 * m * pb) != hipSuccess) return zk_alloc_refused();
    void* folded = (char*)tmp + 2 * m * pb;
    int rc = msm_ops(curve_id)->convert_bases(c, d_key_xy, d_key_inf, 2 * m, tmp);
    if (!rc) rc = zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return launch_fold_key<decltype(cv)>(c, tmp, folded, m, xi_mont); });
    if (!rc) rc = zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return to_abi<decltype(cv)>(c, folded, m, d_out_xy, d_out_inf); });
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = ZK_ERR_HIP;
    (void)hipFree(tmp);
    return rc;
}

int zk_ipa_check_coeffs_dev(zk_ctx* c, int curve_id, uint32_t log_d, const uint64_t* xis_mont, void* d_out) {
    if (!c || !zk_curve_ok(curve_id) || log_d > 32 || !d_out || (log_d && !xis_mont)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return check_coeffs_impl<decltype(cv)>(c, curve_id, log_d, xis_mont, d_out); });
}

size_t zk_ipa_check_combine_workspace_bytes(int curve_id, uint32_t log_d, size_t n_open) {
    if (!zk_curve_ok(curve_id) || log_d > 32 || n_open > COMBINE_MAX_OPEN) return 0;
    return combine_lo_bytes(log_d, n_open) + combine_hi_bytes(log_d, n_open);
}

int zk_ipa_check_combine_dev(zk_ctx* c, int curve_id, uint32_t log_d, size_t n_open, const void* d_xis_mont, const void* d_weights_mont,
                             void* d_work, void* d_out) {
    if (!c || !zk_curve_ok(curve_id) || log_d > 32 || n_open > COMBINE_MAX_OPEN || !d_out) return ZK_ERR_BAD_ARG;
    if (n_open && (!d_weights_mont || !d_work || (log_d && !d_xis_mont))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG,
                       [&](auto cv) { return check_combine_impl<decltype(cv)>(c, log_d, n_open, d_xis_mont, d_weights_mont, d_work, d_out); });
}
