// The KZG pairing check e(L, [tau]H) e(-R, H) = 1: prepared verifier keys, one check on the host, n checks on the device.
//
// Replaces (behind the C ABI) ark_ec::PairingEngine::product_of_pairings and kzg10::KZG10::check (ark-poly-commit 0.3
// kzg10/mod.rs: e(C - vG - ... , H) = e(W, [beta]H - zH) in its folded form, the two G1 inputs being what the batch verifier of
// verify.hip / verifier.py produces).
//
// Both G2 points are fixed per verifier key, so zk_pairing_key_new validates them and walks their Miller loops ONCE, with affine G2
// steps in host Fq2, into two line tables (pairing.cuh).  A check is then line evaluations at G1 points, sparse Fq12 products and
// squarings, and the final exponentiation: no G2 arithmetic where a check runs.
//   * one check (a fold of a whole batch, each step of a bisection) is latency-bound: it runs on the host, with no ctx and no GPU;
//   * n independent checks (per-proof verdicts) run as one launch, one check per lane, the running Fq12 values in scratch memory.
#include "api_internal.h"
#include "pairing.cuh"

#include <mutex>
#include <vector>

namespace {

typedef Pairing<PairingBls12_381Params, FqBls> PairBls;
typedef Pairing<PairingBn254Params, FqBn> PairBn;
template <class Cv>
struct PairOf;
template <>
struct PairOf<CurveBls> {
    typedef PairBls T;
    typedef PairingBls12_381Params PP;
};
template <>
struct PairOf<CurveBn> {
    typedef PairBn T;
    typedef PairingBn254Params PP;
};

constexpr unsigned PAIR_T = 64;           // lanes per workgroup: one wavefront

}  // namespace

// the prepared key: the step kinds (shared by the two tables) and the line tables of H (which = 0) and [tau]H (which = 1)
struct zk_pairing_key {
    int curve = 0;
    std::vector<uint8_t> steps;
    std::vector<uint32_t> lines[2];
    struct Dev {
        int device;
        void* base;
        const uint8_t* steps;
        const uint32_t* lines[2];
    };
    std::mutex mu;
    std::vector<Dev> dev;                 // one copy per device, made by the first device call there, freed with the key
};

namespace {

// ---- host G2: affine points of the twist over Fq2, for validation and the line tables (once per key)
template <class PR>
struct G2 {
    typename PR::Fq2 x, y;
    bool inf;
};

// t + s and (optionally) the line table entry of that step; false where the slope does not exist (t = -s, or a point of order 2)
template <class PR>
bool g2_step(const G2<PR>& t, const G2<PR>& s, G2<PR>& out, uint32_t* entry) {
    typedef typename PR::Fq2 Fq2;
    Fq2 num, den;
    if (PR::eq2(t.x, s.x)) {
        if (!PR::eq2(t.y, s.y)) return false;
        const Fq2 xx = PR::sqr2(t.x);
        num = PR::add2(PR::dbl2(xx), xx);
        den = PR::dbl2(t.y);
    } else {
        num = PR::sub2(s.y, t.y);
        den = PR::sub2(s.x, t.x);
    }
    if (PR::is_zero2(den)) return false;
    const Fq2 m = PR::mul2(num, PR::inv2(den));
    G2<PR> r;
    r.inf = false;
    r.x = PR::sub2(PR::sub2(PR::sqr2(m), t.x), s.x);
    r.y = PR::sub2(PR::mul2(m, PR::sub2(t.x, r.x)), t.y);
    if (entry) {
        const Fq2 k = PR::sub2(PR::mul2(m, t.x), t.y), nm = PR::neg2(m);
        PR::store_fq(entry, k.c0);
        PR::store_fq(entry + PR::N, k.c1);
        PR::store_fq(entry + 2 * PR::N, nm.c0);
        PR::store_fq(entry + 3 * PR::N, nm.c1);
    }
    out = r;
    return true;
}
// the group law with its special cases, for the order test
template <class PR>
G2<PR> g2_add(const G2<PR>& a, const G2<PR>& b) {
    if (a.inf) return b;
    if (b.inf) return a;
    G2<PR> r;
    if (!g2_step<PR>(a, b, r, nullptr)) r.inf = true;               // a = -b (a point of order 2 doubles to infinity too)
    return r;
}

// a coordinate is reduced: its words, most significant first, are below the modulus
template <class Cv>
bool words_below_modulus(const uint32_t* w) {
    typedef typename Cv::FqP P;
    for (int i = P::N - 1; i >= 0; --i) {
        if (w[i] < P::MOD(i)) return true;
        if (w[i] > P::MOD(i)) return false;
    }
    return false;                                                    // equal to the modulus
}

// a validated G2 point from 4 L limbs (x.c0 x.c1 y.c0 y.c1, Montgomery), or false
template <class Cv>
bool g2_read(const uint64_t* limbs, G2<typename PairOf<Cv>::T>& q) {
    typedef typename PairOf<Cv>::T PR;
    typedef typename PairOf<Cv>::PP PP;
    typedef typename PR::Fq2 Fq2;
    constexpr int N = PR::N;
    const uint32_t* w = (const uint32_t*)limbs;
    for (int k = 0; k < 4; ++k)
        if (!words_below_modulus<Cv>(w + k * N)) return false;
    q.x = PR::load2(w);
    q.y = PR::load2(w + 2 * N);
    q.inf = false;
    uint32_t bw[2 * N];
    for (int i = 0; i < 2 * N; ++i) bw[i] = PP::TWIST_B(i);
    const Fq2 rhs = PR::add2(PR::mul2(PR::sqr2(q.x), q.x), PR::load2(bw));
    if (!PR::eq2(PR::sqr2(q.y), rhs)) return false;                  // off the twist (the encodings of infinity included)
    // [r] q = infinity
    G2<PR> acc;
    acc.inf = true;
    acc.x = acc.y = PR::zero2();
    for (int i = Cv::FrP::N - 1; i >= 0; --i)
        for (int b = 31; b >= 0; --b) {
            acc = g2_add<PR>(acc, acc);
            if ((Cv::FrP::MOD(i) >> b) & 1u) acc = g2_add<PR>(acc, q);
        }
    return acc.inf;
}

// the Miller loop of q as a line table; `steps` is filled by the first table of a key and compared by the second
template <class Cv>
bool g2_prepare(const G2<typename PairOf<Cv>::T>& q, std::vector<uint8_t>& steps, std::vector<uint32_t>& lines) {
    typedef typename PairOf<Cv>::T PR;
    typedef typename PairOf<Cv>::PP PP;
    constexpr int N = PR::N;
    std::vector<uint8_t> kinds;
    lines.clear();
    auto push = [&](const G2<PR>& t, const G2<PR>& s, G2<PR>& out) {
        lines.resize(lines.size() + PR::LINE_WORDS);
        return g2_step<PR>(t, s, out, lines.data() + lines.size() - PR::LINE_WORDS);
    };
    int top = 64;
    while (top >= 0 && !(top == 64 ? PP::LOOP_HI : (uint32_t)((PP::LOOP_LO >> top) & 1u))) --top;
    G2<PR> t = q;
    for (int b = top - 1; b >= 0; --b) {
        uint8_t kind = 1;
        if (!push(t, t, t)) return false;
        if ((PP::LOOP_LO >> b) & 1u) {
            kind |= 2;
            if (!push(t, q, t)) return false;
        }
        kinds.push_back(kind);
    }
    if (PP::BN_TAIL) {
        // pi(x', y') = (conj(x') xi^((q - 1) / 3), conj(y') xi^((q - 1) / 2)) on the twist, pi^2 likewise with the q^2 constants
        uint32_t g[2 * N];
        G2<PR> q1, q2;
        q1.inf = q2.inf = false;
        for (int i = 0; i < 2 * N; ++i) g[i] = PP::FROB1(2, i);
        q1.x = PR::mul2(PR::conj2(q.x), PR::load2(g));
        for (int i = 0; i < 2 * N; ++i) g[i] = PP::FROB1(3, i);
        q1.y = PR::mul2(PR::conj2(q.y), PR::load2(g));
        for (int i = 0; i < N; ++i) g[i] = PP::FROB2(2, i);
        q2.x = PR::mul2_fq(q.x, PR::load_fq(g));
        for (int i = 0; i < N; ++i) g[i] = PP::FROB2(3, i);
        q2.y = PR::neg2(PR::mul2_fq(q.y, PR::load_fq(g)));
        if (!push(t, q1, t)) return false;
        kinds.push_back(2);
        if (!push(t, q2, t)) return false;
        kinds.push_back(2);
    }
    if (steps.empty()) steps = kinds;
    return steps == kinds;
}

template <class Cv>
int key_new(const uint64_t* h, const uint64_t* tau_h, zk_pairing_key** out) {
    typedef typename PairOf<Cv>::T PR;
    G2<PR> q[2];
    if (!g2_read<Cv>(h, q[0]) || !g2_read<Cv>(tau_h, q[1])) return ZK_ERR_BAD_ARG;
    std::unique_ptr<zk_pairing_key> key(new zk_pairing_key);
    key->curve = Cv::ID;
    for (int k = 0; k < 2; ++k)
        if (!g2_prepare<Cv>(q[k], key->steps, key->lines[k])) return ZK_ERR_BAD_ARG;
    *out = key.release();
    return ZK_OK;
}

// ---- one G1 point of the caller: coordinates (2 L limbs, Montgomery) and whether it is infinity
template <class PR>
struct G1In {
    decltype(PR::load_fq(nullptr)) x, y;
    bool inf;
};
template <class PR>
ZK_HD G1In<PR> g1_read(const uint32_t* xy, bool flag) {
    G1In<PR> p;
    p.x = PR::load_fq(xy);
    p.y = PR::load_fq(xy + PR::N);
    p.inf = PR::g1_is_inf(p.x, p.y, flag);
    return p;
}

// the host entry points' G1 contract: both coordinates of a point that is not flagged as infinity are below the modulus.  An unreduced
// y would change the verdict (Fp::neg of it is not the negation), and (q, 1) or (q, q) would read as the encodings of infinity.
template <class Cv>
bool g1_reduced(const uint64_t* xy, bool flag) {
    const uint32_t* w = (const uint32_t*)xy;
    return flag || (words_below_modulus<Cv>(w) && words_below_modulus<Cv>(w + PairOf<Cv>::T::N));
}

// [ e(L, tau_h) e(-R, h) == 1 ]
template <class PR>
ZK_HD bool check_one(const uint8_t* steps, int n_steps, const uint32_t* lines_tau, const uint32_t* lines_h, const uint32_t* l_xy, bool l_inf,
                     const uint32_t* r_xy, bool r_inf) {
    const G1In<PR> l = g1_read<PR>(l_xy, l_inf), r = g1_read<PR>(r_xy, r_inf);
    typename PR::Fq12 f;
    PR::miller2(f, steps, n_steps, lines_tau, lines_h, l.x, l.y, l.inf, r.x, decltype(r.y)::neg(r.y), r.inf);
    PR::final_exp(f, f);
    return PR::is_one12(f);
}
// e(P, Q)^GT_POWER for the table of Q, 12 Fq values in tower order
template <class PR>
ZK_HD void gt_one(const uint8_t* steps, int n_steps, const uint32_t* lines, const uint32_t* p_xy, bool p_inf, uint32_t* out) {
    const G1In<PR> p = g1_read<PR>(p_xy, p_inf);
    typename PR::Fq12 f;
    PR::miller2(f, steps, n_steps, lines, lines, p.x, p.y, p.inf, p.x, p.y, true);       // no second pair
    PR::final_exp(f, f);
    PR::store12(out, f);
}

template <class Cv>
__global__ void __launch_bounds__(PAIR_T) pairing_check_batch(const uint8_t* steps, int n_steps, const uint32_t* lines_tau, const uint32_t* lines_h,
                                                              const uint32_t* l_xy, const uint8_t* l_inf, const uint32_t* r_xy,
                                                              const uint8_t* r_inf, uint64_t n, uint8_t* ok) {
    typedef typename PairOf<Cv>::T PR;
    const uint64_t k = (uint64_t)blockIdx.x * PAIR_T + threadIdx.x;
    if (k >= n) return;
    ok[k] = check_one<PR>(steps, n_steps, lines_tau, lines_h, l_xy + k * 2 * PR::N, l_inf && l_inf[k], r_xy + k * 2 * PR::N,
                          r_inf && r_inf[k])
                ? 1
                : 0;
}

template <class Cv>
__global__ void __launch_bounds__(PAIR_T) pairing_gt_batch(const uint8_t* steps, int n_steps, const uint32_t* lines, const uint32_t* p_xy,
                                                           const uint8_t* p_inf, uint64_t n, uint32_t* out) {
    typedef typename PairOf<Cv>::T PR;
    const uint64_t k = (uint64_t)blockIdx.x * PAIR_T + threadIdx.x;
    if (k >= n) return;
    gt_one<PR>(steps, n_steps, lines, p_xy + k * 2 * PR::N, p_inf && p_inf[k], out + k * 12 * PR::N);
}

// the key's tables on the ctx's device (uploaded by the first call there).  ctx lock held, the ctx's device current.
int key_on_device(zk_ctx* c, zk_pairing_key* key, zk_pairing_key::Dev& out) {
    std::lock_guard<std::mutex> lk(key->mu);
    for (const auto& d : key->dev)
        if (d.device == c->device) {
            out = d;
            return ZK_OK;
        }
    const size_t steps_bytes = up256(key->steps.size());
    const size_t line_bytes[2] = {up256(key->lines[0].size() * 4), up256(key->lines[1].size() * 4)};
    zk_pairing_key::Dev d;
    d.device = c->device;
    d.base = nullptr;
    if (hipMalloc(&d.base, steps_bytes + line_bytes[0] + line_bytes[1]) != hipSuccess) return zk_alloc_refused();
    char* p = (char*)d.base;
    d.steps = (const uint8_t*)p;
    d.lines[0] = (const uint32_t*)(p + steps_bytes);
    d.lines[1] = (const uint32_t*)(p + steps_bytes + line_bytes[0]);
    hipError_t e = hipMemcpy(p, key->steps.data(), key->steps.size(), hipMemcpyHostToDevice);
    for (int k = 0; k < 2 && e == hipSuccess; ++k)
        e = hipMemcpy((void*)d.lines[k], key->lines[k].data(), key->lines[k].size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d.base);
        ZK_HIP_TRY(e);
    }
    key->dev.push_back(d);
    out = d;
    return ZK_OK;
}

}  // namespace

int zk_pairing_key_new(int curve_id, const uint64_t* h, const uint64_t* tau_h, void** out) {
    if (!h || !tau_h || !out) return ZK_ERR_BAD_ARG;
    *out = nullptr;
    zk_pairing_key* key = nullptr;
    const int rc = zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return key_new<decltype(cv)>(h, tau_h, &key); });
    *out = key;
    return rc;
}

void zk_pairing_key_free(void* handle) {
    zk_pairing_key* key = (zk_pairing_key*)handle;
    if (!key) return;
    for (const auto& d : key->dev) {
        int prev = -1;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d.device && hipSetDevice(d.device) != hipSuccess) continue;
        (void)hipFree(d.base);                                       // waits for the device: nothing queued still reads the tables
        if (prev >= 0 && prev != d.device) (void)hipSetDevice(prev);
    }
    delete key;
}

int zk_kzg_pairing_check(const void* handle, const uint64_t* L_xy, int L_inf, const uint64_t* R_xy, int R_inf, int* ok) {
    const zk_pairing_key* key = (const zk_pairing_key*)handle;
    if (!key || !L_xy || !R_xy || !ok) return ZK_ERR_BAD_ARG;
    return zk_on_curve(key->curve, ZK_ERR_BAD_ARG, [&](auto cv) {
        typedef typename PairOf<decltype(cv)>::T PR;
        if (!g1_reduced<decltype(cv)>(L_xy, L_inf != 0) || !g1_reduced<decltype(cv)>(R_xy, R_inf != 0)) return (int)ZK_ERR_BAD_ARG;
        *ok = check_one<PR>(key->steps.data(), (int)key->steps.size(), key->lines[1].data(), key->lines[0].data(), (const uint32_t*)L_xy,
                            L_inf != 0, (const uint32_t*)R_xy, R_inf != 0)
                  ? 1
                  : 0;
        return (int)ZK_OK;
    });
}

int zk_pairing_gt(const void* handle, int which, const uint64_t* P_xy, int P_inf, uint64_t* out) {
    const zk_pairing_key* key = (const zk_pairing_key*)handle;
    if (!key || !P_xy || !out || (which != 0 && which != 1)) return ZK_ERR_BAD_ARG;
    return zk_on_curve(key->curve, ZK_ERR_BAD_ARG, [&](auto cv) {
        typedef typename PairOf<decltype(cv)>::T PR;
        if (!g1_reduced<decltype(cv)>(P_xy, P_inf != 0)) return (int)ZK_ERR_BAD_ARG;
        gt_one<PR>(key->steps.data(), (int)key->steps.size(), key->lines[which].data(), (const uint32_t*)P_xy, P_inf != 0, (uint32_t*)out);
        return (int)ZK_OK;
    });
}

int zk_kzg_pairing_check_batch_dev(zk_ctx* c, void* handle, const void* d_L, const uint8_t* d_L_inf, const void* d_R,
                                   const uint8_t* d_R_inf, size_t n, uint8_t* d_ok) {
    zk_pairing_key* key = (zk_pairing_key*)handle;
    if (!c || !key) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    if (!d_L || !d_R || !d_ok) return ZK_ERR_BAD_ARG;
    if (n > ((size_t)1 << 31)) return ZK_ERR_UNSUPPORTED;          // one lane per check in one grid
    Guard g(c);
    if (!g.ok) return ZK_ERR_HIP;
    zk_pairing_key::Dev d;
    if (int rc = key_on_device(c, key, d)) return rc;
    return zk_on_curve(key->curve, ZK_ERR_BAD_ARG, [&](auto cv) {
        ProfScope ps(c, "pairing_check_batch");
        hipLaunchKernelGGL(pairing_check_batch<decltype(cv)>, dim3(blocks_of(n, PAIR_T)), dim3(PAIR_T), 0, c->stream, d.steps,
                           (int)key->steps.size(), d.lines[1], d.lines[0], (const uint32_t*)d_L, d_L_inf, (const uint32_t*)d_R, d_R_inf,
                           (uint64_t)n, d_ok);
        ZK_HIP_TRY(hipGetLastError());
        return (int)ZK_OK;
    });
}

int zk_pairing_gt_batch_dev(zk_ctx* c, void* handle, int which, const void* d_P, const uint8_t* d_inf, size_t n, void* d_out) {
    zk_pairing_key* key = (zk_pairing_key*)handle;
    if (!c || !key || (which != 0 && which != 1)) return ZK_ERR_BAD_ARG;
    if (n == 0) return ZK_OK;
    if (!d_P || !d_out) return ZK_ERR_BAD_ARG;
    if (n > ((size_t)1 << 31)) return ZK_ERR_UNSUPPORTED;
    Guard g(c);
    if (!g.ok) return ZK_ERR_HIP;
    zk_pairing_key::Dev d;
    if (int rc = key_on_device(c, key, d)) return rc;
    return zk_on_curve(key->curve, ZK_ERR_BAD_ARG, [&](auto cv) {
        ProfScope ps(c, "pairing_gt_batch");
        hipLaunchKernelGGL(pairing_gt_batch<decltype(cv)>, dim3(blocks_of(n, PAIR_T)), dim3(PAIR_T), 0, c->stream, d.steps,
                           (int)key->steps.size(), d.lines[which], (const uint32_t*)d_P, d_inf, (uint64_t)n, (uint32_t*)d_out);
        ZK_HIP_TRY(hipGetLastError());
        return (int)ZK_OK;
    });
}
