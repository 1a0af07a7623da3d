// Host cost of the G1 group law over the saturated BLS12-381 base field: 20 000 dependent full additions and 20 000 dependent mixed
// additions, the two steps the MSM's host tail, the IPA round and the subgroup check are made of.  No GPU.
//
//   g++ -O3 -std=c++17 tools/host_law_bench.cpp -o host_law_bench && ./host_law_bench
//
// To compare with an earlier law, name a header that defines XYZZ<Fq> / Affine<Fq> with static add / madd / dbl over its own
// "field.cuh" (the form csrc/ec.cuh had before the law had one definition, taken from a checkout of that commit):
//   g++ -O3 -std=c++17 -DOTHER_LAW_HEADER='"<checkout>/ark_plonk_amd/csrc/ec.cuh"' tools/host_law_bench.cpp -o host_law_bench
// The two laws are then timed alternately, RUNS times each; the line of each gives every run, the minimum and the spread
// (max - min) / min.  Both walk the same points, and the program fails if their results differ.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../ark_plonk_amd/csrc/curve_params.h"
#include "../ark_plonk_amd/csrc/ecu.cuh"
#ifdef OTHER_LAW_HEADER
namespace other {
#include OTHER_LAW_HEADER
}
#endif

constexpr int STEPS = 20000, RUNS = 5;
typedef FqBls12_381Params FqP;

template <class Fq>
static Fq coord(uint32_t (*word)(int)) {
    Fq f;
    for (int i = 0; i < Fq::N; ++i) f.v[i] = word(i);
    return f;
}

// microseconds for STEPS dependent full additions (full = true) or mixed additions of the generator; the sum comes back in `out`
template <class P, class A, class Fq>
static double run(bool full, uint32_t* out) {
    A g;
    g.x = coord<Fq>(FqP::GX);
    g.y = coord<Fq>(FqP::GY);
    const P q = P::dbl(P::dbl(P::from_affine(g)));      // 4G with ZZ != 1: no operand of the full addition is affine
    P acc = P::from_affine(g);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < STEPS; ++i) acc = full ? P::add(acc, q) : P::madd(acc, g);
    const auto t1 = std::chrono::steady_clock::now();
    A a;
    acc.to_affine(a);
    memcpy(out, a.x.v, sizeof a.x.v);
    memcpy(out + Fq::N, a.y.v, sizeof a.y.v);
    return std::chrono::duration<double, std::micro>(t1 - t0).count();
}

static void report(const char* name, const double* t) {
    double lo = t[0], hi = t[0];
    printf("%-28s", name);
    for (int r = 0; r < RUNS; ++r) {
        printf(" %9.1f", t[r]);
        lo = t[r] < lo ? t[r] : lo;
        hi = t[r] > hi ? t[r] : hi;
    }
    printf("   min %9.1f us  %6.4f us/add  spread %.4f\n", lo, lo / STEPS, (hi - lo) / lo);
}

int main() {
    typedef Fp<FqP> Fq;
    uint32_t res[2][2 * Fq::N];
    int bad = 0;
    for (int full = 1; full >= 0; --full) {
        double t_new[RUNS], t_other[RUNS];
        for (int r = 0; r < RUNS; ++r) {
#ifdef OTHER_LAW_HEADER
            typedef other::Fp<FqP> FqO;
            t_other[r] = run<other::XYZZ<FqO>, other::Affine<FqO>, FqO>(full, res[1]);
#endif
            t_new[r] = run<XYZZu<Fq>, AffineU<Fq>, Fq>(full, res[0]);
#ifdef OTHER_LAW_HEADER
            bad |= memcmp(res[0], res[1], sizeof res[0]) != 0;
#endif
        }
#ifdef OTHER_LAW_HEADER
        report(full ? "full add, other law" : "mixed add, other law", t_other);
#endif
        report(full ? "full add, ecu.cuh over Fp" : "mixed add, ecu.cuh over Fp", t_new);
    }
    if (bad) printf("FAIL: the two laws disagree\n");
    return bad;
}
