// Stand-alone host check of the chained products of fields.cuh: Fs<P, true>::mul / sqr / dot2 (one accumulator per column, the high-half
// digit cut from the unbiased sum) against the plain Fs<P> ones, limb for limb, on both moduli.  Operands: random almost-balanced limbs,
// every limb at either end of the almost-balanced range (|v| = 2^29 + 2, all signs equal, alternating, and the doubled limbs of sqr with
// them), zero, one, and p's own limbs.  The two forms add the same terms into one 64-bit sum, so they agree wherever neither overflows;
// built with -fsanitize=undefined by tests/test_field_chains_host.py, a signed overflow in either form ends the run.
// Prints the number of comparisons and exits 0, or prints the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../ark_plonk_amd/csrc/curve_params.h"
#include "../../ark_plonk_amd/csrc/fields.cuh"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

template <class P>
static long check(const char* name) {
    typedef Fs<P> A;
    typedef Fs<P, true> C;
    static_assert(sizeof(A) == sizeof(C), "same limbs");
    constexpr int NL = A::NL;
    constexpr int32_t E = (1 << 29) + 2;
    constexpr int FIXED = 9, N = FIXED + 300;
    static A ops[N];
    for (int i = 0; i < NL; ++i) {
        ops[0].v[i] = 0;
        ops[1].v[i] = (uint32_t)P::ONE(i);
        ops[2].v[i] = (uint32_t)P::MOD(i);
        ops[3].v[i] = (uint32_t)P::NMOD(i);
        ops[4].v[i] = (uint32_t)E;
        ops[5].v[i] = (uint32_t)-E;
        ops[6].v[i] = (uint32_t)((i & 1) ? E : -E);
        ops[7].v[i] = (uint32_t)((i & 1) ? -E : E);
        ops[8].v[i] = (uint32_t)((i % 3) ? (1 << 29) - 1 : -(1 << 29));
    }
    for (int k = FIXED; k < N; ++k)
        for (int i = 0; i < NL; ++i) ops[k].v[i] = (uint32_t)((int32_t)(rnd() % (2u * E + 1)) - E);
    long n = 0;
    auto same = [&](const A& x, const C& y, const char* op, int i, int j) {
        ++n;
        if (memcmp(x.v, y.v, sizeof(x.v)) == 0) return true;
        printf("%s %s operands %d %d differ\n", name, op, i, j);
        return false;
    };
    auto chained = [](const A& x) {
        C y;
        memcpy(y.v, x.v, sizeof(x.v));
        return y;
    };
    for (int i = 0; i < N; ++i) {
        if (!same(A::sqr(ops[i]), C::sqr(chained(ops[i])), "sqr", i, i)) return -1;
        for (int j = 0; j < N; j += (i < FIXED ? 1 : 7)) {
            if (!same(A::mul(ops[i], ops[j]), C::mul(chained(ops[i]), chained(ops[j])), "mul", i, j)) return -1;
            const int k = (i + 3 * j + 1) % N, l = (5 * i + j + 2) % N;
            if (!same(A::dot2(ops[i], ops[j], ops[k], ops[l]), C::dot2(chained(ops[i]), chained(ops[j]), chained(ops[k]), chained(ops[l])), "dot2", i, j))
                return -1;
        }
    }
    return n;
}

int main() {
    const long a = check<FqBls12_381SParams>("bls12_381"), b = check<FqBn254SParams>("bn254");
    if (a < 0 || b < 0) return 1;
    printf("%ld comparisons equal\n", a + b);
    return 0;
}
