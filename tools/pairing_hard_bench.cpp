// Host timing of the two forms of the final exponentiation's hard part on BLS12-381 (csrc/pairing.cuh): the x-chain
// (x - 1)^2 (x + q) (x^2 + q^2 - 1) + 3, which gives the power c = 3 of the reference pairing, against square-and-multiply over the
// digits of (q^4 - q^2 + 1) / r (c = 1), and of the generic form on BN254, where it is the one in use.  Both forms must agree:
// chain(f) == generic(f)^3.
//
//   g++ -O3 -std=c++17 -I ark_plonk_amd/csrc tools/pairing_hard_bench.cpp -o pairing_hard_bench && ./pairing_hard_bench
#include <chrono>
#include <cstdio>

#include "curve_params.h"
#include "pairing.cuh"

template <class PR, bool GENERIC>
static double time_final_exp(const typename PR::Fq12& f, typename PR::Fq12& out, int reps) {
    double best = 1e9;
    for (int it = 0; it < reps; ++it) {
        const auto t0 = std::chrono::steady_clock::now();
        PR::template final_exp<GENERIC>(out, f);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        best = ms < best ? ms : best;
    }
    return best;
}

template <class PR>
static void some_element(typename PR::Fq12& f) {
    typedef typename PR::Fq2 Fq2;
    for (int k = 0; k < 6; ++k) {
        Fq2 c = PR::one2();
        for (int j = 0; j <= k + 2; ++j) c = PR::add2(PR::dbl2(c), PR::mul2_xi(c));
        f.c[k / 3].c[k % 3] = PR::sqr2(c);
    }
}

int main() {
    typedef Pairing<PairingBls12_381Params, Fp<FqBls12_381Params>> Bls;
    typedef Pairing<PairingBn254Params, Fp<FqBn254Params>> Bn;
    {
        Bls::Fq12 f, chain, gen, cube;
        some_element<Bls>(f);
        const double t_chain = time_final_exp<Bls, false>(f, chain, 20);
        const double t_gen = time_final_exp<Bls, true>(f, gen, 20);
        Bls::sqr12(cube, gen);
        Bls::mul12(cube, cube, gen);
        bool same = true;
        for (int k = 0; k < 6; ++k) same = same && Bls::eq2(cube.c[k / 3].c[k % 3], chain.c[k / 3].c[k % 3]);
        std::printf("{\"curve\": \"bls12_381\", \"final_exp_x_chain_ms\": %.3f, \"final_exp_generic_ms\": %.3f, \"chain_is_generic_cubed\": %s}\n",
                    t_chain, t_gen, same ? "true" : "false");
        if (!same) return 1;
    }
    {
        Bn::Fq12 f, gen;
        some_element<Bn>(f);
        std::printf("{\"curve\": \"bn254\", \"final_exp_generic_ms\": %.3f}\n", time_final_exp<Bn, true>(f, gen, 20));
    }
    return 0;
}
