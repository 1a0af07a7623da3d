// Constants of the evaluation domain and of the permutation argument, defined once for every unit that needs them: the root of unity
// of a size-2^k domain and its two-adicity guard, the coset generator, the permutation cosets K_0..K_3, and the identity encoding
// K_w * omega^row that compile.hip writes sigma with and check.hip decodes it with.
#pragma once
#include "fr_io.cuh"

namespace {

// generator of the size-2^log_n subgroup: ROOT has order 2^TWO_ADICITY (log_n <= TWO_ADICITY: domain_log_ok)
template <class FrP, class Fr>
ZK_HD Fr domain_root(uint32_t log_n) {
    Fr r;
#pragma unroll
    for (int i = 0; i < Fr::N; ++i) r.v[i] = FrP::ROOT(i);
    for (uint32_t k = log_n; k < (uint32_t)FrP::TWO_ADICITY; ++k) r = Fr::sqr(r);
    return r;
}
template <class Cv>
typename Cv::Fr domain_root(uint32_t log_n) { return domain_root<typename Cv::FrP, typename Cv::Fr>(log_n); }
// false: the caller's ZK_ERR_DOMAIN_TOO_LARGE
template <class Cv>
bool domain_log_ok(uint32_t log_n) { return log_n <= (uint32_t)Cv::FrP::TWO_ADICITY; }
template <class Cv>
typename Cv::Fr coset_gen() { return Cv::Fr::from_u32(Cv::FrP::GENERATOR); }

constexpr uint32_t PERM_K[4] = {1, 7, 13, 17};    // permutation/constants.rs:12-22

// ---- the identity encoding: position (wire w, row) of the 4n cells <-> K_w * omega^row
// consts: K_0..K_3 (Montgomery), then omega^(2^j), j < ID_MAX_LOG_N.  omega^row is the product of omega^(2^j) over the set bits of row:
// no n-entry table to build, keep and gather from.
constexpr uint32_t ID_MAX_LOG_N = 28;             // 4n positions and the sentinel fit 32 bits; also BN254's two-adicity
constexpr uint32_t ID_N_CONSTS = 4 + ID_MAX_LOG_N;
template <class Cv>
void fill_id_consts(uint32_t log_n, typename Cv::Fr* cs /* ID_N_CONSTS */) {
    typedef typename Cv::Fr Fr;
    for (int k = 0; k < 4; ++k) cs[k] = Fr::from_u32(PERM_K[k]);
    Fr pw = domain_root<Cv>(log_n);
    for (uint32_t j = 0; j < ID_MAX_LOG_N; ++j) {
        cs[4 + j] = pw;
        pw = Fr::sqr(pw);
    }
}
template <class Fr>
ZK_D Fr id_encode(const void* consts, uint32_t wire, uint32_t row, uint32_t log_n) {
    Fr r = ld_fr<Fr>(consts, wire);
    for (uint32_t j = 0; j < log_n; ++j)
        if ((row >> j) & 1u) r = Fr::mul(r, ld_fr<Fr>(consts, 4 + j));
    return r;
}
template <class Fr>
ZK_D Fr id_omega_pow(const void* consts, uint32_t row, uint32_t log_n) { return id_encode<Fr>(consts, 0, row, log_n); }   // K_0 = 1

}  // namespace
