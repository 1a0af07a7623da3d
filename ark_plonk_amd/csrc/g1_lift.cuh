// From an x to a point of y^2 = x^3 + b on the device: the steps the point decoder (verify.hip: g1_decompress) and the hash-to-curve
// derivation of IPA keys (ipa_setup.hip) share -- x as integer words into the device's Montgomery form, x^3 + b, the candidate root
// (both base fields are 3 mod 4), the root a sign flag names by ark's order on canonical integers.  The one definition.  The field is
// the signed-limb form of the MSM base field (fields.cuh); every comparand is a product, as its zero test asks.
#pragma once
#include "ctx.h"

// x (plain integer words, below q) -> the device's Montgomery form, and x^3 + b as a product
template <class Cv>
ZK_D void g1_curve_rhs(const uint32_t* w, typename Cv::FqU& x, typename Cv::FqU& rhs) {
    typedef typename Cv::FqU F;
    typedef typename Cv::FqP FqP;
    constexpr int SAT = F::SAT;
    uint32_t r2[SAT];
#pragma unroll
    for (int k = 0; k < SAT; ++k) r2[k] = FqP::R2(k);
    // from_sat reads the words as x = v R and returns v R'; times R (in that form) is x R'
    x = F::mul(F::from_sat(w), F::from_sat(r2));
    F b = F::one();
    for (uint32_t k = 1; k < FqP::COEFF_B; ++k) b = F::add(b, F::one());
    // every comparand is a product: rhs = (x^3 + b) * 1
    rhs = F::mul(F::add(F::mul(F::sqr(x), x), F::mul(b, F::one())), F::one());
}

// both base fields are 3 mod 4: the candidate root rhs^((q + 1) / 4), and whether it is one
template <class Cv>
ZK_D bool g1_sqrt(const typename Cv::FqU& rhs, typename Cv::FqU& y) {
    typedef typename Cv::FqU F;
    typedef typename Cv::FqP FqP;
    constexpr int SAT = F::SAT;
    uint32_t e[SAT + 1];
    uint64_t carry = 1;
#pragma unroll
    for (int k = 0; k < SAT; ++k) {
        const uint64_t t = (uint64_t)FqP::MOD(k) + carry;
        e[k] = (uint32_t)t;
        carry = t >> 32;
    }
    e[SAT] = (uint32_t)carry;
#pragma unroll
    for (int k = 0; k < SAT; ++k) e[k] = (e[k] >> 2) | (e[k + 1] << 30);
    y = F::pow_words(rhs, e, SAT);
    return F::sub(F::sqr(y), rhs).is_zero_mod();
}

// of (y, -y) the one the flag names: ark's Ord on Fp compares canonical integers, y > q - y  <=>  y > (q - 1) / 2
template <class Cv>
ZK_D typename Cv::FqU g1_pick_root(const typename Cv::FqU& y, bool want_greatest) {
    typedef typename Cv::FqU F;
    typedef typename Cv::FqP FqP;
    constexpr int SAT = F::SAT;
    uint32_t unit[SAT], yw[SAT];
#pragma unroll
    for (int k = 0; k < SAT; ++k) unit[k] = k == 0 ? 1u : 0u;
    const F one_plain = F::split_words(unit);                  // the integer 1: a product with it strips the Montgomery factor
    F::canon_floor(F::mul(y, one_plain)).pack_words(yw);
    bool greatest = false;
    for (int k = SAT - 1; k >= 0; --k) {
        const uint32_t half = (FqP::MOD(k) >> 1) | (k + 1 < SAT ? FqP::MOD(k + 1) << 31 : 0u);
        if (yw[k] != half) {
            greatest = yw[k] > half;
            break;
        }
    }
    return greatest != want_greatest ? F::neg(y) : y;
}

// the row of the point in zk_srs_register_dev's layout (affine Montgomery words)
template <class Cv>
ZK_D void g1_write_lifted(const typename Cv::FqU& x, const typename Cv::FqU& y, uint32_t* dst) {
    typedef typename Cv::FqU F;
    F::canonical_lt2p(x).to_sat(dst);
    F::canonical_lt2p(y).to_sat(dst + F::SAT);
}
