// What the three field forms (field.cuh, fieldu.cuh, fields.cuh) share that does not depend on how a limb is stored: the exponentiation
// loop, the Fermat exponent, and the regrouping of narrower limbs into 32-bit words.  The members of Fp / Fu / Fs that carry
// these names forward here; the Montgomery products stay with each form.
#pragma once
#include "zk_common.h"

// a^e for a little-endian 32-bit-word exponent (square-and-multiply, most significant bit first); zk_pow_words(a, e, 0) = one.
// inverse and pow_u64 call it directly, not through their field's pow_words / pow_limbs.  That is no rule of the design: it only keeps
// the kernels' assembly byte-identical to what the pinned counter files describe (profiles/one_group_law/asm_digests.md; one more call
// level reordered the sums inside the loop).  tests/test_abi.py is what notices a change here.
template <class F>
ZK_HD F zk_pow_words(const F& a, const uint32_t* e, int n) {
    F r = F::one();
    bool started = false;
    for (int i = n - 1; i >= 0; --i)
        for (int b = 31; b >= 0; --b) {
            if (started) r = F::sqr(r);
            if ((e[i] >> b) & 1u) {
                r = F::mul(r, a);
                started = true;
            }
        }
    return r;
}

// e -= 2 over N little-endian words: the Fermat exponent p - 2 from the words of p.  Every word takes part, with no early way out of
// the loop, so that for a modulus known at compile time the exponent is one too
template <int N>
ZK_HD void zk_words_minus_two(uint32_t (&e)[N]) {
    uint32_t borrow = 2;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t t = (uint64_t)e[i] - borrow;
        e[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 32) & 1u;
    }
}

// NL limbs of BITS bits, each in [0, 2^BITS) below the top one, value below 2^(32 SAT) -> SAT 32-bit words.  Word j holds bits
// [32j, 32j + 32): pieces of up to three limbs.  (The way in, split_words, stays with each form: through a shared template the base
// conversion kernel of msm_accumulate.hip no longer compiled to the same instructions -- profiles/one_group_law/asm_digests.md.)
template <int BITS, class F>
ZK_HD void zk_pack_words(const F& t, uint32_t* w) {
    constexpr int NL = F::NL, SAT = F::SAT;
#pragma unroll
    for (int j = 0; j < SAT; ++j) {
        const int lo_bit = 32 * j;
        uint64_t acc = 0;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int lb = BITS * i;
            if (lb + BITS <= lo_bit || lb >= lo_bit + 32) continue;
            if (lb >= lo_bit) acc |= (uint64_t)t.v[i] << (lb - lo_bit);
            else acc |= (uint64_t)t.v[i] >> (lo_bit - lb);
        }
        w[j] = (uint32_t)acc;
    }
}
