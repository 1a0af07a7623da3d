// The generator derivation of ipa_pc::setup (ark-poly-commit 0.3 `InnerProductArgPC::sample_generators`), the device's statement of
// the rule whose host statement is ark_plonk_amd/ipa.py (generator_preimage, from_random_bytes, sample_generators).  AS RECALLED: the
// crate's source is not vendored, so every encoding below is an assumption, unpinned against it, exactly like ipa.transcript_hash:
//   * generator i hashes D("PC-DL-2020" || u64_le(i)); if the digest is no point, D("PC-DL-2020" || u64_le(i) || u64_le(j)) for
//     j = 0, 1, ... until one is; the generator is affine(cofactor * P);
//   * D is Blake2s-256 or Blake2b-512, unkeyed, sequential mode (RFC 7693);
//   * a digest becomes a point by `GroupAffine::from_random_bytes` over `Fp::from_random_bytes_with_flags::<SWFlags>`: the first
//     min(len, G) bytes in a zeroed buffer of G bytes (G: the byte length of a compressed point), the flags in the top two bits of
//     byte G - 1 (bit 7: y is the larger of (y, -y); bit 6: infinity), x the buffer little-endian with every bit from MODULUS_BITS up
//     cleared.  x >= q, both flags, the infinity flag with x != 0 and a non-residue x^3 + b give no point.  No subgroup check.
//
// The two hashes are one compression each: a preimage is 18 or 26 bytes, so there is one block and no streaming interface.  State and
// message words are indexed by literals only (the sigma schedule is written out), so they stay in registers on the device.
// Host and device: tests/native/blake2_check.cpp compiles this header with the host compiler under ASan + UBSan against hashlib.
#pragma once
#include <stdint.h>

#include "zk_common.h"

enum { H2C_BLAKE2S = 0, H2C_BLAKE2B = 1 };                // the digest ids of the C ABI (ZK_H2C_BLAKE2S, ZK_H2C_BLAKE2B)

// cofactor of G1, little-endian 32-bit words (BLS12-381: 0x396c8c005555e1568c00aaab0000aaab; BN254: 1, never multiplied by)
ZK_HD uint32_t h2c_bls12_381_cofactor_word(int k) {
    return k == 0 ? 0x0000aaabu : k == 1 ? 0x8c00aaabu : k == 2 ? 0x5555e156u : 0x396c8c00u;
}

ZK_HD uint32_t h2c_rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
ZK_HD uint64_t h2c_rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

#define H2C_G32(a, b, c, d, x, y)       \
    a = a + b + (x);                    \
    d = h2c_rotr32(d ^ a, 16);          \
    c = c + d;                          \
    b = h2c_rotr32(b ^ c, 12);          \
    a = a + b + (y);                    \
    d = h2c_rotr32(d ^ a, 8);           \
    c = c + d;                          \
    b = h2c_rotr32(b ^ c, 7);
#define H2C_G64(a, b, c, d, x, y)       \
    a = a + b + (x);                    \
    d = h2c_rotr64(d ^ a, 32);          \
    c = c + d;                          \
    b = h2c_rotr64(b ^ c, 24);          \
    a = a + b + (y);                    \
    d = h2c_rotr64(d ^ a, 16);          \
    c = c + d;                          \
    b = h2c_rotr64(b ^ c, 63);
// one round: the four columns, then the four diagonals, message words in the order one row of sigma names
#define H2C_ROUND(G, s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    G(v0, v4, v8, v12, m[s0], m[s1])                                                       \
    G(v1, v5, v9, v13, m[s2], m[s3])                                                       \
    G(v2, v6, v10, v14, m[s4], m[s5])                                                      \
    G(v3, v7, v11, v15, m[s6], m[s7])                                                      \
    G(v0, v5, v10, v15, m[s8], m[s9])                                                      \
    G(v1, v6, v11, v12, m[s10], m[s11])                                                    \
    G(v2, v7, v8, v13, m[s12], m[s13])                                                     \
    G(v3, v4, v9, v14, m[s14], m[s15])
#define H2C_ROUNDS_10(G)                                               \
    H2C_ROUND(G, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15) \
    H2C_ROUND(G, 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3) \
    H2C_ROUND(G, 11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4) \
    H2C_ROUND(G, 7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8) \
    H2C_ROUND(G, 9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13) \
    H2C_ROUND(G, 2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9) \
    H2C_ROUND(G, 12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11) \
    H2C_ROUND(G, 13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10) \
    H2C_ROUND(G, 6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5) \
    H2C_ROUND(G, 10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)

// Blake2s-256 of a message of len <= 64 bytes given as the 16 little-endian words of its one (zero-padded) block
ZK_HD void h2c_blake2s_block(const uint32_t (&m)[16], uint32_t len, uint32_t (&out)[8]) {
    const uint32_t h0 = 0x6a09e667u ^ 0x01010020u, h1 = 0xbb67ae85u, h2 = 0x3c6ef372u, h3 = 0xa54ff53au, h4 = 0x510e527fu, h5 = 0x9b05688cu,
                   h6 = 0x1f83d9abu, h7 = 0x5be0cd19u;              // IV ^ parameter block: 32-byte digest, no key, fanout = depth = 1
    uint32_t v0 = h0, v1 = h1, v2 = h2, v3 = h3, v4 = h4, v5 = h5, v6 = h6, v7 = h7;
    uint32_t v8 = 0x6a09e667u, v9 = 0xbb67ae85u, v10 = 0x3c6ef372u, v11 = 0xa54ff53au;
    uint32_t v12 = 0x510e527fu ^ len, v13 = 0x9b05688cu, v14 = ~0x1f83d9abu, v15 = 0x5be0cd19u;     // t = len, the last block
    H2C_ROUNDS_10(H2C_G32)
    out[0] = h0 ^ v0 ^ v8;
    out[1] = h1 ^ v1 ^ v9;
    out[2] = h2 ^ v2 ^ v10;
    out[3] = h3 ^ v3 ^ v11;
    out[4] = h4 ^ v4 ^ v12;
    out[5] = h5 ^ v5 ^ v13;
    out[6] = h6 ^ v6 ^ v14;
    out[7] = h7 ^ v7 ^ v15;
}

// Blake2b-512 of a message of len <= 128 bytes given as the 16 little-endian 64-bit words of its one block: 12 rounds, sigma's rows 0
// and 1 again after the tenth
ZK_HD void h2c_blake2b_block(const uint64_t (&m)[16], uint32_t len, uint64_t (&out)[8]) {
    const uint64_t h0 = 0x6a09e667f3bcc908ull ^ 0x01010040ull, h1 = 0xbb67ae8584caa73bull, h2 = 0x3c6ef372fe94f82bull, h3 = 0xa54ff53a5f1d36f1ull,
                   h4 = 0x510e527fade682d1ull, h5 = 0x9b05688c2b3e6c1full, h6 = 0x1f83d9abfb41bd6bull, h7 = 0x5be0cd19137e2179ull;
    uint64_t v0 = h0, v1 = h1, v2 = h2, v3 = h3, v4 = h4, v5 = h5, v6 = h6, v7 = h7;
    uint64_t v8 = 0x6a09e667f3bcc908ull, v9 = 0xbb67ae8584caa73bull, v10 = 0x3c6ef372fe94f82bull, v11 = 0xa54ff53a5f1d36f1ull;
    uint64_t v12 = 0x510e527fade682d1ull ^ len, v13 = 0x9b05688c2b3e6c1full, v14 = ~0x1f83d9abfb41bd6bull, v15 = 0x5be0cd19137e2179ull;
    H2C_ROUNDS_10(H2C_G64)
    H2C_ROUND(H2C_G64, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    H2C_ROUND(H2C_G64, 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    out[0] = h0 ^ v0 ^ v8;
    out[1] = h1 ^ v1 ^ v9;
    out[2] = h2 ^ v2 ^ v10;
    out[3] = h3 ^ v3 ^ v11;
    out[4] = h4 ^ v4 ^ v12;
    out[5] = h5 ^ v5 ^ v13;
    out[6] = h6 ^ v6 ^ v14;
    out[7] = h7 ^ v7 ^ v15;
}

#undef H2C_ROUNDS_10
#undef H2C_ROUND
#undef H2C_G64
#undef H2C_G32

// The preimage of attempt `attempt` (0, 1, ...) at generator i, as the integer tag | i << 80 | j << 144 cut into 32-bit words:
// attempt 0 is "PC-DL-2020" || u64_le(i), 18 bytes; attempt a >= 1 appends u64_le(a - 1), 26 bytes.  Returns the length.
ZK_HD uint32_t h2c_preimage_words(uint64_t i, uint32_t attempt, uint32_t (&w)[7]) {
    const uint64_t j = attempt ? (uint64_t)(attempt - 1) : 0;
    w[0] = 0x442d4350u;                                     // "PC-D"
    w[1] = 0x30322d4cu;                                     // "L-20"
    w[2] = 0x3032u | (uint32_t)(i << 16);                   // "20", then i
    w[3] = (uint32_t)(i >> 16);
    w[4] = (uint32_t)(i >> 48) | (uint32_t)(j << 16);
    w[5] = (uint32_t)(j >> 16);
    w[6] = (uint32_t)(j >> 48);
    return attempt ? 26u : 18u;
}

// The first N 32-bit words of D(preimage), zero beyond the digest's own length (the zeroed buffer of from_random_bytes)
template <int DIGEST, int N>
ZK_HD void h2c_generator_digest(uint64_t i, uint32_t attempt, uint32_t (&out)[N]) {
    uint32_t p[7];
    const uint32_t len = h2c_preimage_words(i, attempt, p);
    if (DIGEST == H2C_BLAKE2S) {
        const uint32_t m[16] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t d[8];
        h2c_blake2s_block(m, len, d);
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = k < 8 ? d[k < 8 ? k : 0] : 0u;
    } else {
        const uint64_t m[16] = {p[0] | (uint64_t)p[1] << 32, p[2] | (uint64_t)p[3] << 32, p[4] | (uint64_t)p[5] << 32, p[6], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t d[8];
        h2c_blake2b_block(m, len, d);
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = k < 16 ? (uint32_t)(d[k < 16 ? k / 2 : 0] >> (32 * (k & 1))) : 0u;
    }
}

// The checks of from_random_bytes that need no field arithmetic, on the G-byte buffer as SAT little-endian words.  Leaves x (every
// bit from MODULUS_BITS up cleared) in w and the two flag bits in `flags` (bit 1: y is the larger; bit 0: infinity).  MOD(k): word k
// of q.  Order as in ark: the field element is read first (x >= q), then the flags.
enum { H2C_X_ON_CURVE_PENDING = 0, H2C_INFINITY = 1, H2C_X_NOT_REDUCED = 2, H2C_BAD_FLAGS = 3, H2C_INFINITY_X_NONZERO = 4 };
template <class FqP, int SAT>
ZK_HD int h2c_classify(uint32_t (&w)[SAT], uint32_t& flags) {
    constexpr int TOP_BITS = FqP::BITS - 32 * (SAT - 1);       // bits of x in the top word: 29 on BLS12-381, 30 on BN254
    static_assert(TOP_BITS > 0 && TOP_BITS <= 30, "the flags lie above the modulus' bits in the top word");
    flags = w[SAT - 1] >> 30;
    w[SAT - 1] &= (1u << TOP_BITS) - 1u;
    bool below = false, decided = false;
    uint32_t any = 0;
#pragma unroll
    for (int k = SAT - 1; k >= 0; --k) {
        const uint32_t m = FqP::MOD(k);
        if (!decided && w[k] != m) {
            below = w[k] < m;
            decided = true;
        }
        any |= w[k];
    }
    if (!below) return H2C_X_NOT_REDUCED;
    if (flags == 3u) return H2C_BAD_FLAGS;
    if (flags & 1u) return any ? H2C_INFINITY_X_NONZERO : H2C_INFINITY;
    return H2C_X_ON_CURVE_PENDING;
}
