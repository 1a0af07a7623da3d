// The two hashes of csrc/h2c.cuh on the host: a stand-alone program (tests/test_ipa_setup.py builds it with the host compiler and
// -fsanitize=address,undefined and compares its output with hashlib).  Prints one line per message: the name of the hash, the message
// in hex, the digest in hex.  Messages: counting bytes 0, 1, 2, ... of lengths 0, 1, 10, 18 and 26; 26 bytes of 0xff; and -- through
// h2c_generator_digest, the form the kernel calls -- the preimages of (i, attempt) = (0, 0), (1, 3) and (2^32 + 5, 40).
#include <cstdio>
#include <cstring>

#include "h2c.cuh"

static void hex(const uint8_t* p, size_t n) {
    for (size_t k = 0; k < n; ++k) printf("%02x", p[k]);
}

static void run(const uint8_t* msg, uint32_t len) {
    uint8_t block[128];
    memset(block, 0, sizeof block);
    memcpy(block, msg, len);
    uint32_t m32[16], d32[8];
    uint64_t m64[16], d64[8];
    for (int k = 0; k < 16; ++k) {
        m32[k] = 0;
        m64[k] = 0;
        for (int b = 0; b < 4; ++b) m32[k] |= (uint32_t)block[4 * k + b] << (8 * b);
        for (int b = 0; b < 8; ++b) m64[k] |= (uint64_t)block[8 * k + b] << (8 * b);
    }
    h2c_blake2s_block(m32, len, d32);
    h2c_blake2b_block(m64, len, d64);
    uint8_t out[64];
    for (int k = 0; k < 32; ++k) out[k] = (uint8_t)(d32[k / 4] >> (8 * (k % 4)));
    printf("blake2s ");
    hex(msg, len);
    printf(" ");
    hex(out, 32);
    printf("\n");
    for (int k = 0; k < 64; ++k) out[k] = (uint8_t)(d64[k / 8] >> (8 * (k % 8)));
    printf("blake2b ");
    hex(msg, len);
    printf(" ");
    hex(out, 64);
    printf("\n");
}

template <int DIGEST>
static void generator(const char* name, uint64_t i, uint32_t attempt) {
    uint32_t w[16];
    h2c_generator_digest<DIGEST>(i, attempt, w);
    uint8_t out[64];
    for (int k = 0; k < 64; ++k) out[k] = (uint8_t)(w[k / 4] >> (8 * (k % 4)));
    printf("%s generator %llu %u ", name, (unsigned long long)i, attempt);
    hex(out, 64);
    printf("\n");
}

int main() {
    uint8_t msg[26];
    for (int k = 0; k < 26; ++k) msg[k] = (uint8_t)k;
    const uint32_t lens[5] = {0, 1, 10, 18, 26};
    for (uint32_t len : lens) run(msg, len);
    memset(msg, 0xff, sizeof msg);
    run(msg, 26);
    const uint64_t is[3] = {0, 1, ((uint64_t)1 << 32) + 5};
    const uint32_t attempts[3] = {0, 3, 40};
    for (int k = 0; k < 3; ++k) {
        generator<H2C_BLAKE2S>("blake2s", is[k], attempts[k]);
        generator<H2C_BLAKE2B>("blake2b", is[k], attempts[k]);
    }
    printf("blake2_check ok\n");
    return 0;
}
