// Stand-alone driver for AddressSanitizer + UBSan over the verifier's parse and replay (csrc/wire.hip: zk_proof_replay_batch), built
// and run by tests/test_verifier_host.py.  A well-formed proof is cut at every length, its length fields are set to values around what
// is left of the buffer and to huge ones, and random bytes are flipped; every variant lives in a heap block of exactly its size, so a
// read past the end is a report.  Every call must return ZK_OK with a status the header names.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ark_plonk_amd.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void put_u64(std::string& s, uint64_t v) {
    for (int b = 0; b < 8; ++b) s.push_back((char)(v >> (8 * b)));
}

static std::string well_formed(int curve) {
    const size_t g = zk_g1_compressed_size(curve), f = zk_fr_serialized_size(curve);
    std::string s;
    for (int i = 0; i < 15; ++i) {
        std::string p(g, '\0');
        p[g - 1] = 0x40;                                  // infinity: decodes without a curve
        s += p;
        if (i >= 13) s.push_back('\0');
    }
    s += std::string(16 * f, '\x01');
    const char* labels[7] = {"q_arith_eval", "q_c_eval", "q_l_eval", "q_r_eval", "a_next_eval", "b_next_eval", "d_next_eval"};
    put_u64(s, 7);
    for (const char* l : labels) {
        put_u64(s, strlen(l));
        s += l;
        s += std::string(f, '\x02');
    }
    return s;
}

static long calls = 0;
static int seen[8] = {0};

static void run(const zk_transcript* t, int curve, const std::string& bytes, size_t n_pi) {
    uint8_t* heap = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
    memcpy(heap, bytes.data(), bytes.size());
    const uint8_t* proofs[1] = {heap};
    const size_t lens[1] = {bytes.size()};
    const uint64_t off[2] = {0, n_pi};
    const uint64_t pos[3] = {1, 5, 9};
    uint64_t vals[12];
    for (int i = 0; i < 12; ++i) vals[i] = i % 4 == 0 ? 7 : 0;
    uint64_t ch[4 * ZK_VERIFY_N_CHALLENGES], ev[4 * ZK_VERIFY_N_EVALS];
    std::vector<uint8_t> pts(15 * zk_g1_compressed_size(curve));
    uint8_t st = 0xff;
    const int rc = zk_proof_replay_batch(t, curve, 1, proofs, lens, off, pos, vals, ch, ev, (calls & 1) ? pts.data() : nullptr, &st);
    free(heap);
    if (rc != ZK_OK || st > ZK_PROOF_BAD_PUBLIC_INPUTS) {
        fprintf(stderr, "rc %d status %d at length %zu\n", rc, (int)st, bytes.size());
        exit(1);
    }
    ++seen[st];
    ++calls;
}

int main() {
    for (int curve = 0; curve < 2; ++curve) {
        zk_transcript* t = zk_transcript_new((const uint8_t*)"fuzz", 4);
        zk_transcript_circuit_domain_sep(t, 32);
        const std::string good = well_formed(curve);
        const size_t g = zk_g1_compressed_size(curve), f = zk_fr_serialized_size(curve);
        const size_t cnt = 15 * g + 2 + 16 * f;
        const int ok_before = seen[ZK_PROOF_OK];
        run(t, curve, good, 0);
        run(t, curve, good, 3);
        if (seen[ZK_PROOF_OK] != ok_before + 2) {
            fprintf(stderr, "the well-formed proof was not accepted:");
            for (int k = 0; k < 8; ++k) fprintf(stderr, " status %d x %d", k, seen[k]);
            fprintf(stderr, "\n");
            return 1;
        }
        for (size_t len = 0; len <= good.size(); ++len) run(t, curve, good.substr(0, len), len % 4);
        run(t, curve, good + std::string(1, '\0'), 0);
        // the custom count, and the length of every label, around what the buffer holds and far beyond it
        std::vector<size_t> fields = {cnt};
        for (size_t p = cnt + 8; p + 8 <= good.size();) {
            uint64_t ll = 0;
            for (int b = 0; b < 8; ++b) ll |= (uint64_t)(uint8_t)good[p + b] << (8 * b);
            fields.push_back(p);
            p += 8 + ll + f;
        }
        for (size_t p : fields) {
            const uint64_t left = good.size() - p - 8;
            const uint64_t vals[] = {0, 1, 6, 8, left - 1, left, left + 1, left - f, left - f + 1, left / (8 + f), left / (8 + f) + 1,
                                     0xffffffffull, 1ull << 32, 1ull << 63, ~0ull, ~0ull - 7, ~0ull - left};
            for (uint64_t v : vals) {
                std::string s = good;
                for (int b = 0; b < 8; ++b) s[p + b] = (char)(v >> (8 * b));
                run(t, curve, s, 1);
                run(t, curve, s.substr(0, s.size() - 1), 1);
            }
        }
        for (int it = 0; it < 20000; ++it) {
            std::string s = good.substr(0, (it & 3) == 0 ? rnd() % (good.size() + 1) : good.size());
            const int flips = 1 + (int)(rnd() % 4);
            for (int k = 0; k < flips && !s.empty(); ++k) s[rnd() % s.size()] = (char)rnd();
            run(t, curve, s, rnd() % 4);
        }
        zk_transcript_free(t);
    }
    for (int k = ZK_PROOF_OK; k <= ZK_PROOF_BAD_COUNT; ++k)
        if (!seen[k]) {
            fprintf(stderr, "status %d never seen\n", k);
            return 1;
        }
    printf("fuzz_replay ok: %ld calls\n", calls);
    return 0;
}
