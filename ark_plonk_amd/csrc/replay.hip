// The verifier's stage 2 on the device: the parse and transcript replay of replay_walk.cuh -- the code wire.hip's
// zk_proof_replay_batch runs on the host -- with every proof of a batch in a lane of its own.
//
// One proof per lane, one wave per workgroup.  A replay is some 35 Keccak-f[1600] permutations between byte-wise absorbs whose cursor
// depends on the data (the public-input message comes first and its length varies), so a lane's 200 sponge bytes live in LDS,
// word-interleaved -- word w of lane l at w * 64 + l: lanes in step touch 64 distinct banks, and no barrier is needed because a lane owns
// its column.  A permutation loads the 25 64-bit words into registers, runs the 24 unrolled rounds and stores them back.  The cursor,
// the parse position and everything else per proof are registers: the sponge operations take and return the cursor by value and are
// inlined; the permutation and the field product are the only calls, both of functions that call nothing (no scratch memory).
//
// Lanes fall out of step only where public-input counts or custom labels differ: the wave then runs both sides of a branch one after
// the other until the lanes meet again -- every challenge forces a permutation at the same place of the script.  Out-of-step lanes
// cost time, not correctness; the batch is not sorted to avoid it.
#include "api_internal.h"
#include "replay_walk.cuh"

namespace {

constexpr uint32_t RT = 64;                                 // lanes of a workgroup: one wave
constexpr uint32_t SPONGE_WORDS = 200 / 4;
__shared__ uint32_t lds_sponge[SPONGE_WORDS * RT];          // 12.8 KB: every sponge of the workgroup, a column per lane

__device__ __noinline__ void lds_permute(uint32_t lane) {
    uint64_t w[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) w[i] = (uint64_t)lds_sponge[2 * i * RT + lane] | (uint64_t)lds_sponge[(2 * i + 1) * RT + lane] << 32;
    keccak_f1600(w);
#pragma unroll
    for (int i = 0; i < 25; ++i) {
        lds_sponge[2 * i * RT + lane] = (uint32_t)w[i];
        lds_sponge[(2 * i + 1) * RT + lane] = (uint32_t)(w[i] >> 32);
    }
}

// strobe.cuh's sponge over a lane's column
struct LdsSponge {
    uint32_t lane, pos, pos_begin, cur_flags;
    ZK_D void xor_byte(uint32_t p, uint32_t b) const { lds_sponge[(p >> 2) * RT + lane] ^= b << (8 * (p & 3)); }
    ZK_D uint32_t take_byte(uint32_t p) const {
        const uint32_t sh = 8 * (p & 3), w = lds_sponge[(p >> 2) * RT + lane];
        lds_sponge[(p >> 2) * RT + lane] = w & ~(0xffu << sh);
        return (w >> sh) & 0xffu;
    }
    ZK_D void permute() const { lds_permute(lane); }
};

struct ReplayArgs {
    uint32_t seed[SPONGE_WORDS];                            // the seeded transcript, by value: every lane starts from a copy
    uint32_t pos, pos_begin, cur_flags;
    uint32_t n_proofs;
    const uint8_t* proofs;
    const uint64_t *proof_offsets, *pi_offsets, *pi_positions, *pi_values;
    uint64_t proofs_bytes, n_pi_total;
    uint64_t *challenges, *evals;
    uint8_t *points, *status;
};

template <class Cv>
__global__ void __launch_bounds__(RT) proof_replay(ReplayArgs A) {
    constexpr size_t G = WireSizes<Cv>::FQ_BYTES;
    const uint32_t lane = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * RT + lane;
    if (j >= A.n_proofs) return;
    uint64_t* ch = A.challenges + j * 4 * ZK_VERIFY_N_CHALLENGES;
    uint64_t* ev = A.evals + j * 4 * ZK_VERIFY_N_EVALS;
    uint8_t* pt = A.points ? A.points + j * 15 * G : nullptr;
    // the offsets are data: a range that descends or leaves its buffer is a status, and nothing of it is read
    const uint64_t p0 = A.proof_offsets[j], p1 = A.proof_offsets[j + 1];
    const uint64_t o0 = A.pi_offsets[j], o1 = A.pi_offsets[j + 1];
    uint8_t st = ZK_PROOF_OK;
    ProofLayout lay;
    if (p1 < p0 || p1 > A.proofs_bytes) st = ZK_PROOF_TRUNCATED;
    if (st == ZK_PROOF_OK) st = replay_parse<Cv>(A.proofs + p0, (size_t)(p1 - p0), ev, pt, lay);
    if (st == ZK_PROOF_OK && (o1 < o0 || o1 > A.n_pi_total)) st = ZK_PROOF_BAD_PUBLIC_INPUTS;
    if (st == ZK_PROOF_OK) {
#pragma unroll
        for (uint32_t w = 0; w < SPONGE_WORDS; ++w) lds_sponge[w * RT + lane] = A.seed[w];
        const LdsSponge s = {lane, A.pos, A.pos_begin, A.cur_flags};
        st = replay_script<Cv>(s, A.proofs + p0, lay, A.pi_positions + o0, A.pi_values + 4 * o0, (size_t)(o1 - o0), ch);
    }
    if (st != ZK_PROOF_OK) {                                 // a rejected proof leaves zero rows and infinity encodings behind
        for (int k = 0; k < 4 * ZK_VERIFY_N_CHALLENGES; ++k) ch[k] = 0;
        for (int k = 0; k < 4 * ZK_VERIFY_N_EVALS; ++k) ev[k] = 0;
        if (pt) {
            for (size_t k = 0; k < 15 * G; ++k) pt[k] = k % G == G - 1 ? 0x40 : 0;
        }
    }
    A.status[j] = st;
}

template <class Cv>
int replay_impl(zk_ctx* c, size_t n_proofs, const ReplayArgs& a) {
    ProfScope ps(c, "proof_replay");
    hipLaunchKernelGGL(proof_replay<Cv>, dim3(blocks_of(n_proofs, RT)), dim3(RT), 0, c->stream, a);
    ZK_HIP_TRY(hipGetLastError());
    return ZK_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ C ABI
int zk_proof_replay_batch_dev(zk_ctx* c, const zk_transcript* seeded, int curve_id, size_t n_proofs, const void* d_proofs, size_t proofs_bytes,
                              const void* d_proof_offsets, const void* d_pi_offsets, const void* d_pi_positions, const void* d_pi_values_mont,
                              size_t n_pi_total, void* d_out_challenges_mont, void* d_out_evals_mont, void* d_out_points, void* d_out_status) {
    if (!c || !seeded || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (n_proofs && (!d_proofs || !d_proof_offsets || !d_pi_offsets || !d_out_challenges_mont || !d_out_evals_mont || !d_out_status))
        return ZK_ERR_BAD_ARG;
    if (n_proofs && n_pi_total && (!d_pi_positions || !d_pi_values_mont)) return ZK_ERR_BAD_ARG;
    if (n_proofs >= ((size_t)1 << 31)) return ZK_ERR_UNSUPPORTED;
    if (n_proofs == 0) return ZK_OK;
    ReplayArgs a;
    const StrobeState& s = seeded->st;
    for (uint32_t w = 0; w < SPONGE_WORDS; ++w)
        a.seed[w] = (uint32_t)s.state[4 * w] | (uint32_t)s.state[4 * w + 1] << 8 | (uint32_t)s.state[4 * w + 2] << 16 | (uint32_t)s.state[4 * w + 3] << 24;
    a.pos = s.pos;
    a.pos_begin = s.pos_begin;
    a.cur_flags = s.cur_flags;
    a.n_proofs = (uint32_t)n_proofs;
    a.proofs = (const uint8_t*)d_proofs;
    a.proof_offsets = (const uint64_t*)d_proof_offsets;
    a.pi_offsets = (const uint64_t*)d_pi_offsets;
    a.pi_positions = (const uint64_t*)d_pi_positions;
    a.pi_values = (const uint64_t*)d_pi_values_mont;
    a.proofs_bytes = proofs_bytes;
    a.n_pi_total = n_pi_total;
    a.challenges = (uint64_t*)d_out_challenges_mont;
    a.evals = (uint64_t*)d_out_evals_mont;
    a.points = (uint8_t*)d_out_points;
    a.status = (uint8_t*)d_out_status;
    Guard g(c);
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return replay_impl<decltype(cv)>(c, n_proofs, a); });
}
