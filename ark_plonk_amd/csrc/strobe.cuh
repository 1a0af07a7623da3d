// merlin 3.0's sponge, once, for the host (wire.hip) and the device (replay.hip): Keccak-f[1600], the STROBE-128 operations merlin uses
// (meta-AD / AD / PRF) and the two transcript operations on top of them (append_message, challenge_bytes).  merlin is a crates.io
// dependency absent from the reference tree; this restates its published behaviour and tests pin it on its conformance vector.
//
// The operations are templates over a SPONGE: a small value, passed and returned by value so that a device caller keeps it in
// registers, that names where the 200 state bytes live and carries the byte cursor:
//     pos, pos_begin, cur_flags      STROBE's cursor, integers
//     xor_byte(p, b)                 state[p] ^= b
//     take_byte(p)                   returns state[p] and clears it
//     permute()                      Keccak-f[1600] over the 200 bytes read as 25 little-endian 64-bit words
// HostSponge (below) is a view of a uint8_t[200]; the device's keeps a lane's bytes in LDS (replay.hip).
// On the device everything here is inlined into its caller, and a device sponge makes permute() a CALL of a function that calls
// nothing itself (a function that calls another saves its return address through scratch memory, a leaf does not).
#pragma once
#include "zk_common.h"

// ------------------------------------------------------------------------------------------ Keccak-f[1600]
ZK_HD constexpr uint64_t keccak_rc(int round) {
    constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                                 0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return RC[round];
}
ZK_HD constexpr int keccak_rot(int lane) {
    constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return ROT[lane];
}
ZK_HD constexpr uint64_t keccak_rol(uint64_t x, int s) { return s ? (x << s) | (x >> (64 - s)) : x; }

// Every loop has constant bounds and is unrolled, so every index, rotation and round constant is a literal: the 25 words of a device
// caller stay in registers (an array indexed at run time would go to scratch memory).  The host keeps the 24 rounds a loop -- unrolled
// they are most of its first-level instruction cache -- and unrolls what is inside a round.
ZK_HD void keccak_f1600(uint64_t (&st)[25]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#else
#pragma nounroll
#endif
    for (int round = 0; round < 24; ++round) {
        uint64_t c[5], d[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = st[x] ^ st[x + 5] ^ st[x + 10] ^ st[x + 15] ^ st[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ keccak_rol(c[(x + 1) % 5], 1);
#pragma unroll
        for (int i = 0; i < 25; ++i) st[i] ^= d[i % 5];
        // rho + pi: lane (x, y) -> (y, 2x + 3y)
#pragma unroll
        for (int x = 0; x < 5; ++x) {
#pragma unroll
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rol(st[x + 5 * y], keccak_rot(x + 5 * y));
        }
#pragma unroll
        for (int y = 0; y < 5; ++y) {
#pragma unroll
            for (int x = 0; x < 5; ++x) st[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        }
        st[0] ^= keccak_rc(round);
    }
}

// ------------------------------------------------------------------------------------------ STROBE-128 (merlin's subset)
constexpr uint32_t STROBE_R = 166;
constexpr uint32_t STROBE_I = 1, STROBE_A = 2, STROBE_C = 4, STROBE_T = 8, STROBE_M = 16, STROBE_K = 32;

// the state of a transcript at rest: what zk_transcript holds and what a kernel takes as its seed
struct StrobeState {
    uint8_t state[200];
    uint8_t pos, pos_begin, cur_flags;
};

// the host's sponge: a view of a StrobeState's bytes; the cursor travels in the value and is written back by save()
struct HostSponge {
    uint8_t* st;
    uint32_t pos, pos_begin, cur_flags;
    explicit HostSponge(StrobeState& s) : st(s.state), pos(s.pos), pos_begin(s.pos_begin), cur_flags(s.cur_flags) {}
    void save(StrobeState& s) const {
        s.pos = (uint8_t)pos;
        s.pos_begin = (uint8_t)pos_begin;
        s.cur_flags = (uint8_t)cur_flags;
    }
    void xor_byte(uint32_t p, uint32_t b) const { st[p] ^= (uint8_t)b; }
    uint32_t take_byte(uint32_t p) const {
        const uint8_t b = st[p];
        st[p] = 0;
        return b;
    }
    void permute() const {
        uint64_t w[25];
        for (int i = 0; i < 25; ++i) {
            w[i] = 0;
            for (int b = 0; b < 8; ++b) w[i] |= (uint64_t)st[8 * i + b] << (8 * b);
        }
        keccak_f1600(w);
        for (int i = 0; i < 25; ++i)
            for (int b = 0; b < 8; ++b) st[8 * i + b] = (uint8_t)(w[i] >> (8 * b));
    }
};

template <class S>
ZK_HD S strobe_run_f(S s) {
    s.xor_byte(s.pos, s.pos_begin);
    s.xor_byte(s.pos + 1, 0x04);
    s.xor_byte(STROBE_R + 1, 0x80);
    s.permute();
    s.pos = 0;
    s.pos_begin = 0;
    return s;
}
template <class S>
ZK_HD S strobe_absorb_byte(S s, uint32_t b) {
    s.xor_byte(s.pos, b);
    if (++s.pos == STROBE_R) s = strobe_run_f(s);
    return s;
}
template <class S>
ZK_HD S strobe_squeeze_byte(S s, uint32_t& b) {
    b = s.take_byte(s.pos);
    if (++s.pos == STROBE_R) s = strobe_run_f(s);
    return s;
}
// n bytes at d
template <class S>
ZK_HD S strobe_absorb(S s, const uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; ++i) s = strobe_absorb_byte(s, d[i]);
    return s;
}
// n zero bytes: the cursor moves, the state does not
template <class S>
ZK_HD S strobe_absorb_zeros(S s, size_t n) {
    for (size_t i = 0; i < n; ++i) s = strobe_absorb_byte(s, 0);
    return s;
}
// the n low bytes of v, least significant first (n <= 8)
template <class S>
ZK_HD S strobe_absorb_le(S s, uint64_t v, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        s = strobe_absorb_byte(s, (uint32_t)v & 0xffu);
        v >>= 8;
    }
    return s;
}
template <class S>
ZK_HD S strobe_squeeze(S s, uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t b;
        s = strobe_squeeze_byte(s, b);
        d[i] = (uint8_t)b;
    }
    return s;
}
// more: continuation of the running operation (same flags by construction here)
template <class S>
ZK_HD S strobe_begin_op(S s, uint32_t flags, bool more) {
    if (more) return s;
    const uint32_t old_begin = s.pos_begin;
    s.pos_begin = s.pos + 1;
    s.cur_flags = flags;
    s = strobe_absorb_byte(s, old_begin);
    s = strobe_absorb_byte(s, flags);
    if ((flags & (STROBE_C | STROBE_K)) && s.pos != 0) s = strobe_run_f(s);
    return s;
}
template <class S>
ZK_HD S strobe_meta_ad(S s, const uint8_t* d, size_t n, bool more) {
    return strobe_absorb(strobe_begin_op(s, STROBE_M | STROBE_A, more), d, n);
}
template <class S>
ZK_HD S strobe_ad(S s, const uint8_t* d, size_t n, bool more) {
    return strobe_absorb(strobe_begin_op(s, STROBE_A, more), d, n);
}
template <class S>
ZK_HD S strobe_prf(S s, uint8_t* d, size_t n, bool more) {
    return strobe_squeeze(strobe_begin_op(s, STROBE_I | STROBE_A | STROBE_C, more), d, n);
}
// Strobe128::new(label): the sponge must be over 200 zero bytes with a zero cursor
template <class S>
ZK_HD S strobe_init(S s, const uint8_t* label, size_t len) {
    const uint8_t head[18] = {1, (uint8_t)(STROBE_R + 2), 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
    for (uint32_t i = 0; i < 18; ++i) s.xor_byte(i, head[i]);
    s.permute();
    return strobe_meta_ad(s, label, len, false);
}

// ------------------------------------------------------------------------------------------ merlin's Transcript
// The head of append_message / challenge_bytes: meta-AD(label), meta-AD(LE32(n), more), then the operation that takes (`flags` =
// STROBE_A: AD) or gives (STROBE_I | STROBE_A | STROBE_C: PRF) the n bytes themselves -- which the caller absorbs or squeezes next,
// from wherever they are (a buffer, words in registers, zeros).
template <class S>
ZK_HD S transcript_op_begin(S s, const uint8_t* label, size_t label_len, size_t n, uint32_t flags) {
    s = strobe_meta_ad(s, label, label_len, false);
    s = strobe_absorb_le(strobe_begin_op(s, STROBE_M | STROBE_A, true), (uint32_t)n, 4);
    return strobe_begin_op(s, flags, false);
}
template <class S>
ZK_HD S transcript_append_begin(S s, const uint8_t* label, size_t label_len, size_t msg_len) {
    return transcript_op_begin(s, label, label_len, msg_len, STROBE_A);
}
template <class S>
ZK_HD S transcript_challenge_begin(S s, const uint8_t* label, size_t label_len, size_t out_len) {
    return transcript_op_begin(s, label, label_len, out_len, STROBE_I | STROBE_A | STROBE_C);
}
template <class S>
ZK_HD S transcript_append(S s, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
    return strobe_absorb(transcript_append_begin(s, label, label_len, msg_len), msg, msg_len);
}
template <class S>
ZK_HD S transcript_challenge(S s, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
    return strobe_squeeze(transcript_challenge_begin(s, label, label_len, out_len), out, out_len);
}
