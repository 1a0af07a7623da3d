// The verifier's parse and transcript replay of ONE proof (stage 2), once, for the host (wire.hip: zk_proof_replay_batch)
// and the device (replay.hip: one proof per lane): the walk over proof.rs:41-103 followed by the label script of proof.rs:128-300,
// 343-378 on a sponge of strobe.cuh, and the public-input message in front of it.  No allocation, no library call, no array indexed at
// run time: the custom evaluations are walked twice instead of collected, label lengths come from the literals' types.
#pragma once
#include "field.cuh"
#include "strobe.cuh"
#include "../../include/ark_plonk_amd.h"

// the C ABI's transcript handle: a sponge at rest (wire.hip creates and advances it; replay.hip hands a copy to its kernel)
struct zk_transcript {
    StrobeState st;
};

ZK_HD uint64_t le_u64(const uint8_t* p) {
    uint64_t v = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// ------------------------------------------------------------------------------------------ field elements and bytes
// little-endian bytes -> the integer they spell; false when it is >= p (ark-serialize refuses a non-canonical encoding)
template <class F, class P>
ZK_HD bool fp_canon_from_le(const uint8_t* in, size_t nbytes, F& c) {
    c = F::zero();
    bool high = false;
#pragma unroll
    for (size_t i = 0; i < 4 * (size_t)F::N; ++i)
        if (i < nbytes) c.v[i / 4] |= (uint32_t)in[i] << (8 * (i % 4));
    for (size_t i = 4 * (size_t)F::N; i < nbytes; ++i) high |= in[i] != 0;
    if (high) return false;
    bool below = false, decided = false;
#pragma unroll
    for (int i = F::N - 1; i >= 0; --i) {
        if (!decided && c.v[i] != P::MOD(i)) {
            below = c.v[i] < P::MOD(i);
            decided = true;
        }
    }
    return below;                                   // undecided: c == p
}
// the Montgomery product behind a call on the device (field.cuh's members are force-inlined; a proof has some forty conversions)
#if defined(__HIP_DEVICE_COMPILE__)
#define ZK_HD_CALLED __host__ __device__ __noinline__
#else
#define ZK_HD_CALLED __host__ __device__ inline
#endif
template <class F>
ZK_HD_CALLED F fp_mul_called(F a, F b) {
    return F::mul(a, b);
}
template <class F>
ZK_HD F fp_to_mont_called(const F& c) {
    return fp_mul_called(c, F::r2());
}
template <class F>
ZK_HD F fp_from_mont_called(const F& m) {
    F o = F::zero();
    o.v[0] = 1;
    return fp_mul_called(m, o);
}
// a row of the C ABI: 4 x uint64 limbs, the same bytes as the 8 words of Fp
template <class F>
ZK_HD F ld_row(const uint64_t* row) {
    F r;
#pragma unroll
    for (int i = 0; i < F::N / 2; ++i) {
        r.v[2 * i] = (uint32_t)row[i];
        r.v[2 * i + 1] = (uint32_t)(row[i] >> 32);
    }
    return r;
}
template <class F>
ZK_HD void st_row(uint64_t* row, const F& r) {
#pragma unroll
    for (int i = 0; i < F::N / 2; ++i) row[i] = (uint64_t)r.v[2 * i] | (uint64_t)r.v[2 * i + 1] << 32;
}
// the words of c shifted down one byte, `top` coming in at the high end
template <class F>
ZK_HD F words_shift_byte(F c, uint32_t top) {
#pragma unroll
    for (int k = 0; k < F::N; ++k) c.v[k] = (c.v[k] >> 8) | ((k + 1 < F::N ? c.v[k + 1] : top) << 24);
    return c;
}
// The n low bytes of the integer c, least significant first, into the running operation.  The device shifts them out of the words one
// by one -- c.v[i / 4] would index the registers at run time and send them to scratch memory; the host indexes.
template <class S, class F>
ZK_HD S strobe_absorb_words(S s, F c, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
        s = strobe_absorb_byte(s, c.v[0] & 0xffu);
        c = words_shift_byte(c, 0);
#else
        s = strobe_absorb_byte(s, (c.v[i / 4] >> (8 * (i % 4))) & 0xffu);
#endif
    }
    return s;
}
template <class S, class F>
struct Squeezed {
    S s;
    F v;
};
// n bytes out of the running operation, read as a little-endian integer (n <= 4 F::N)
template <class S, class F>
ZK_HD Squeezed<S, F> strobe_squeeze_words(S s, uint32_t n) {
    F c = F::zero();
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t b;
        s = strobe_squeeze_byte(s, b);
#if defined(__HIP_DEVICE_COMPILE__)
        c = words_shift_byte(c, b);                 // bytes come in at the high end and travel down ...
#else
        c.v[i / 4] |= b << (8 * (i % 4));
#endif
    }
#if defined(__HIP_DEVICE_COMPILE__)
    for (uint32_t i = n; i < 4 * (uint32_t)F::N; ++i) c = words_shift_byte(c, 0);      // ... the rest of the way
#endif
    return Squeezed<S, F>{s, c};
}

// ------------------------------------------------------------------------------------------ the reference's TranscriptProtocol
// Sizes of ark-serialize 0.3: Fr as ceil(bits / 8) bytes, a compressed G1 as x with the two SWFlags bits in its last byte
template <class Cv>
struct WireSizes {
    static constexpr size_t FQ_BYTES = (Cv::FqP::BITS + 2 + 7) / 8;
    static constexpr size_t FR_BYTES = (Cv::FrP::BITS + 7) / 8;
    static constexpr size_t CHALLENGE_BYTES = Cv::FrP::BITS / 8;      // transcript.rs:35-46: size_in_bits / 8, always below the modulus
};

struct Label {
    const uint8_t* p;
    size_t n;
};
template <size_t N>
ZK_HD Label label_of(const char (&s)[N]) {
    return Label{(const uint8_t*)s, N - 1};
}

// challenge_scalar: CHALLENGE_BYTES bytes as a little-endian integer (ark-ff `from_random_bytes`); v is that integer, not yet Montgomery
template <class Cv, class S>
ZK_HD Squeezed<S, typename Cv::Fr> transcript_challenge_canon(S s, Label label) {
    constexpr uint32_t SZ = (uint32_t)WireSizes<Cv>::CHALLENGE_BYTES;
    return strobe_squeeze_words<S, typename Cv::Fr>(transcript_challenge_begin(s, label.p, label.n, SZ), SZ);
}
// append(label, Fr): the canonical integer's FR_BYTES bytes
template <class Cv, class S>
ZK_HD S transcript_append_fr_canon(S s, Label label, const typename Cv::Fr& canon) {
    constexpr uint32_t F = (uint32_t)WireSizes<Cv>::FR_BYTES;
    return strobe_absorb_words(transcript_append_begin(s, label.p, label.n, F), canon, F);
}
// append(label, G1Affine) from an encoding: ark appends the re-serialised point -- for a decodable encoding that is its own bytes,
// except that infinity is written with x = 0 whatever the bytes held
template <class Cv, class S>
ZK_HD S transcript_append_g1_encoding(S s, Label label, const uint8_t* enc) {
    constexpr size_t G = WireSizes<Cv>::FQ_BYTES;
    s = transcript_append_begin(s, label.p, label.n, G);
    if ((enc[G - 1] & 0xC0) == 0x40) return strobe_absorb_byte(strobe_absorb_zeros(s, G - 1), 0x40);
    return strobe_absorb(s, enc, G);
}

// `PublicInputs { values: BTreeMap<usize, F> }` (pi.rs:28-36) under `label` (prover.rs:182 uses b"pi"): u64 count, then
// (u64 position, Fr) in ascending position order.  `PublicInputs::insert` (pi.rs:56-65) drops zero values ("zeros are the implicit
// value of empty positions"), so the reference's map never holds one -- neither on the prover's nor on the verifier's side: a zero
// entry handed in here is skipped the same way, it is not part of the message.  false (and s as it came): positions not strictly
// ascending -- a BTreeMap iterates in strictly ascending key order.
template <class Cv, class S>
ZK_HD bool transcript_append_public_inputs(S& s, Label label, const uint64_t* positions, const uint64_t* values_mont, size_t n) {
    typedef typename Cv::Fr Fr;
    constexpr size_t F = WireSizes<Cv>::FR_BYTES;
    uint64_t kept = 0;
    for (size_t i = 0; i < n; ++i) {
        if (i && positions[i] <= positions[i - 1]) return false;
        kept += (values_mont[4 * i] | values_mont[4 * i + 1] | values_mont[4 * i + 2] | values_mont[4 * i + 3]) ? 1 : 0;
    }
    S t = transcript_append_begin(s, label.p, label.n, (size_t)(8 + kept * (8 + F)));
    t = strobe_absorb_le(t, kept, 8);
    for (size_t i = 0; i < n; ++i) {
        const Fr m = ld_row<Fr>(values_mont + 4 * i);
        if (m.is_zero()) continue;
        t = strobe_absorb_le(t, positions[i], 8);
        t = strobe_absorb_words(t, fp_from_mont_called(m), (uint32_t)F);
    }
    s = t;
    return true;
}

// ------------------------------------------------------------------------------------------ the verifier's parse and replay
// the seven custom evaluations the verifier reads by label (proof.rs:488-611), in the order of the evaluation row
ZK_HD Label verify_custom_label(int j) {
    switch (j) {
        case 0: return label_of("a_next_eval");
        case 1: return label_of("b_next_eval");
        case 2: return label_of("d_next_eval");
        case 3: return label_of("q_arith_eval");
        case 4: return label_of("q_c_eval");
        case 5: return label_of("q_l_eval");
        default: return label_of("q_r_eval");
    }
}
ZK_HD bool label_equals(const uint8_t* p, uint64_t n, Label l) {
    if (n != l.n) return false;
    bool same = true;
    for (size_t i = 0; i < l.n; ++i) same &= p[i] == l.p[i];
    return same;
}
// where point i of a proof stands: 13 commitments, then two openings followed by an Option byte each
template <class Cv>
ZK_HD size_t proof_point_offset(int i) {
    return (size_t)i * WireSizes<Cv>::FQ_BYTES + (i > 13 ? 1 : 0);
}

// what the parse of a well-formed proof leaves for the replay: where its evaluations and custom evaluations stand, how many of the latter
struct ProofLayout {
    size_t evals_at, custom_at;
    uint64_t n_custom;
};

// One proof, first half: walk proof.rs:41-103.  Fills the evaluation row (the proof's 16, then the seven found by label) and
// points_out (optional): the 13 commitments and the two openings, FQ_BYTES each, as they stand in the proof.  Never reads outside
// data[0, len); writes the row as it goes, so a caller zeroes it when the status is not ZK_PROOF_OK.
template <class Cv>
ZK_HD uint8_t replay_parse(const uint8_t* data, size_t len, uint64_t* ev_out, uint8_t* points_out, ProofLayout& lay) {
    typedef typename Cv::Fr Fr;
    typedef typename Cv::FrP FrP;
    constexpr size_t G = WireSizes<Cv>::FQ_BYTES, F = WireSizes<Cv>::FR_BYTES;
    size_t pos = 0;
    for (int i = 0; i < 15; ++i) {
        if (len - pos < G) return ZK_PROOF_TRUNCATED;
        pos += G;
        if (i >= 13) {                                       // kzg10::Proof { w, random_v }: random_v is None in every proof of this scheme
            if (len - pos < 1) return ZK_PROOF_TRUNCATED;
            if (data[pos] != 0) return ZK_PROOF_BAD_OPTION;
            pos += 1;
        }
    }
    if (points_out) {
        for (int i = 0; i < 15; ++i) {
            const uint8_t* src = data + proof_point_offset<Cv>(i);
            for (size_t b = 0; b < G; ++b) points_out[(size_t)i * G + b] = src[b];
        }
    }
    lay.evals_at = pos;
    for (int i = 0; i < ZK_PROOF_N_EVALS; ++i) {
        if (len - pos < F) return ZK_PROOF_TRUNCATED;
        Fr c;
        if (!fp_canon_from_le<Fr, FrP>(data + pos, F, c)) return ZK_PROOF_FR_NOT_REDUCED;
        st_row(ev_out + 4 * i, fp_to_mont_called(c));
        pos += F;
    }
    if (len - pos < 8) return ZK_PROOF_TRUNCATED;
    const uint64_t k = le_u64(data + pos);
    pos += 8;
    if (k > (len - pos) / (8 + F)) return ZK_PROOF_BAD_COUNT;       // more entries than bytes: also bounds the loops below
    // first pass over the custom evaluations: bounds, ranges, and the seven the verifier reads -- a repeated label: the last one counts
    lay.custom_at = pos;
    lay.n_custom = k;
    uint32_t found = 0;
    for (uint64_t i = 0; i < k; ++i) {
        if (pos == len) return ZK_PROOF_BAD_COUNT;                  // the bytes end on an entry boundary with entries still announced
        if (len - pos < 8) return ZK_PROOF_TRUNCATED;
        const uint64_t ll = le_u64(data + pos);
        pos += 8;
        if (ll > len - pos || len - pos - ll < F) return ZK_PROOF_TRUNCATED;
        const uint8_t* label = data + pos;
        pos += (size_t)ll;
        Fr c;
        if (!fp_canon_from_le<Fr, FrP>(data + pos, F, c)) return ZK_PROOF_FR_NOT_REDUCED;
        pos += F;
        int hit = -1;
#pragma unroll
        for (int j = 0; j < 7; ++j)
            if (label_equals(label, ll, verify_custom_label(j))) hit = j;
        if (hit >= 0) {
            st_row(ev_out + 4 * (ZK_PROOF_N_EVALS + hit), fp_to_mont_called(c));
            found |= 1u << hit;
        }
    }
    if (pos != len) return ZK_PROOF_TRAILING;
    if (found != 0x7fu) return ZK_PROOF_MISSING_LABEL;
    return ZK_PROOF_OK;
}

// One proof, second half: replay proof.rs:128-300, 343-378 over a proof replay_parse accepted, on the sponge s (a copy of the seeded
// transcript's), the public-input message first.  Fills the challenge row.
template <class Cv, class S>
ZK_HD uint8_t replay_script(S s, const uint8_t* data, const ProofLayout& lay, const uint64_t* pi_pos, const uint64_t* pi_val, size_t n_pi,
                            uint64_t* ch_out) {
    typedef typename Cv::Fr Fr;
    constexpr size_t F = WireSizes<Cv>::FR_BYTES;
    if (!transcript_append_public_inputs<Cv>(s, label_of("pi"), pi_pos, pi_val, n_pi)) return ZK_PROOF_BAD_PUBLIC_INPUTS;
    // indices of put_g1: a b c d z f h_1 h_2 z_2 t_1 t_2 t_3 t_4, the proof's order
    auto put_g1 = [&](Label label, int i) __attribute__((always_inline)) {
        s = transcript_append_g1_encoding<Cv>(s, label, data + proof_point_offset<Cv>(i));
    };
    // an evaluation that passed the range check is appended as it stands in the proof: the canonical encoding is unique
    auto put_bytes = [&](Label label, const uint8_t* fr_bytes) __attribute__((always_inline)) {
        s = transcript_append(s, label.p, label.n, fr_bytes, F);
    };
    int slot = 0;
    // a challenge, and (put.p != nullptr) the same scalar appended under the label `put`
    auto draw = [&](Label label, Label put) __attribute__((always_inline)) {
        const Squeezed<S, Fr> q = transcript_challenge_canon<Cv>(s, label);
        s = q.s;
        st_row(ch_out + 4 * slot++, fp_to_mont_called(q.v));
        if (put.p) s = transcript_append_fr_canon<Cv>(s, put, q.v);
    };
    const Label none = {nullptr, 0};
    put_g1(label_of("w_l"), 0), put_g1(label_of("w_r"), 1), put_g1(label_of("w_o"), 2), put_g1(label_of("w_4"), 3);
    draw(label_of("zeta"), label_of("zeta"));
    put_g1(label_of("f"), 5), put_g1(label_of("h1"), 6), put_g1(label_of("h2"), 7);
    draw(label_of("beta"), label_of("beta")), draw(label_of("gamma"), label_of("gamma"));
    draw(label_of("delta"), label_of("delta")), draw(label_of("epsilon"), label_of("epsilon"));
    put_g1(label_of("z"), 4);
    draw(label_of("alpha"), label_of("alpha"));
    draw(label_of("range separation challenge"), label_of("range seperation challenge"));
    draw(label_of("logic separation challenge"), label_of("logic seperation challenge"));
    draw(label_of("fixed base separation challenge"), label_of("fixed base separation challenge"));
    draw(label_of("variable base separation challenge"), label_of("variable base separation challenge"));
    draw(label_of("lookup separation challenge"), label_of("lookup separation challenge"));
    put_g1(label_of("t_1"), 9), put_g1(label_of("t_2"), 10), put_g1(label_of("t_3"), 11), put_g1(label_of("t_4"), 12);
    draw(label_of("z"), label_of("z"));
    // the 14 evaluations proof.rs:253-300 appends, by their index in the proof's evaluation block
    for (int e = 0; e < 14; ++e) {
        Label l;
        int idx;
        switch (e) {
            case 0: l = label_of("a_eval"), idx = 0; break;
            case 1: l = label_of("b_eval"), idx = 1; break;
            case 2: l = label_of("c_eval"), idx = 2; break;
            case 3: l = label_of("d_eval"), idx = 3; break;
            case 4: l = label_of("left_sig_eval"), idx = 4; break;
            case 5: l = label_of("right_sig_eval"), idx = 5; break;
            case 6: l = label_of("out_sig_eval"), idx = 6; break;
            case 7: l = label_of("perm_eval"), idx = 7; break;
            case 8: l = label_of("f_eval"), idx = 13; break;
            case 9: l = label_of("q_lookup_eval"), idx = 8; break;
            case 10: l = label_of("lookup_perm_eval"), idx = 9; break;
            case 11: l = label_of("h_1_eval"), idx = 10; break;
            case 12: l = label_of("h_1_next_eval"), idx = 11; break;
            default: l = label_of("h_2_eval"), idx = 12; break;
        }
        put_bytes(l, data + lay.evals_at + (size_t)idx * F);
    }
    // second pass over the custom evaluations, every one of them, in the proof's order (the first pass vetted the lengths)
    size_t pos = lay.custom_at;
    for (uint64_t i = 0; i < lay.n_custom; ++i) {
        const size_t ll = (size_t)le_u64(data + pos);
        s = transcript_append(s, data + pos + 8, ll, data + pos + 8 + ll, F);
        pos += 8 + ll + F;
    }
    draw(label_of("aggregate_witness"), none);
    draw(label_of("aggregate_witness"), none);
    return ZK_PROOF_OK;
}

// both halves: the host's replay of one proof
template <class Cv, class S>
ZK_HD uint8_t replay_walk(S s, const uint8_t* data, size_t len, const uint64_t* pi_pos, const uint64_t* pi_val, size_t n_pi, uint64_t* ch_out,
                          uint64_t* ev_out, uint8_t* points_out) {
    ProofLayout lay;
    const uint8_t st = replay_parse<Cv>(data, len, ev_out, points_out, lay);
    return st != ZK_PROOF_OK ? st : replay_script<Cv>(s, data, lay, pi_pos, pi_val, n_pi, ch_out);
}
