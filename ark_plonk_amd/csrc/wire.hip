// N4: canonical wire formats and the transcript, host side only (no device code).
//
//  * ark-serialize 0.3 encodings the reference uses wherever it serialises (transcript.rs:27-33 `append`, the derive on
//    proof.rs:41-103 `Proof`, widget/mod.rs:252-278 verifier key):
//      Fp           little-endian canonical integer, ceil((MODULUS_BITS + flag bits) / 8) bytes
//                   (Fr: 32 B; Fq as the x of a compressed point: 48 B BLS12-381 / 32 B BN254)
//      G1Affine     compressed = x with SWFlags in the two top bits of the LAST byte: bit 7 = "y is the larger of
//                   (y, -y)" (PositiveY), bit 6 = infinity (x written as 0); uncompressed = x, then y carrying the
//                   infinity flag
//  * merlin 3.0 `Transcript` (STROBE-128 over Keccak-f[1600], operations meta-AD / AD / PRF only) and the reference's
//    TranscriptProtocol on top of it (transcript.rs:27-49): append = serialize + append_message, challenge_scalar =
//    size_in_bits/8 = 31 challenge bytes read as a little-endian integer (ark-ff `from_random_bytes`),
//    circuit_domain_sep = ("dom-sep","circuit_size") + append_u64("n").
// The sponge (Keccak-f[1600], STROBE-128, append / challenge) is strobe.cuh and the verifier's parse and replay of a proof
// replay_walk.cuh: one definition each, which replay.hip runs on the device.  This file holds the transcript handle, the encodings,
// and the entry points.
// merlin, ark-serialize and ark-ff are crates.io dependencies absent from /root/reference (plonk-core/Cargo.toml:51-65):
// this file restates their published behaviour; tests pin it on merlin's published conformance vector.
#include "g1_host.h"
#include "replay_walk.cuh"

namespace {

// ------------------------------------------------------------------------------------------ field / curve helpers
template <class F>
void fp_to_le_bytes(const F& mont, uint8_t* out, size_t nbytes) {
    F c = F::from_mont(mont);
    for (size_t i = 0; i < nbytes; ++i) out[i] = i / 4 < (size_t)F::N ? (uint8_t)(c.v[i / 4] >> (8 * (i % 4))) : 0;
}
// canonical little-endian bytes -> Montgomery; false when the integer is >= p
template <class F, class P>
bool fp_from_le_bytes(const uint8_t* in, size_t nbytes, F& out) {
    F c;
    if (!fp_canon_from_le<F, P>(in, nbytes, c)) return false;
    out = F::to_mont(c);
    return true;
}
// a > b as canonical integers (ark's Ord on Fp compares into_repr())
template <class F>
bool fp_gt(const F& a_mont, const F& b_mont) {
    F a = F::from_mont(a_mont), b = F::from_mont(b_mont);
    for (int i = F::N - 1; i >= 0; --i) {
        if (a.v[i] != b.v[i]) return a.v[i] > b.v[i];
    }
    return false;
}

template <class Cv>
struct Wire {
    typedef typename Cv::Fq Fq;
    typedef typename Cv::Fr Fr;
    typedef typename Cv::FqP FqP;
    typedef typename Cv::FrP FrP;
    typedef G1Host<Fq> H;
    static constexpr size_t FQ_BYTES = WireSizes<Cv>::FQ_BYTES;   // serialize_with_flags::<SWFlags>: 2 flag bits
    static constexpr size_t FR_BYTES = WireSizes<Cv>::FR_BYTES;

    static int fr_ser(const uint64_t* mont, uint8_t* out) {
        Fr x;
        memcpy(x.v, mont, 32);
        fp_to_le_bytes<Fr>(x, out, FR_BYTES);
        return ZK_OK;
    }
    static int fr_de(const uint8_t* in, uint64_t* mont) {
        Fr x;
        if (!fp_from_le_bytes<Fr, FrP>(in, FR_BYTES, x)) return ZK_ERR_BAD_ARG;
        memcpy(mont, x.v, 32);
        return ZK_OK;
    }
    static int g1_ser_c(const uint64_t* xy, uint8_t inf, uint8_t* out) {
        const typename H::A a = H::ld_affine(xy);
        if (H::affine_is_inf(a, inf)) {
            memset(out, 0, FQ_BYTES);
            out[FQ_BYTES - 1] |= 1u << 6;
            return ZK_OK;
        }
        fp_to_le_bytes<Fq>(a.x, out, FQ_BYTES);
        if (fp_gt<Fq>(a.y, Fq::neg(a.y))) out[FQ_BYTES - 1] |= 1u << 7;
        return ZK_OK;
    }
    static int g1_ser_u(const uint64_t* xy, uint8_t inf, uint8_t* out) {
        const typename H::A a = H::ld_affine(xy);
        if (H::affine_is_inf(a, inf)) {
            memset(out, 0, 2 * FQ_BYTES);
            out[2 * FQ_BYTES - 1] |= 1u << 6;
            return ZK_OK;
        }
        fp_to_le_bytes<Fq>(a.x, out, FQ_BYTES);
        fp_to_le_bytes<Fq>(a.y, out + FQ_BYTES, FQ_BYTES);
        return ZK_OK;
    }
    static Fq curve_rhs(const Fq& x) { return Fq::add(Fq::mul(Fq::sqr(x), x), Fq::from_u32(FqP::COEFF_B)); }
    // r * P == O ?  (ark's is_in_correct_subgroup_assuming_on_curve)
    static bool in_subgroup(const Fq& x, const Fq& y) {
        uint32_t r[Fr::N];
        for (int i = 0; i < Fr::N; ++i) r[i] = FrP::MOD(i);
        return H::scalar_mul(typename H::A{x, y}, r, Fr::N).is_inf();
    }
    static int g1_de_c(const uint8_t* in, uint64_t* xy, uint8_t* inf) {
        uint8_t buf[FQ_BYTES];
        memcpy(buf, in, FQ_BYTES);
        const uint8_t flags = buf[FQ_BYTES - 1] & 0xC0;
        buf[FQ_BYTES - 1] &= 0x3F;
        if (flags == 0xC0) return ZK_ERR_BAD_ARG;           // SWFlags::from_u8: both bits set is invalid
        Fq x;
        if (!fp_from_le_bytes<Fq, FqP>(buf, FQ_BYTES, x)) return ZK_ERR_BAD_ARG;
        if (flags & 0x40) {                                  // infinity: GroupAffine::zero() = (0, 1)
            H::st_affine_inf(xy, inf);
            return ZK_OK;
        }
        // both base fields are 3 mod 4: sqrt(a) = a^((p+1)/4)
        uint32_t e[Fq::N + 1];
        uint64_t carry = 1;
        for (int i = 0; i < Fq::N; ++i) {
            uint64_t t = (uint64_t)FqP::MOD(i) + carry;
            e[i] = (uint32_t)t;
            carry = t >> 32;
        }
        e[Fq::N] = (uint32_t)carry;
        for (int i = 0; i < Fq::N; ++i) e[i] = (e[i] >> 2) | (e[i + 1] << 30);
        const Fq rhs = curve_rhs(x);
        Fq y = Fq::pow_limbs(rhs, e, Fq::N);
        if (Fq::sqr(y) != rhs) return ZK_ERR_BAD_ARG;        // x is not on the curve
        const Fq ny = Fq::neg(y);
        const bool want_greatest = (flags & 0x80) != 0;
        if (fp_gt<Fq>(y, ny) != want_greatest) y = ny;
        if (!in_subgroup(x, y)) return ZK_ERR_BAD_ARG;
        H::st_affine(xy, inf, typename H::A{x, y});
        return ZK_OK;
    }
    static int g1_de_u(const uint8_t* in, uint64_t* xy, uint8_t* inf) {
        uint8_t buf[FQ_BYTES];
        memcpy(buf, in + FQ_BYTES, FQ_BYTES);
        const uint8_t flags = buf[FQ_BYTES - 1] & 0xC0;
        if (flags == 0xC0) return ZK_ERR_BAD_ARG;           // SWFlags::from_u8: both bits set is invalid (as g1_de_c)
        buf[FQ_BYTES - 1] &= 0x3F;
        Fq x, y;
        if (!fp_from_le_bytes<Fq, FqP>(in, FQ_BYTES, x) || !fp_from_le_bytes<Fq, FqP>(buf, FQ_BYTES, y)) return ZK_ERR_BAD_ARG;
        if (flags & 0x40) {
            H::st_affine_inf(xy, inf);
            return ZK_OK;
        }
        if (Fq::sqr(y) != curve_rhs(x) || !in_subgroup(x, y)) return ZK_ERR_BAD_ARG;
        H::st_affine(xy, inf, typename H::A{x, y});
        return ZK_OK;
    }
    // transcript.rs:35-46: size = size_in_bits / 8 challenge bytes -> F::from_random_bytes
    static int challenge(StrobeState& st, const uint8_t* label, size_t len, uint64_t* out_mont) {
        HostSponge s(st);
        const Squeezed<HostSponge, Fr> q = transcript_challenge_canon<Cv>(s, Label{label, len});
        q.s.save(st);
        st_row(out_mont, Fr::to_mont(q.v));       // 31 bytes for both curves: always below the modulus
        return ZK_OK;
    }
};

// the sponge of strobe.cuh over a transcript at rest
void host_append(StrobeState& st, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
    transcript_append(HostSponge(st), label, label_len, msg, msg_len).save(st);
}
void host_challenge(StrobeState& st, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
    transcript_challenge(HostSponge(st), label, label_len, out, out_len).save(st);
}
// merlin's Transcript::new(label)
void transcript_init(StrobeState& st, const uint8_t* label, size_t label_len) {
    memset(&st, 0, sizeof st);
    strobe_init(HostSponge(st), (const uint8_t*)"Merlin v1.0", 11).save(st);
    host_append(st, (const uint8_t*)"dom-sep", 7, label, label_len);
}

}  // namespace

// `call` on the curve's Wire<Cv>, written with W for that type
#define WIRE_DISPATCH(curve_id, call)                                    \
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {          \
        typedef Wire<decltype(cv)> W;                                    \
        return call;                                                     \
    })

extern "C" {

size_t zk_fr_serialized_size(int curve_id) {
    return zk_on_curve(curve_id, (size_t)0, [](auto cv) { return (size_t)Wire<decltype(cv)>::FR_BYTES; });
}
size_t zk_g1_compressed_size(int curve_id) {
    return zk_on_curve(curve_id, (size_t)0, [](auto cv) { return (size_t)Wire<decltype(cv)>::FQ_BYTES; });
}
int zk_fr_serialize(int curve_id, const uint64_t* fr_mont, uint8_t* out) {
    if (!fr_mont || !out) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::fr_ser(fr_mont, out));
}
int zk_fr_deserialize(int curve_id, const uint8_t* in, uint64_t* fr_mont) {
    if (!fr_mont || !in) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::fr_de(in, fr_mont));
}
int zk_g1_serialize_compressed(int curve_id, const uint64_t* xy_mont, uint8_t inf, uint8_t* out) {
    if (!xy_mont || !out) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::g1_ser_c(xy_mont, inf, out));
}
int zk_g1_deserialize_compressed(int curve_id, const uint8_t* in, uint64_t* xy_mont, uint8_t* inf) {
    if (!xy_mont || !in) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::g1_de_c(in, xy_mont, inf));
}
int zk_g1_serialize_uncompressed(int curve_id, const uint64_t* xy_mont, uint8_t inf, uint8_t* out) {
    if (!xy_mont || !out) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::g1_ser_u(xy_mont, inf, out));
}
int zk_g1_deserialize_uncompressed(int curve_id, const uint8_t* in, uint64_t* xy_mont, uint8_t* inf) {
    if (!xy_mont || !in) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::g1_de_u(in, xy_mont, inf));
}

zk_transcript* zk_transcript_new(const uint8_t* label, size_t label_len) {
    if (!label && label_len) return nullptr;
    zk_transcript* t = new zk_transcript;
    transcript_init(t->st, label, label_len);
    return t;
}
zk_transcript* zk_transcript_clone(const zk_transcript* t) { return t ? new zk_transcript(*t) : nullptr; }
void zk_transcript_free(zk_transcript* t) { delete t; }
int zk_transcript_append_message(zk_transcript* t, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
    if (!t || (!label && label_len) || (!msg && msg_len)) return ZK_ERR_BAD_ARG;
    host_append(t->st, label, label_len, msg, msg_len);
    return ZK_OK;
}
int zk_transcript_append_u64(zk_transcript* t, const uint8_t* label, size_t label_len, uint64_t v) {
    uint8_t le[8];
    for (int i = 0; i < 8; ++i) le[i] = (uint8_t)(v >> (8 * i));
    return zk_transcript_append_message(t, label, label_len, le, 8);
}
int zk_transcript_challenge_bytes(zk_transcript* t, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
    if (!t || (!label && label_len) || (!out && out_len)) return ZK_ERR_BAD_ARG;
    host_challenge(t->st, label, label_len, out, out_len);
    return ZK_OK;
}
int zk_transcript_append_fr(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* fr_mont) {
    uint8_t buf[32];
    int rc = zk_fr_serialize(curve_id, fr_mont, buf);
    if (rc) return rc;
    return zk_transcript_append_message(t, label, label_len, buf, zk_fr_serialized_size(curve_id));
}
int zk_transcript_append_g1(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* xy_mont, uint8_t inf) {
    uint8_t buf[48];
    int rc = zk_g1_serialize_compressed(curve_id, xy_mont, inf, buf);
    if (rc) return rc;
    return zk_transcript_append_message(t, label, label_len, buf, zk_g1_compressed_size(curve_id));
}
int zk_transcript_challenge_scalar(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, uint64_t* fr_mont) {
    if (!t || !fr_mont || (!label && label_len)) return ZK_ERR_BAD_ARG;
    WIRE_DISPATCH(curve_id, W::challenge(t->st, label, label_len, fr_mont));
}
// `PublicInputs` under `label`: the message is replay_walk.cuh's (zero values skipped, ascending positions or ZK_ERR_BAD_ARG)
int zk_transcript_append_public_inputs(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* positions,
                                       const uint64_t* values_mont, size_t n) {
    if (!t || (n && (!positions || !values_mont))) return ZK_ERR_BAD_ARG;
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) {
        HostSponge sp(t->st);
        if (!transcript_append_public_inputs<decltype(cv)>(sp, Label{label, label_len}, positions, values_mont, n)) return ZK_ERR_BAD_ARG;
        sp.save(t->st);
        return ZK_OK;
    });
}

int zk_transcript_circuit_domain_sep(zk_transcript* t, uint64_t n) {
    int rc = zk_transcript_append_message(t, (const uint8_t*)"dom-sep", 7, (const uint8_t*)"circuit_size", 12);
    if (rc) return rc;
    return zk_transcript_append_u64(t, (const uint8_t*)"n", 1, n);
}

// proof.rs:41-103 + proof.rs ProofEvaluations: the derive serialises the fields in declaration order, every commitment
// and opening proof as a compressed G1 (kzg10::Commitment(G1Affine); kzg10::Proof { w: G1Affine, random_v: Option<Fr> }
// with random_v = None -> one 0 byte), every evaluation as an Fr
size_t zk_proof_serialized_size(int curve_id, uint32_t n_custom_evals, const uint32_t* label_lens) {
    const size_t g = zk_g1_compressed_size(curve_id), f = zk_fr_serialized_size(curve_id);
    if (!g) return 0;
    size_t sz = 13 * g + 2 * (g + 1) + (ZK_PROOF_N_EVALS)*f + 8;   // 13 commitments, 2 openings, fixed evaluations, Vec length
    for (uint32_t i = 0; i < n_custom_evals; ++i) sz += 8 + (label_lens ? label_lens[i] : 0) + f;   // (String, F): u64 length + bytes + Fr
    return sz;
}

int zk_proof_serialize(int curve_id, const zk_proof* p, uint8_t* out, size_t cap, size_t* written) {
    if (!p || !out) return ZK_ERR_BAD_ARG;
    if (!p->commitments || !p->commitment_inf || !p->openings || !p->opening_inf || !p->evals) return ZK_ERR_BAD_ARG;
    if (p->n_custom_evals && (!p->custom_labels || !p->custom_evals)) return ZK_ERR_BAD_ARG;
    const size_t g = zk_g1_compressed_size(curve_id), f = zk_fr_serialized_size(curve_id);
    if (!g) return ZK_ERR_BAD_ARG;
    std::vector<uint32_t> ll(p->n_custom_evals);
    for (uint32_t i = 0; i < p->n_custom_evals; ++i) {
        if (!p->custom_labels[i]) return ZK_ERR_BAD_ARG;
        ll[i] = (uint32_t)strlen(p->custom_labels[i]);
    }
    const size_t need = zk_proof_serialized_size(curve_id, p->n_custom_evals, ll.data());
    if (cap < need) return ZK_ERR_BAD_ARG;
    const int L = zk_on_curve(curve_id, 4, [](auto cv) { return (int)decltype(cv)::Fq::N / 2; });   // an unknown id was refused above
    uint8_t* w = out;
    int rc;
    for (int i = 0; i < 13; ++i) {
        if ((rc = zk_g1_serialize_compressed(curve_id, p->commitments + (size_t)i * 2 * L, p->commitment_inf[i], w))) return rc;
        w += g;
    }
    for (int i = 0; i < 2; ++i) {
        if ((rc = zk_g1_serialize_compressed(curve_id, p->openings + (size_t)i * 2 * L, p->opening_inf[i], w))) return rc;
        w += g;
        *w++ = 0;     // Option<Fr>::None
    }
    for (int i = 0; i < ZK_PROOF_N_EVALS; ++i) {
        if ((rc = zk_fr_serialize(curve_id, p->evals + (size_t)i * 4, w))) return rc;
        w += f;
    }
    const uint64_t nc = p->n_custom_evals;
    for (int b = 0; b < 8; ++b) *w++ = (uint8_t)(nc >> (8 * b));
    for (uint32_t i = 0; i < p->n_custom_evals; ++i) {
        const uint64_t sl = ll[i];
        for (int b = 0; b < 8; ++b) *w++ = (uint8_t)(sl >> (8 * b));
        memcpy(w, p->custom_labels[i], sl);
        w += sl;
        if ((rc = zk_fr_serialize(curve_id, p->custom_evals + (size_t)i * 4, w))) return rc;
        w += f;
    }
    if (written) *written = (size_t)(w - out);
    return ZK_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ the verifier's parse and replay
extern "C" int zk_proof_replay_batch(const zk_transcript* seeded, int curve_id, size_t n_proofs, const uint8_t* const* proofs, const size_t* proof_lens,
                                     const uint64_t* pi_offsets, const uint64_t* pi_positions, const uint64_t* pi_values_mont,
                                     uint64_t* out_challenges_mont, uint64_t* out_evals_mont, uint8_t* out_points, uint8_t* out_status) {
    if (!seeded || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (n_proofs && (!proofs || !proof_lens || !pi_offsets || !out_challenges_mont || !out_evals_mont || !out_status)) return ZK_ERR_BAD_ARG;
    for (size_t j = 0; j < n_proofs; ++j) {
        if (!proofs[j] && proof_lens[j]) return ZK_ERR_BAD_ARG;
        if (pi_offsets[j + 1] < pi_offsets[j]) return ZK_ERR_BAD_ARG;
    }
    if (n_proofs && pi_offsets[n_proofs] && (!pi_positions || !pi_values_mont)) return ZK_ERR_BAD_ARG;
    const size_t g = zk_g1_compressed_size(curve_id);
    for (size_t j = 0; j < n_proofs; ++j) {
        uint64_t* ch = out_challenges_mont + j * 4 * ZK_VERIFY_N_CHALLENGES;
        uint64_t* ev = out_evals_mont + j * 4 * ZK_VERIFY_N_EVALS;
        uint8_t* pt = out_points ? out_points + j * 15 * g : nullptr;
        const uint64_t o = pi_offsets[j];
        const size_t n_pi = (size_t)(pi_offsets[j + 1] - o);
        out_status[j] = zk_on_curve(curve_id, (uint8_t)ZK_PROOF_TRUNCATED, [&](auto cv) {
            StrobeState st = seeded->st;                     // the replay runs on a copy: `seeded` serves every proof
            return replay_walk<decltype(cv)>(HostSponge(st), proofs[j], proof_lens[j], n_pi ? pi_positions + o : nullptr,
                                             n_pi ? pi_values_mont + 4 * o : nullptr, n_pi, ch, ev, pt);
        });
        if (out_status[j] != ZK_PROOF_OK) {                 // a rejected proof leaves no half-written rows behind
            memset(ch, 0, 32 * ZK_VERIFY_N_CHALLENGES);
            memset(ev, 0, 32 * ZK_VERIFY_N_EVALS);
            if (pt) {                                        // ... and its points decode as infinity: stage 1 has nothing to report for them
                memset(pt, 0, 15 * g);
                for (int i = 0; i < 15; ++i) pt[i * g + g - 1] = 0x40;
            }
        }
    }
    return ZK_OK;
}
