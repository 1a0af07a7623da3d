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
// merlin, ark-serialize and ark-ff are crates.io dependencies absent from /root/reference (plonk-core/Cargo.toml:51-65):
// this file restates their published behaviour; tests pin it on merlin's published conformance vector.
#include "g1_host.h"

namespace {

// ------------------------------------------------------------------------------------------ Keccak-f[1600]
inline uint64_t rol(uint64_t x, int s) { return s ? (x << s) | (x >> (64 - s)) : x; }

void keccak_f1600(uint64_t st[25]) {
    static const uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                                    0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                    0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static const int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    for (int round = 0; round < 24; ++round) {
        uint64_t c[5], d[5], b[25];
        for (int x = 0; x < 5; ++x) c[x] = st[x] ^ st[x + 5] ^ st[x + 10] ^ st[x + 15] ^ st[x + 20];
        for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ rol(c[(x + 1) % 5], 1);
        for (int i = 0; i < 25; ++i) st[i] ^= d[i % 5];
        // rho + pi: lane (x, y) -> (y, 2x + 3y)
        for (int x = 0; x < 5; ++x)
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol(st[x + 5 * y], ROT[x + 5 * y]);
        for (int y = 0; y < 5; ++y)
            for (int x = 0; x < 5; ++x) st[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        st[0] ^= RC[round];
    }
}

// ------------------------------------------------------------------------------------------ STROBE-128 (merlin's subset)
struct Strobe128 {
    static constexpr uint8_t R = 166;
    static constexpr uint8_t FLAG_I = 1, FLAG_A = 2, FLAG_C = 4, FLAG_T = 8, FLAG_M = 16, FLAG_K = 32;
    uint8_t state[200];
    uint8_t pos = 0, pos_begin = 0, cur_flags = 0;

    void permute() {
        uint64_t w[25];
        for (int i = 0; i < 25; ++i) {
            w[i] = 0;
            for (int b = 0; b < 8; ++b) w[i] |= (uint64_t)state[8 * i + b] << (8 * b);
        }
        keccak_f1600(w);
        for (int i = 0; i < 25; ++i)
            for (int b = 0; b < 8; ++b) state[8 * i + b] = (uint8_t)(w[i] >> (8 * b));
    }
    explicit Strobe128(const uint8_t* label, size_t len) {
        memset(state, 0, sizeof state);
        const uint8_t head[6] = {1, (uint8_t)(R + 2), 1, 0, 1, 96};
        memcpy(state, head, 6);
        memcpy(state + 6, "STROBEv1.0.2", 12);
        permute();
        meta_ad(label, len, false);
    }
    void run_f() {
        state[pos] ^= pos_begin;
        state[pos + 1] ^= 0x04;
        state[R + 1] ^= 0x80;
        permute();
        pos = 0;
        pos_begin = 0;
    }
    void absorb(const uint8_t* d, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            state[pos] ^= d[i];
            if (++pos == R) run_f();
        }
    }
    void squeeze(uint8_t* d, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            d[i] = state[pos];
            state[pos] = 0;
            if (++pos == R) run_f();
        }
    }
    void begin_op(uint8_t flags, bool more) {
        if (more) return;      // continuation of the running operation (same flags by construction here)
        const uint8_t old_begin = pos_begin;
        pos_begin = (uint8_t)(pos + 1);
        cur_flags = flags;
        const uint8_t hdr[2] = {old_begin, flags};
        absorb(hdr, 2);
        if ((flags & (FLAG_C | FLAG_K)) && pos != 0) run_f();
    }
    void meta_ad(const uint8_t* d, size_t n, bool more) {
        begin_op(FLAG_M | FLAG_A, more);
        absorb(d, n);
    }
    void ad(const uint8_t* d, size_t n, bool more) {
        begin_op(FLAG_A, more);
        absorb(d, n);
    }
    void prf(uint8_t* d, size_t n, bool more) {
        begin_op(FLAG_I | FLAG_A | FLAG_C, more);
        squeeze(d, n);
    }
};

// ------------------------------------------------------------------------------------------ field / curve helpers
template <class F>
void fp_to_le_bytes(const F& mont, uint8_t* out, size_t nbytes) {
    F c = F::from_mont(mont);
    for (size_t i = 0; i < nbytes; ++i) out[i] = i / 4 < (size_t)F::N ? (uint8_t)(c.v[i / 4] >> (8 * (i % 4))) : 0;
}
// canonical little-endian bytes -> Montgomery; false when the integer is >= p
template <class F, class P>
bool fp_from_le_bytes(const uint8_t* in, size_t nbytes, F& out) {
    F c = F::zero();
    for (size_t i = 0; i < nbytes; ++i) {
        if (i / 4 >= (size_t)F::N) {
            if (in[i]) return false;
            continue;
        }
        c.v[i / 4] |= (uint32_t)in[i] << (8 * (i % 4));
    }
    for (int i = F::N - 1; i >= 0; --i) {      // c < p ?
        if (c.v[i] < P::MOD(i)) break;
        if (c.v[i] > P::MOD(i)) return false;
        if (i == 0) return false;               // c == p
    }
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
    static constexpr size_t FQ_BYTES = (FqP::BITS + 2 + 7) / 8;   // serialize_with_flags::<SWFlags>: 2 flag bits
    static constexpr size_t FR_BYTES = (FrP::BITS + 7) / 8;

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
    static int challenge(Strobe128& st, const uint8_t* label, size_t len, uint64_t* out_mont);
};

void transcript_append(Strobe128& st, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
    const uint32_t n = (uint32_t)msg_len;
    const uint8_t le[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
    st.meta_ad(label, label_len, false);
    st.meta_ad(le, 4, true);
    st.ad(msg, msg_len, false);
}
void transcript_challenge(Strobe128& st, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
    const uint32_t n = (uint32_t)out_len;
    const uint8_t le[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
    st.meta_ad(label, label_len, false);
    st.meta_ad(le, 4, true);
    st.prf(out, out_len, false);
}

template <class Cv>
int Wire<Cv>::challenge(Strobe128& st, const uint8_t* label, size_t len, uint64_t* out_mont) {
    constexpr size_t SZ = FrP::BITS / 8;      // 31 for both curves: always below the modulus
    uint8_t buf[32] = {0};
    transcript_challenge(st, label, len, buf, SZ);
    Fr x;
    if (!fp_from_le_bytes<Fr, FrP>(buf, 32, x)) return ZK_ERR_BAD_ARG;
    memcpy(out_mont, x.v, 32);
    return ZK_OK;
}

}  // namespace

struct zk_transcript {
    Strobe128 st;
    explicit zk_transcript(const uint8_t* l, size_t n) : st((const uint8_t*)"Merlin v1.0", 11) { transcript_append(st, (const uint8_t*)"dom-sep", 7, l, n); }
};

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
    return new zk_transcript(label, label_len);
}
zk_transcript* zk_transcript_clone(const zk_transcript* t) { return t ? new zk_transcript(*t) : nullptr; }
void zk_transcript_free(zk_transcript* t) { delete t; }
int zk_transcript_append_message(zk_transcript* t, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
    if (!t || (!label && label_len) || (!msg && msg_len)) return ZK_ERR_BAD_ARG;
    transcript_append(t->st, label, label_len, msg, msg_len);
    return ZK_OK;
}
int zk_transcript_append_u64(zk_transcript* t, const uint8_t* label, size_t label_len, uint64_t v) {
    uint8_t le[8];
    for (int i = 0; i < 8; ++i) le[i] = (uint8_t)(v >> (8 * i));
    return zk_transcript_append_message(t, label, label_len, le, 8);
}
int zk_transcript_challenge_bytes(zk_transcript* t, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
    if (!t || (!label && label_len) || (!out && out_len)) return ZK_ERR_BAD_ARG;
    transcript_challenge(t->st, label, label_len, out, out_len);
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
// `PublicInputs { values: BTreeMap<usize, F> }` (pi.rs:28-36) under `label` (prover.rs:182 uses b"pi"):
// u64 count, then (u64 position, Fr) in ascending position order.  `PublicInputs::insert` (pi.rs:56-65) drops zero values
// ("zeros are the implicit value of empty positions"), so the reference's map never holds one -- neither on the prover's nor on
// the verifier's side: a zero entry handed in here is skipped the same way, it is not part of the message.
int zk_transcript_append_public_inputs(zk_transcript* t, int curve_id, const uint8_t* label, size_t label_len, const uint64_t* positions,
                                       const uint64_t* values_mont, size_t n) {
    if (!t || (n && (!positions || !values_mont))) return ZK_ERR_BAD_ARG;
    const size_t f = zk_fr_serialized_size(curve_id);
    if (!f) return ZK_ERR_BAD_ARG;
    for (size_t i = 1; i < n; ++i)
        if (positions[i] <= positions[i - 1]) return ZK_ERR_BAD_ARG;     // a BTreeMap iterates in strictly ascending key order
    auto is_zero = [&](size_t i) { return (values_mont[4 * i] | values_mont[4 * i + 1] | values_mont[4 * i + 2] | values_mont[4 * i + 3]) == 0; };
    size_t kept = 0;
    for (size_t i = 0; i < n; ++i) kept += is_zero(i) ? 0 : 1;
    std::vector<uint8_t> buf(8 + kept * (8 + f));
    uint8_t* w = buf.data();
    for (int b = 0; b < 8; ++b) *w++ = (uint8_t)((uint64_t)kept >> (8 * b));
    for (size_t i = 0; i < n; ++i) {
        if (is_zero(i)) continue;
        for (int b = 0; b < 8; ++b) *w++ = (uint8_t)(positions[i] >> (8 * b));
        int rc = zk_fr_serialize(curve_id, values_mont + 4 * i, w);
        if (rc) return rc;
        w += f;
    }
    return zk_transcript_append_message(t, label, label_len, buf.data(), buf.size());
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
namespace {

// the seven custom evaluations the verifier reads by label (proof.rs:488-611), in the order of the evaluation row
const char* const VERIFY_CUSTOM[7] = {"a_next_eval", "b_next_eval", "d_next_eval", "q_arith_eval", "q_c_eval", "q_l_eval", "q_r_eval"};

uint64_t le_u64(const uint8_t* p) {
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// One proof: walk proof.rs:41-103, then replay proof.rs:128-300, 343-378 on a copy of the seeded transcript.
// points_out (optional): the 13 commitments and the two openings, FQ_BYTES each, as they stand in the proof.
template <class Cv>
uint8_t replay_one(const zk_transcript& seeded, const uint8_t* data, size_t len, const uint64_t* pi_pos, const uint64_t* pi_val, size_t n_pi,
                   uint64_t* ch_out, uint64_t* ev_out, uint8_t* points_out) {
    typedef Wire<Cv> W;
    constexpr size_t G = W::FQ_BYTES, F = W::FR_BYTES;
    constexpr int CID = Cv::ID;
    size_t pos = 0;
    const uint8_t* pts[15];
    for (int i = 0; i < 15; ++i) {
        if (len - pos < G) return ZK_PROOF_TRUNCATED;
        pts[i] = data + pos;
        pos += G;
        if (i >= 13) {                                       // kzg10::Proof { w, random_v }: random_v is None in every proof of this scheme
            if (len - pos < 1) return ZK_PROOF_TRUNCATED;
            if (data[pos] != 0) return ZK_PROOF_BAD_OPTION;
            pos += 1;
        }
    }
    if (points_out) {
        for (int i = 0; i < 15; ++i) memcpy(points_out + i * G, pts[i], G);
    }
    for (int i = 0; i < ZK_PROOF_N_EVALS; ++i) {
        if (len - pos < F) return ZK_PROOF_TRUNCATED;
        if (W::fr_de(data + pos, ev_out + 4 * i)) return ZK_PROOF_FR_NOT_REDUCED;
        pos += F;
    }
    if (len - pos < 8) return ZK_PROOF_TRUNCATED;
    const uint64_t k = le_u64(data + pos);
    pos += 8;
    if (k > (len - pos) / (8 + F)) return ZK_PROOF_BAD_COUNT;       // more entries than bytes: also bounds the loop below
    struct Custom {
        const uint8_t* label;
        size_t label_len;
        uint64_t v[4];
    };
    std::vector<Custom> custom((size_t)k);
    for (uint64_t i = 0; i < k; ++i) {
        if (pos == len) return ZK_PROOF_BAD_COUNT;                  // the bytes end on an entry boundary with entries still announced
        if (len - pos < 8) return ZK_PROOF_TRUNCATED;
        const uint64_t ll = le_u64(data + pos);
        pos += 8;
        if (ll > len - pos || len - pos - ll < F) return ZK_PROOF_TRUNCATED;
        Custom& c = custom[(size_t)i];
        c.label = data + pos;
        c.label_len = (size_t)ll;
        pos += (size_t)ll;
        if (W::fr_de(data + pos, c.v)) return ZK_PROOF_FR_NOT_REDUCED;
        pos += F;
    }
    if (pos != len) return ZK_PROOF_TRAILING;
    for (int j = 0; j < 7; ++j) {
        const size_t ll = strlen(VERIFY_CUSTOM[j]);
        const Custom* hit = nullptr;
        for (const Custom& c : custom)
            if (c.label_len == ll && memcmp(c.label, VERIFY_CUSTOM[j], ll) == 0) hit = &c;     // a repeated label: the last one counts
        if (!hit) return ZK_PROOF_MISSING_LABEL;
        memcpy(ev_out + 4 * (ZK_PROOF_N_EVALS + j), hit->v, 32);
    }

    zk_transcript t(seeded);
    if (zk_transcript_append_public_inputs(&t, CID, (const uint8_t*)"pi", 2, pi_pos, pi_val, n_pi)) return ZK_PROOF_BAD_PUBLIC_INPUTS;
    // ark appends the re-serialised point: for a decodable encoding that is the proof's own bytes, except that infinity is written with x = 0
    auto put_g1 = [&](const char* label, int i) {
        uint8_t buf[G];
        memcpy(buf, pts[i], G);
        if ((buf[G - 1] & 0xC0) == 0x40) {
            memset(buf, 0, G);
            buf[G - 1] = 0x40;
        }
        transcript_append(t.st, (const uint8_t*)label, strlen(label), buf, G);
    };
    auto put_fr = [&](const char* label, const uint64_t* mont) {
        uint8_t buf[F];
        W::fr_ser(mont, buf);
        transcript_append(t.st, (const uint8_t*)label, strlen(label), buf, F);
    };
    int slot = 0;
    auto draw = [&](const char* label, const char* put) {
        uint64_t* c = ch_out + 4 * slot++;
        W::challenge(t.st, (const uint8_t*)label, strlen(label), c);
        if (put) put_fr(put, c);
    };
    // indices into pts: a b c d z f h_1 h_2 z_2 t_1 t_2 t_3 t_4
    put_g1("w_l", 0), put_g1("w_r", 1), put_g1("w_o", 2), put_g1("w_4", 3);
    draw("zeta", "zeta");
    put_g1("f", 5), put_g1("h1", 6), put_g1("h2", 7);
    draw("beta", "beta"), draw("gamma", "gamma"), draw("delta", "delta"), draw("epsilon", "epsilon");
    put_g1("z", 4);
    draw("alpha", "alpha");
    draw("range separation challenge", "range seperation challenge");
    draw("logic separation challenge", "logic seperation challenge");
    draw("fixed base separation challenge", "fixed base separation challenge");
    draw("variable base separation challenge", "variable base separation challenge");
    draw("lookup separation challenge", "lookup separation challenge");
    put_g1("t_1", 9), put_g1("t_2", 10), put_g1("t_3", 11), put_g1("t_4", 12);
    draw("z", "z");
    // the 14 evaluations proof.rs:253-300 appends, by their index in the proof's evaluation block
    static const struct {
        const char* label;
        int idx;
    } EV[14] = {{"a_eval", 0}, {"b_eval", 1}, {"c_eval", 2}, {"d_eval", 3}, {"left_sig_eval", 4}, {"right_sig_eval", 5}, {"out_sig_eval", 6},
                {"perm_eval", 7}, {"f_eval", 13}, {"q_lookup_eval", 8}, {"lookup_perm_eval", 9}, {"h_1_eval", 10}, {"h_1_next_eval", 11},
                {"h_2_eval", 12}};
    for (const auto& e : EV) put_fr(e.label, ev_out + 4 * e.idx);
    for (const Custom& c : custom) {
        uint8_t buf[F];
        W::fr_ser(c.v, buf);
        transcript_append(t.st, c.label, c.label_len, buf, F);
    }
    draw("aggregate_witness", nullptr);
    draw("aggregate_witness", nullptr);
    return ZK_PROOF_OK;
}

}  // namespace

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
            return replay_one<decltype(cv)>(*seeded, proofs[j], proof_lens[j], n_pi ? pi_positions + o : nullptr, n_pi ? pi_values_mont + 4 * o : nullptr,
                                            n_pi, ch, ev, pt);
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
