// Host-side harness for the unsaturated fields / the XYZZ group law (fieldu.cuh, fields.cuh, ecu.cuh): the same
// templates the HIP kernels instantiate, and the law's host instantiation over the saturated field (field.cuh), compiled with g++ so
// tests/test_fieldu.py can check them against the big-int oracle without a GPU; and for the device-only load conversion of the quotient kernel and the circuit
// check (zbound.cuh) and the hash of the device key maps (fr_io.cuh).  The group law is instantiated a third time over Fb (fb_field.h), the
// signed-limb field with the preconditions of fields.cuh checked at every call, and with it the quad-cooperative law of ecq.cuh (fb_laws.h).
#include <cstdint>
#include <cstring>
#include <type_traits>
#include "../../ark_plonk_amd/csrc/curve_params.h"
#include "../../ark_plonk_amd/csrc/field.cuh"
#include "../../ark_plonk_amd/csrc/fieldu.cuh"
#include "../../ark_plonk_amd/csrc/ecu.cuh"
#if !defined(__HIPCC__)
struct uint4 {                            // the 16-byte vector type of the device headers, for the host build
    uint32_t x, y, z, w;
};
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
#endif
#include "../../ark_plonk_amd/csrc/fr_io.cuh"
#include "../../ark_plonk_amd/csrc/domain.cuh"
#include "../../ark_plonk_amd/csrc/zbound.cuh"
#include "fb_field.h"                     // the checked signed-limb field Fb: the contract of fields.cuh at every call
#include "fb_laws.h"                      // ecu.cuh and ecq.cuh over Fb, one run per branch (brings in ecq.cuh with host wave primitives)

template <class F>
struct is_fs : std::false_type {};
template <class P>
struct is_fs<Fs<P>> : std::true_type {};
template <class F>
struct is_fp : std::false_type {};
template <class P>
struct is_fp<Fp<P>> : std::true_type {};

// x - y and -x as each field names them: Fu says which multiple of p keeps the value positive (8p, or 16p for `wide`), Fs has one of each
template <class F>
static F f_sub(const F& x, const F& y, bool wide) {
    if constexpr (is_fs<F>::value) return F::sub(x, y);
    else return wide ? F::sub16(x, y) : F::sub8(x, y);
}
template <class F>
static F f_neg(const F& x) {
    if constexpr (is_fs<F>::value) return F::neg(x);
    else return F::neg_canonical(x);
}

template <class F>
static void fs_dot2(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    F x = F::from_sat(a), y = F::from_sat(b), r;
    if (op == 9) r = F::dot2(x, y, F::sub(x, y), F::add3(x, x, y));         // x*y + (x - y)(2x + y) with one reduction
    else if (op == 10) r = F::dot2(x, y, F::neg(y), y);                     // x*y - y*y through the negated operand
    else r = F::sub_sum3(F::mul(x, y), F::sqr(x), F::sqr(y), F::mul(x, x));  // xy - 2x^2 - y^2, one carry step
    r.to_sat(out);
}

template <class F>
static void fu_binop(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    F x = F::from_sat(a), y = F::from_sat(b), r;
    switch (op) {
    case 0: r = F::mul(x, y); break;
    case 1: r = F::add(x, y); break;
    case 2: r = f_sub(x, y, false); break;
    case 3: r = f_sub(x, y, true); break;
    case 4: r = F::sqr(x); break;
    case 5: r = F::inverse(x); break;
    case 6: r = f_neg(x); break;
    case 7: r = F::dbl(x); break;
    case 8: {  // a long lazy chain: ((x - y + 16p) * (x + x + y) - x*y + 8p)^2
        F t = F::mul(f_sub(x, y, true), F::add3(x, x, y));
        r = F::sqr(f_sub(t, F::mul(x, y), false));
        break;
    }
    default: r = F::zero();
    }
    r.to_sat(out);
}

// a coordinate in / out of the law's field: Fp holds the arkworks words themselves, Fs converts (stored coordinates are canonical)
template <class F>
constexpr int sat_words() {
    if constexpr (is_fp<F>::value) return F::N;
    else return F::SAT;
}
template <class F>
static F coord_in(const uint32_t* w) {
    if constexpr (is_fp<F>::value) {
        F f;
        memcpy(f.v, w, sizeof f.v);
        return f;
    } else {
        return F::canonical_lt2p(F::from_sat(w));
    }
}
template <class F>
static void coord_out(const F& f, uint32_t* w) {
    if constexpr (is_fp<F>::value) memcpy(w, f.v, sizeof f.v);
    else f.to_sat(w);
}

// acc (affine or infinity) + sequence of affine points with signs -> affine result
template <class F>
static int xyzz_chain(const uint32_t* pts_xy, const uint8_t* flags /* bit0 negate, bit1 use full add, bit2 double acc first */, int n,
                      uint32_t* out_xy) {
    constexpr int W = sat_words<F>();
    XYZZu<F> acc = XYZZu<F>::infinity();
    for (int i = 0; i < n; ++i) {
        AffineU<F> p;
        p.x = coord_in<F>(pts_xy + (2 * i) * W);
        p.y = coord_in<F>(pts_xy + (2 * i + 1) * W);
        bool null = true;
        for (int k = 0; k < 2 * W; ++k) null = null && pts_xy[2 * i * W + k] == 0;
        if (null) continue;
        if (flags[i] & 1) p.y = F::neg(p.y);
        if (flags[i] & 4) acc = XYZZu<F>::dbl(acc);
        if (flags[i] & 2) acc = XYZZu<F>::add(acc, XYZZu<F>::from_affine(p));
        else acc = XYZZu<F>::madd(acc, p);
    }
    AffineU<F> a;
    bool fin = acc.to_affine(a);
    coord_out(a.x, out_xy);
    coord_out(a.y, out_xy + W);
    return fin ? 0 : 1;
}

typedef Fu<FrBls12_381UParams> FrB;      // 29-bit limbs (fieldu.cuh): the scalar fields
typedef Fu<FrBn254UParams> FrN;
typedef Fs<FqBls12_381SParams> FqBs;     // signed 30-bit limbs (fields.cuh): the base fields
typedef Fs<FqBn254SParams> FqNs;
typedef Fb<FqBls12_381SParams> FqBb;     // the same, with the preconditions of fields.cuh checked at every call (fb_field.h)
typedef Fb<FqBn254SParams> FqNb;

// the device-only pieces of the quotient kernel and the circuit check: the load conversion (zbound.cuh) and the hash of the key maps
// (fr_io.cuh), over the three members of a curve they read
struct HostBls {
    typedef Fp<FrBls12_381Params> Fr;
    typedef FrB FrU;
    typedef FrBls12_381Params FrP;
};
struct HostBn {
    typedef Fp<FrBn254Params> Fr;
    typedef FrN FrU;
    typedef FrBn254Params FrP;
};
constexpr uint32_t RP_ROWS = 64;         // multiples of r held by the harness: more than either kernel holds
static El el_of(const uint32_t* w) {
    El e;
    e.a = make_uint4(w[0], w[1], w[2], w[3]);
    e.b = make_uint4(w[4], w[5], w[6], w[7]);
    return e;
}
template <class Cv>
static void to_rp_many(const uint32_t* words_in, uint32_t* limbs_out, uint64_t n) {
    typedef typename Cv::FrU FU;
    static uint32_t rtab[RP_ROWS][FU::NL];
    uint32_t ratio_fx, top_shift;
    rp_table<Cv>(rtab, RP_ROWS, ratio_fx, top_shift);
    for (uint64_t k = 0; k < n; ++k) {
        const Z<FU, RP_B> z = to_rp<FU>(el_of(words_in + 8 * k), rtab, ratio_fx, top_shift);
        for (int i = 0; i < FU::NL; ++i) limbs_out[FU::NL * k + i] = z.v.v[i];
    }
}
// x R (stored words, canonical) -> x R' three ways: the packer behind every kernel-argument multiplier (pack_rp, fr_io.cuh: doublings),
// to_rp_host (zbound.cuh) as limbs, and the route the units used to write out: one Montgomery product with R' mod r as a plain integer
template <class Cv>
static void pack_rp_many(const uint32_t* words_in, uint32_t* packed_out, uint32_t* limbs_out, uint32_t* product_out, uint64_t n) {
    typedef typename Cv::Fr Fr;
    typedef typename Cv::FrU FU;
    Fr rp;
    FU::one().pack_words(rp.v);
    for (uint64_t k = 0; k < n; ++k) {
        Fr v;
        memcpy(v.v, words_in + 8 * k, 32);
        const Packed p = pack_rp(v);
        memcpy(packed_out + 8 * k, p.w, 32);
        const FU l = to_rp_host<Cv>(v);
        for (int i = 0; i < FU::NL; ++i) limbs_out[FU::NL * k + i] = l.v[i];
        const Fr m = Fr::mul(v, rp);
        memcpy(product_out + 8 * k, m.v, 32);
    }
}
// the domain constants (domain.cuh) as stored words, and the shared constants of the two gate-argument blocks (fill_gate_consts,
// zbound.cuh) filled into a block of the harness's own: the members the filler names, in an order neither kernel's block has
template <class Cv>
static void id_consts_of(uint32_t log_n, uint32_t* words_out) {
    typename Cv::Fr cs[ID_N_CONSTS];
    fill_id_consts<Cv>(log_n, cs);
    for (uint32_t k = 0; k < ID_N_CONSTS; ++k) memcpy(words_out + 8 * k, cs[k].v, 32);
}
template <class FU>
struct GateBlock {
    uint32_t top_shift, ratio_fx;
    uint32_t rtab[RP_ROWS][FU::NL];
    FU c83, c81, c18, c9, c4, c3, c2, one, coeff_d, coeff_a;
};
template <class Cv>
static void gate_consts_of(const uint64_t* coeff_a, const uint64_t* coeff_d, uint32_t table_len, uint32_t* limbs_out, uint32_t* rtab_out,
                           uint32_t* scalars_out) {
    typedef typename Cv::FrU FU;
    static GateBlock<FU> A;
    fill_gate_consts<Cv>(A, coeff_a, coeff_d, table_len);
    const FU* c[10] = {&A.coeff_a, &A.coeff_d, &A.one, &A.c2, &A.c3, &A.c4, &A.c9, &A.c18, &A.c81, &A.c83};
    for (int k = 0; k < 10; ++k)
        for (int i = 0; i < FU::NL; ++i) limbs_out[FU::NL * k + i] = c[k]->v[i];
    for (uint32_t q = 0; q < table_len; ++q)
        for (int i = 0; i < FU::NL; ++i) rtab_out[FU::NL * q + i] = A.rtab[q][i];
    scalars_out[0] = A.ratio_fx;
    scalars_out[1] = A.top_shift;
}
template <int W>
static uint32_t key_hash_of(const uint32_t* words) {
    Key<W> k;
    for (int j = 0; j < W; ++j) k.e[j] = el_of(words + 8 * j);
    return key_hash<W>(k);
}

// raw signed-limb operands (no conversion on the way in): the worst-case limb patterns of the column bounds of fields.cuh.
// op 0: mul(a, b)   1: sqr(a)   2: dot2(a, b, c, d)   3: sub_sum3(a, b, c, d) (strict operands)   4: add3 / sub chains
// and every operator alone, for the rule table of fb_field.h: 5 add(a, b)   6 sub(a, b)   7 dbl(a)   8 add3(a, b, c)   9 neg(a)
// 10 canonical_lt2p(a)   11 is_zero_mod_reduced(a) and 12 limb0_of_zero_mod(a), the flag in out[0]
template <class F>
static void fs_raw(int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out) {
    F x, y, z, w, r;
    for (int i = 0; i < F::NL; ++i) {
        x.v[i] = (uint32_t)a[i];
        y.v[i] = (uint32_t)b[i];
        z.v[i] = (uint32_t)c[i];
        w.v[i] = (uint32_t)d[i];
    }
    switch (op) {
    case 0: r = F::mul(x, y); break;
    case 1: r = F::sqr(x); break;
    case 2: r = F::dot2(x, y, z, w); break;
    case 3: r = F::sub_sum3(x, y, z, w); break;
    case 5: r = F::add(x, y); break;
    case 6: r = F::sub(x, y); break;
    case 7: r = F::dbl(x); break;
    case 8: r = F::add3(x, y, z); break;
    case 9: r = F::neg(x); break;
    case 10: r = F::canonical_lt2p(x); break;
    case 11: r = F::zero(); r.v[0] = x.is_zero_mod_reduced(); break;
    case 12: r = F::zero(); r.v[0] = x.limb0_of_zero_mod(); break;
    default: r = F::sub(F::add3(x, y, z), w); break;
    }
    for (int i = 0; i < F::NL; ++i) out[i] = (int32_t)r.v[i];
}

// raw 29-bit-limb operands (no conversion on the way in or out): the limb patterns of lazily reduced intermediates, which no stored
// word can choose.  The normalising operators of fieldu.cuh: 0 mul(a, b)   1 mul_fenced(a, b)   2 sqr(a)   3 add(a, b)   4 add3(a, b, c)
// 5 sub2(a, b)   6 sub8(a, b)   7 sub16(a, b)   8 neg16(a); the lazily normalised ones of the NTT butterflies: 9 add_raw(a, b)
// 10 sub_raw3(a, b)   11 sub_raw8(a, b)   12 sub_raw16(a, b)   13 sweep(a); and 14 canonical_lt2p(a)   15 is_zero_mod_reduced(a), the flag
// in out[0]
template <class F>
static void fu_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
    F x, y, z, r;
    for (int i = 0; i < F::NL; ++i) {
        x.v[i] = a[i];
        y.v[i] = b[i];
        z.v[i] = c[i];
    }
    switch (op) {
    case 0: r = F::mul(x, y); break;
    case 1: r = F::mul_fenced(x, y); break;
    case 2: r = F::sqr(x); break;
    case 3: r = F::add(x, y); break;
    case 4: r = F::add3(x, y, z); break;
    case 5: r = F::sub2(x, y); break;
    case 6: r = F::sub8(x, y); break;
    case 7: r = F::sub16(x, y); break;
    case 8: r = F::neg16(x); break;
    case 9: r = F::add_raw(x, y); break;
    case 10: r = F::sub_raw3(x, y); break;
    case 11: r = F::sub_raw8(x, y); break;
    case 12: r = F::sub_raw16(x, y); break;
    case 13: r = x; F::sweep(r); break;
    case 14: r = F::canonical_lt2p(x); break;
    case 15: r = F::zero(); r.v[0] = x.is_zero_mod_reduced(); break;
    default: r = F::zero();
    }
    for (int i = 0; i < F::NL; ++i) out[i] = r.v[i];
}

extern "C" {
int fu_limbs(int field) { return field == 1 ? FrB::NL : FrN::NL; }
// field: 1 Fr-BLS, 3 Fr-BN (as fu_op)
void fu_raw_op(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
    if (field == 1) fu_raw<FrB>(op, a, b, c, out);
    else fu_raw<FrN>(op, a, b, c, out);
}
int fs_limbs(int field) { return field == 0 ? FqBs::NL : FqNs::NL; }
void fs_raw_op(int field, int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out) {
    if (field == 0) fs_raw<FqBs>(op, a, b, c, d, out);
    else fs_raw<FqNs>(op, a, b, c, d, out);
}
// field: 0 Fq-BLS, 2 Fq-BN (signed 30-bit limbs); 1 Fr-BLS, 3 Fr-BN (29-bit limbs)
void fu_op(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    switch (field) {
    case 0: op >= 9 ? fs_dot2<FqBs>(op, a, b, out) : fu_binop<FqBs>(op, a, b, out); break;
    case 1: fu_binop<FrB>(op, a, b, out); break;
    case 2: op >= 9 ? fs_dot2<FqNs>(op, a, b, out) : fu_binop<FqNs>(op, a, b, out); break;
    case 3: fu_binop<FrN>(op, a, b, out); break;
    }
}
// field: 1 Fr-BLS, 3 Fr-BN.  n stored words (8 x 32 bits each, canonical) -> the limbs to_rp returns (FrU::NL each), as they are
void fu_to_rp(int field, const uint32_t* words_in, uint32_t* limbs_out, uint64_t n) {
    if (field == 1) to_rp_many<HostBls>(words_in, limbs_out, n);
    else to_rp_many<HostBn>(words_in, limbs_out, n);
}
void fu_pack_rp(int field, const uint32_t* words_in, uint32_t* packed_out, uint32_t* limbs_out, uint32_t* product_out, uint64_t n) {
    if (field == 1) pack_rp_many<HostBls>(words_in, packed_out, limbs_out, product_out, n);
    else pack_rp_many<HostBn>(words_in, packed_out, limbs_out, product_out, n);
}
// field: 1 Fr-BLS, 3 Fr-BN.  domain.cuh: the two-adicity guard; the root of unity of the size-2^log_n domain (8 stored words); the
// ID_N_CONSTS constants of the identity encoding (8 words each)
int fu_domain_log_ok(int field, uint32_t log_n) { return field == 1 ? domain_log_ok<HostBls>(log_n) : domain_log_ok<HostBn>(log_n); }
void fu_domain_root(int field, uint32_t log_n, uint32_t* words_out) {
    if (field == 1) memcpy(words_out, domain_root<HostBls>(log_n).v, 32);
    else memcpy(words_out, domain_root<HostBn>(log_n).v, 32);
}
int fu_id_n_consts() { return (int)ID_N_CONSTS; }
void fu_id_consts(int field, uint32_t log_n, uint32_t* words_out) {
    if (field == 1) id_consts_of<HostBls>(log_n, words_out);
    else id_consts_of<HostBn>(log_n, words_out);
}
// table_len <= 64 rows.  limbs_out: coeff_a, coeff_d, one, c2, c3, c4, c9, c18, c81, c83 (FrU::NL limbs each); rtab_out: table_len rows;
// scalars_out: ratio_fx, top_shift
void fu_gate_consts(int field, const uint64_t* coeff_a, const uint64_t* coeff_d, uint32_t table_len, uint32_t* limbs_out, uint32_t* rtab_out,
                    uint32_t* scalars_out) {
    if (field == 1) gate_consts_of<HostBls>(coeff_a, coeff_d, table_len, limbs_out, rtab_out, scalars_out);
    else gate_consts_of<HostBn>(coeff_a, coeff_d, table_len, limbs_out, rtab_out, scalars_out);
}
int fu_rp_bound() { return RP_B; }      // a loaded value is < RP_B / 10 * r
int fu_rp_limbs() { return FrB::NL; }
uint64_t fu_el_mix(uint64_t h, const uint32_t* words) { return el_mix(h, el_of(words)); }
uint32_t fu_key_hash(int w, const uint32_t* words) { return w == 1 ? key_hash_of<1>(words) : key_hash_of<4>(words); }
// law: 0 BLS12-381, 1 BN254 over the signed-limb field (the device's instantiation); 2, 3 the same curves over the saturated field (the host's)
int fu_xyzz_chain(int law, const uint32_t* pts_xy, const uint8_t* flags, int n, uint32_t* out_xy) {
    switch (law) {
    case 0: return xyzz_chain<FqBs>(pts_xy, flags, n, out_xy);
    case 1: return xyzz_chain<FqNs>(pts_xy, flags, n, out_xy);
    case 2: return xyzz_chain<Fp<FqBls12_381Params>>(pts_xy, flags, n, out_xy);
    case 3: return xyzz_chain<Fp<FqBn254Params>>(pts_xy, flags, n, out_xy);
    case 4: return xyzz_chain<FqBb>(pts_xy, flags, n, out_xy);      // the signed-limb field, checked: violations go to the record
    case 5: return xyzz_chain<FqNb>(pts_xy, flags, n, out_xy);
    }
    return -1;
}
// ---- the checked field (fb_field.h, fb_laws.h).  field / cid: 0 BLS12-381, 1 BN254
// the rule table: operation (fb::Op) and operand envelopes (lo, hi, V in units of 2^-16 p each) in; ok flag and result envelope out
int fb_units() { return (int)fb::VU; }
int fb_op_count() { return fb::OP_COUNT; }
const char* fb_op_name(int op) { return fb::op_name(op); }
int fb_op_arity(int op) { return fb::op_arity(op); }
int fb_rule(int field, int op, const int64_t* operands, int64_t* result) {
    fb::Env e[4] = {};
    for (int i = 0; i < fb::op_arity(op); ++i) e[i] = fb::Env{operands[3 * i], operands[3 * i + 1], operands[3 * i + 2]};
    const fb::RuleOut r = field == 0 ? fb::rule(op, e, FqBb::tp(), FqBb::words_v()) : fb::rule(op, e, FqNb::tp(), FqNb::words_v());
    result[0] = r.res.lo;
    result[1] = r.res.hi;
    result[2] = r.res.V;
    return r.ok ? 1 : 0;
}
// the records since the last call, one per line, then forgotten; returns their number
int fb_log_take(char* out, int cap) {
    std::lock_guard<std::mutex> g(fb::log_mutex());
    std::string s;
    for (const fb::Record& r : fb::log()) s += fb::record_text(r) + "\n";
    const int n = (int)fb::log().size();
    fb::log().clear();
    snprintf(out, (size_t)cap, "%s", s.c_str());
    return n;
}
// which: 0 the single-lane law of ecu.cuh, 1 qadd / qdbl of ecq.cuh.  words: two affine points P, Q (x, y, x, y; arkworks words).
// Writes "CASE name" per case run, "FAIL ..." / "VIOLATION ..." per failure, "QUADVIOLATION ..." per record of a quad lane; returns
// the failures other than quad records
int fb_closure(int cid, int which, const uint32_t* words, char* out, int cap) {
    return cid == 0 ? fbl::closure<FqBls12_381SParams>(which, words, out, cap) : fbl::closure<FqBn254SParams>(which, words, out, cap);
}
}
