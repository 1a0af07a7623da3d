// Loads / stores of scalar-field elements, defined once for every unit that is free to include it:
// the 32-byte element as the 8 x 32-bit-word type of field.cuh (ld_fr / st_fr) and as an opaque value (El: equality, zero test,
// hash mix), and for the kernels that work on the 29-bit-limb Fr type: 32-byte arkworks elements <-> limbs with no domain change,
// lazily reduced limb vectors (48 bytes), and the kernel-argument form of a constant multiplier -- untyped here; kzg.hip and
// lookup.hip reach them through the typed forms of zbound.cuh.  Host side: the one conversion x R -> x R' behind every such
// multiplier (and behind the NTT's tables), and the "is a reduced field element" test of the ABI's scalar arguments.
#pragma once
#include "zk_common.h"

namespace {

// ---- the 32-byte element as two 16-byte accesses: the saturated type of field.cuh (arkworks Montgomery or canonical, as stored)
template <class Fr>
ZK_D Fr ld_fr(const void* base, uint64_t idx) {
    const uint4* q = reinterpret_cast<const uint4*>(base) + 2 * idx;
    uint4 a = q[0], b = q[1];
    Fr r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
template <class Fr>
ZK_D void st_fr(void* base, uint64_t idx, const Fr& r) {
    uint4* q = reinterpret_cast<uint4*>(base) + 2 * idx;
    q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

// ---- the same 32 bytes as a value that is only compared and hashed (lookup.hip's multiset table, check.hip's key maps)
struct El {
    uint4 a, b;
};
ZK_D El ld_el(const void* base, uint64_t i) {
    const uint4* q = reinterpret_cast<const uint4*>(base) + 2 * i;
    El e;
    e.a = q[0];
    e.b = q[1];
    return e;
}
ZK_D void st_el(void* base, uint64_t i, const El& e) {
    uint4* q = reinterpret_cast<uint4*>(base) + 2 * i;
    q[0] = e.a;
    q[1] = e.b;
}
ZK_D bool el_eq(const El& x, const El& y) {
    return x.a.x == y.a.x && x.a.y == y.a.y && x.a.z == y.a.z && x.a.w == y.a.w && x.b.x == y.b.x && x.b.y == y.b.y && x.b.z == y.b.z &&
           x.b.w == y.b.w;
}
ZK_D bool el_zero(const El& x) { return (x.a.x | x.a.y | x.a.z | x.a.w | x.b.x | x.b.y | x.b.z | x.b.w) == 0; }
// 64-bit mix, chained over the elements of a key: h = 0 for the first (or only) element
ZK_D uint64_t el_mix(uint64_t h, const El& e) {
    h ^= ((uint64_t)e.a.y << 32 | e.a.x) * 0x9E3779B97F4A7C15ull;
    h ^= ((uint64_t)e.a.w << 32 | e.a.z) * 0xC2B2AE3D27D4EB4Full;
    h ^= ((uint64_t)e.b.y << 32 | e.b.x) * 0x165667B19E3779F9ull;
    h ^= ((uint64_t)e.b.w << 32 | e.b.z) * 0xD6E8FEB86659FD93ull;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
    return h;
}
ZK_D uint32_t el_hash(const El& e) { return (uint32_t)el_mix(0, e); }
// a key of W elements (check.hip's maps: W = 4 a table row, W = 1 an identity encoding; lookup_map.hip's: W = 3, the (a, b, d) of a
// table row) and its hash; element j of key i is col[j][i]
template <int W>
struct Key {
    El e[W];
};
struct KeyCols {
    const void* col[4];
};
template <int W>
ZK_D Key<W> ld_key(const KeyCols& c, uint64_t i) {
    Key<W> k;
#pragma unroll
    for (int j = 0; j < W; ++j) k.e[j] = ld_el(c.col[j], i);
    return k;
}
template <int W>
ZK_D bool key_eq(const Key<W>& x, const Key<W>& y) {
    bool eq = true;
#pragma unroll
    for (int j = 0; j < W; ++j) eq = eq && el_eq(x.e[j], y.e[j]);
    return eq;
}
template <int W>
ZK_D uint32_t key_hash(const Key<W>& k) {
    uint64_t h = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) h = el_mix(h, k.e[j]);
    return (uint32_t)(h ^ (h >> 32));
}

// ---- the 29-bit-limb type

struct Packed {            // a field element as 8 little-endian words (kernel argument form)
    uint32_t w[8];
};

template <class FU>
ZK_D FU ld_u(const void* base, uint64_t idx) {       // 32-byte element -> limbs (no domain change)
    const uint4* q = reinterpret_cast<const uint4*>(base) + 2 * idx;
    uint4 a = q[0], b = q[1];
    uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return FU::split_words(w);
}
template <class FU>
ZK_D void st_u(void* base, uint64_t idx, const FU& x) {   // value < 2r -> canonical 32-byte element
    uint32_t w[8];
    FU::canonical_lt2p(x).pack_words(w);
    uint4* q = reinterpret_cast<uint4*>(base) + 2 * idx;
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// lazily reduced limb vectors: 9 limbs in 12 words
template <class FU>
ZK_D FU ld_l(const void* base, uint64_t idx) {
    const uint4* q = reinterpret_cast<const uint4*>(base) + 3 * idx;
    uint4 a = q[0], b = q[1], c = q[2];
    const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    FU r;
#pragma unroll
    for (int i = 0; i < FU::NL; ++i) r.v[i] = w[i];
    return r;
}
template <class FU>
ZK_D void st_l(void* base, uint64_t idx, const FU& x) {
    uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < FU::NL; ++i) w[i] = x.v[i];
    uint4* q = reinterpret_cast<uint4*>(base) + 3 * idx;
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
    q[2] = make_uint4(w[8], w[9], w[10], w[11]);
}
template <class FU>
ZK_D FU unpack(const Packed& p) { return FU::split_words(p.w); }

// ---- host side: the arguments of those kernels
// x R (arkworks form, R = 2^256) -> x R' mod r, R' = 2^261 the radix of the 29-bit-limb type: five modular doublings, canonical.
// to_rprime(Fr::one()) is R' mod r itself, the plain integer whose Montgomery product with x R is the same value (ntt.hip's tables).
template <class Fr>
Fr to_rprime(const Fr& v) {
    Fr t = v;
    for (int k = 0; k < 5; ++k) t = Fr::add(t, t);
    return t;
}
template <class Fr>
Packed pack_rp(const Fr& v) {                   // the kernel-argument form of the multiplier v
    Packed p;
    const Fr t = to_rprime(v);
    memcpy(p.w, t.v, 32);
    return p;
}
// the 4 x 64-bit words of an ABI argument as a field element; false when they are not a reduced one (the caller's ZK_ERR_BAD_ARG)
template <class Fr>
bool fr_reduced(const uint64_t* m, Fr& out) {
    memcpy(out.v, m, 32);
    return Fr::reduce_once(out) == out;
}

}  // namespace
