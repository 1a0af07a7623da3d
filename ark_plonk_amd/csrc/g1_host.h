// G1 points as the C ABI carries them, and the host's use of the group law: ecu.cuh over the saturated base field Fq (field.cuh).
// Host code only (msm_plan.hip, ipa.hip, wire.hip, commit.hip).  A coordinate is L = Fq::N / 2 64-bit limbs, Montgomery, arkworks layout.
//   Jacobian  X | Y | Z; infinity as arkworks writes GroupProjective::zero(): (1, 1, 0)
//   affine    x | y with an optional flag byte; infinity as GroupAffine::zero(): (0, 1), flag 1.  Read as infinity: the flag, or
//             x = 0 and y in {0, 1} (a caller without flags)
#pragma once
#include "ctx.h"

template <class Fq>
struct G1Host {
    typedef XYZZu<Fq> P;      // four Fq in a row: the layout the device writes its window sums in
    typedef AffineU<Fq> A;
    static constexpr int L = Fq::N / 2;

    static Fq ld(const uint64_t* w) {
        Fq f;
        memcpy(f.v, w, sizeof f.v);
        return f;
    }
    static void st(uint64_t* w, const Fq& f) { memcpy(w, f.v, sizeof f.v); }

    static bool jacobian_is_inf(const uint64_t* xyz) { return ld(xyz + 2 * L).is_zero(); }
    // Jacobian (X, Y, Z) -> XYZZ (X, Y, Z^2, Z^3); Z = 0 gives ZZ = 0, the law's infinity
    static P ld_jacobian(const uint64_t* xyz) {
        const Fq Z = ld(xyz + 2 * L);
        P p;
        p.x = ld(xyz);
        p.y = ld(xyz + L);
        p.zz = Fq::sqr(Z);
        p.zzz = Fq::mul(p.zz, Z);
        return p;
    }
    // XYZZ -> Jacobian (X*ZZ, Y*ZZZ, ZZ):  x = X/ZZ = X*ZZ/ZZ^2, y = Y/ZZZ = Y*ZZZ/ZZ^3
    static void st_jacobian(uint64_t* xyz, const P& p) {
        const bool inf = p.is_inf();
        st(xyz, inf ? Fq::one() : Fq::mul(p.x, p.zz));
        st(xyz + L, inf ? Fq::one() : Fq::mul(p.y, p.zzz));
        st(xyz + 2 * L, p.zz);
    }

    static A ld_affine(const uint64_t* xy) { return A{ld(xy), ld(xy + L)}; }
    static bool affine_is_inf(const A& a, uint8_t flag = 0) { return flag || (a.x.is_zero() && (a.y.is_zero() || a.y == Fq::one())); }
    static void st_affine(uint64_t* xy, uint8_t* inf, const A& a) {
        st(xy, a.x);
        st(xy + L, a.y);
        if (inf) *inf = 0;
    }
    static void st_affine_inf(uint64_t* xy, uint8_t* inf) {
        st(xy, Fq::zero());
        st(xy + L, Fq::one());
        if (inf) *inf = 1;
    }
    // the affine form of p (one field inversion)
    static void st_normalised(uint64_t* xy, uint8_t* inf, const P& p) {
        A a;
        if (p.to_affine(a)) st_affine(xy, inf, a);
        else st_affine_inf(xy, inf);
    }

    // k * q for a canonical k of n little-endian 32-bit words, q not infinity: double-and-add, most significant bit first
    static P scalar_mul(const A& q, const uint32_t* k, int n) {
        P acc = P::infinity();
        for (int w = n - 1; w >= 0; --w)
            for (int bit = 31; bit >= 0; --bit) {
                acc = P::dbl(acc);
                if ((k[w] >> bit) & 1u) acc = P::madd(acc, q);
            }
        return acc;
    }
};

// Jacobian infinity of a curve known by its id
inline void st_jacobian_inf(int curve, uint64_t* xyz) {
    zk_on_curve(curve, 0, [&](auto cv) {
        typedef G1Host<typename decltype(cv)::Fq> H;
        H::st_jacobian(xyz, H::P::infinity());
        return 0;
    });
}
