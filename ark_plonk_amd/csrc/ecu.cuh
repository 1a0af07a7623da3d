// The G1 group law (short Weierstrass, a = 0): the one definition, taken by the signed-limb Fs (fields.cuh) on the device and by the
// saturated Fp (field.cuh) on the host.
//
// Stands behind ark-ec 0.3 `GroupProjective::{add_assign_mixed, add_assign, double_in_place, into_affine}` as used by
// `VariableBaseMSM::multi_scalar_mul` (reference call sites: plonk-core/src/commitment.rs:45, every PC::commit in
// proof_system/prover.rs).  The reference accumulates in Jacobian coordinates; here points are kept in extended-Jacobian XYZZ
// (x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2; infinity <=> ZZ = 0) because the mixed addition is 8M + 2S with no field inversion and fewer
// live registers than Jacobian madd.  The formulas are madd-2008-s / add-2008-s / dbl-2008-s-1.  Results are compared after affine
// normalisation, where the group element has a single representation.
//
// Over Fs the law is written for the lazy reduction calculus of fields.cuh: limbs are signed, so a difference is just a difference, and
//   * products and squares come out in (-p, p) with strict limbs; stored coordinates are |X| < 4p (a
//     sum of four products, almost-balanced limbs) and Y, ZZ, ZZZ products;
//   * every operand of a product is a product, a stored coordinate or ONE sum / difference of those
//     (|value| < 12p, limbs re-centred by one carry step) -- the bound fields.cuh asks for;
//   * Y3 = R*(Q - X3) - Y1*PPP is ONE double product with one Montgomery reduction (dot2 against -Y1);
//   * P == +-Q is detected on the *result*: ZZ3 = ZZ1*PP is a product, so ZZ3 == 0 mod p iff its strict
//     limbs are those of 0 (or +-p) -- compares on one limb in the common path.
// These bullets are enforced, not only argued: tests/test_fieldu.py (test_g1_law_is_closed_under_the_signed_limb_contract) runs every
// function below once per branch outcome over a field that checks the preconditions of fields.cuh at each call (tests/native/fb_field.h),
// with the inputs widened to the class invariant -- X: |limb| <= 2^29 + 2, |X| < 4p; Y: |limb| <= 2^29, |Y| < p; ZZ, ZZZ: strict,
// below p in magnitude; affine x strict, affine y |limb| <= 2^29, both below p -- and demands that the outputs are inside it again.
// Over Fp every value is canonical, so none of these bounds is needed: add3 / sub_sum3 / dot2 are the plain sums, limbs_zero and
// is_zero_mod_reduced are both the exact zero test, and the law computes the same group elements with the same formulas.
// Infinity is ZZ = 0 with all limbs zero (only ever created explicitly, or read as such from a device sum).
#pragma once
#include "field.cuh"
#include "fields.cuh"

// A condition the compiler cannot see through.  Steps that exclude one another, written as `if (zk_apart(a)) A; if (zk_apart(b)) B;`,
// stay two blocks that a lane enters or walks past.  As alternatives (if / else) the device code lays them out one after the other
// with the values of one side alive across the other, and what both sides assign is moved into place at the join by every lane.
ZK_HD bool zk_apart(uint32_t flag) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(flag));
#endif
    return flag != 0;
}

template <class F>
struct AffineU {
    F x, y;  // over Fs: residues in (-p, p), strict limbs, R' Montgomery domain.  x = y = 0 limbs encodes "no point"
    ZK_HD bool is_null() const { return x.limbs_zero() && y.limbs_zero(); }
};

template <class F>
struct XYZZu {
    F x, y, zz, zzz;

    ZK_HD static XYZZu infinity() {
        XYZZu r;
        r.x = F::zero();
        r.y = F::zero();
        r.zz = F::zero();
        r.zzz = F::zero();
        return r;
    }
    ZK_HD bool is_inf() const { return zz.limbs_zero(); }

    ZK_HD static XYZZu from_affine(const AffineU<F>& p) {
        XYZZu r;
        r.x = p.x;
        r.y = p.y;
        r.zz = F::one();
        r.zzz = F::one();
        return r;
    }

    // 2 * (affine p), p not null
    ZK_HD static XYZZu dbl_affine(const AffineU<F>& p) {
        F u = F::dbl(p.y);
        F v = F::sqr(u);
        F w = F::mul(u, v);
        F s = F::mul(p.x, v);
        F xx = F::sqr(p.x);
        F m = F::add3(xx, xx, xx);
        XYZZu r;
        r.x = F::sub(F::sqr(m), F::dbl(s));
        r.y = F::dot2(m, F::sub(s, r.x), w, F::neg(p.y));   // m*(s - x3) - w*y, one reduction
        r.zz = v;
        r.zzz = w;
        return r;
    }

    ZK_HD static XYZZu dbl(const XYZZu& p) {
        if (p.is_inf()) return p;
        F u = F::dbl(p.y);
        F v = F::sqr(u);
        F w = F::mul(u, v);
        F s = F::mul(p.x, v);
        F xx = F::sqr(p.x);
        F m = F::add3(xx, xx, xx);
        XYZZu r;
        r.x = F::sub(F::sqr(m), F::dbl(s));
        r.y = F::dot2(m, F::sub(s, r.x), w, F::neg(p.y));
        r.zz = F::mul(v, p.zz);
        r.zzz = F::mul(w, p.zzz);
        return r;
    }

    // this + affine q (q not null); handles this == infinity, this == +-q
    ZK_HD static XYZZu madd(const XYZZu& p, const AffineU<F>& q) {
        if (p.is_inf()) return from_affine(q);
        F u2 = F::mul(q.x, p.zz);
        F s2 = F::mul(q.y, p.zzz);
        F pp_ = F::sub(u2, p.x);
        F r_ = F::sub(s2, p.y);
        F pp = F::sqr(pp_);
        F rr = F::sqr(r_);
        XYZZu o;
        o.zz = F::mul(p.zz, pp);
        if (o.zz.is_zero_mod_reduced()) {  // P == 0  <=>  same x
            if (rr.is_zero_mod_reduced()) return dbl_affine(q);
            return infinity();
        }
        F ppp = F::mul(pp_, pp);
        F qq = F::mul(p.x, pp);
        o.x = F::sub_sum3(rr, ppp, qq, qq);
        o.y = F::dot2(r_, F::sub(qq, o.x), F::neg(p.y), ppp);   // r*(qq - x3) - y1*ppp, one reduction
        o.zzz = F::mul(p.zzz, ppp);
        return o;
    }

    // The addition of the MSM accumulation loop in two halves, the sum written over p: p += q for p NOT infinity and q not null.
    // q's coordinates are read in madd_begin alone, so between the halves the caller can request the next point into q's own
    // registers, with four fifths of the addition in front of its first use.  madd_finish returns MADD_SUM (p holds the sum), or
    // MADD_SAME (p == q: the caller doubles q) / MADD_OPPOSITE (p == -q: the sum is infinity) with p left undefined -- neither needs
    // it, and ZZ3 can then be written over ZZ1 before it is tested.  The full compare of ZZ3 is reached only by lanes whose limb 0
    // is that of 0 or +-p (fields.cuh); the arithmetic is madd's, instruction for instruction.
    enum : int { MADD_SUM = 0, MADD_SAME = 1, MADD_OPPOSITE = 2 };
    struct MaddHalf {
        F u2, s2;
    };
    ZK_HD static MaddHalf madd_begin(const XYZZu& p, const AffineU<F>& q) {
        MaddHalf h;
        h.u2 = F::mul(q.x, p.zz);
        h.s2 = F::mul(q.y, p.zzz);
        return h;
    }
    ZK_HD static int madd_finish(XYZZu& p, const MaddHalf& h) {
        F pp_ = F::sub(h.u2, p.x);
        F r_ = F::sub(h.s2, p.y);
        F pp = F::sqr(pp_);
        F rr = F::sqr(r_);
        p.zz = F::mul(p.zz, pp);
        int how = MADD_SUM;
        if (p.zz.limb0_of_zero_mod()) {
            if (p.zz.is_zero_mod_reduced()) how = rr.is_zero_mod_reduced() ? MADD_SAME : MADD_OPPOSITE;
        }
        if (zk_apart(how == MADD_SUM)) {
            F ppp = F::mul(pp_, pp);
            F qq = F::mul(p.x, pp);
            p.x = F::sub_sum3(rr, ppp, qq, qq);
            p.y = F::dot2(r_, F::sub(qq, p.x), F::neg(p.y), ppp);   // r*(qq - x3) - y1*ppp, one reduction
            p.zzz = F::mul(p.zzz, ppp);
        }
        return how;
    }

    // this + q, both XYZZ; handles infinities, doubling and cancellation
    ZK_HD static XYZZu add(const XYZZu& p, const XYZZu& q) {
        if (p.is_inf()) return q;
        if (q.is_inf()) return p;
        F u1 = F::mul(p.x, q.zz);
        F u2 = F::mul(q.x, p.zz);
        F s1 = F::mul(p.y, q.zzz);
        F s2 = F::mul(q.y, p.zzz);
        F pp_ = F::sub(u2, u1);
        F r_ = F::sub(s2, s1);
        F pp = F::sqr(pp_);
        F rr = F::sqr(r_);
        XYZZu o;
        o.zz = F::mul(F::mul(p.zz, q.zz), pp);
        if (o.zz.is_zero_mod_reduced()) {
            if (rr.is_zero_mod_reduced()) return dbl(p);
            return infinity();
        }
        F ppp = F::mul(pp_, pp);
        F qq = F::mul(u1, pp);
        o.x = F::sub_sum3(rr, ppp, qq, qq);
        o.y = F::dot2(r_, F::sub(qq, o.x), F::neg(s1), ppp);
        o.zzz = F::mul(F::mul(p.zzz, q.zzz), ppp);
        return o;
    }

    ZK_HD static XYZZu neg(const XYZZu& p) {
        XYZZu r = p;
        r.y = F::neg(p.y);
        return r;
    }

    // affine normalisation of a finite point from i3 = 1 / ZZZ, a product (for a caller with a batched inversion: the key fold of
    // ipa.hip after block_inverse.cuh).  ZZ * i3 = 1 / Z.  Output coordinates are products (< 2p).
    ZK_HD void to_affine_given(const F& i3, AffineU<F>& out) const {
        F zi = F::mul(zz, i3);
        F zi2 = F::sqr(zi);
        out.x = F::mul(x, zi2);
        out.y = F::mul(y, i3);
    }
    // affine normalisation (one field inversion); returns false for infinity.  Output coordinates are products (< 2p).
    // The three products of to_affine_given stand here a second time: as a call of that member -- in any of the forms tried,
    // profiles/block_inverse/asm_digests.md -- the device code of msm_accumulate.hip's fixed-base kernel is scheduled differently, and
    // that unit's code is pinned (profiles/pmc_msm_accumulate.json).
    ZK_HD bool to_affine(AffineU<F>& out) const {
        if (is_inf()) {
            out.x = F::zero();
            out.y = F::zero();
            return false;
        }
        F i3 = F::inverse(zzz);
        F zi = F::mul(zz, i3);
        F zi2 = F::sqr(zi);
        out.x = F::mul(x, zi2);
        out.y = F::mul(y, i3);
        return true;
    }
};
