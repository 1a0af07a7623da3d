// Device storage of base-field elements and points in the MSM's internal form: what the MSM units (through msm_common.cuh) and the
// folded key of the inner-product argument (ipa.hip) read and write.  Nothing here depends on the curve a unit is built for.
#pragma once
#include "ecu.cuh"

namespace zkmsm {

// ---- device storage of a field element (Fs, fields.cuh): NL limbs padded to a multiple of 4 words (16-byte vector access)
template <class F>
struct Store {
    static constexpr int U4 = (F::NL + 3) / 4;      // uint4 per field element
    static constexpr int WORDS = 4 * U4;
    static constexpr size_t POINT_BYTES = (size_t)4 * WORDS * 4;    // bytes of one stored XYZZ point
};
template <class F>
ZK_D F ld_fu(const uint4* q) {
    F r;
#pragma unroll
    for (int i = 0; i < Store<F>::U4; ++i) {
        uint4 a = q[i];
        if (4 * i + 0 < F::NL) r.v[4 * i + 0] = a.x;
        if (4 * i + 1 < F::NL) r.v[4 * i + 1] = a.y;
        if (4 * i + 2 < F::NL) r.v[4 * i + 2] = a.z;
        if (4 * i + 3 < F::NL) r.v[4 * i + 3] = a.w;
    }
    return r;
}
template <class F>
ZK_D void st_fu(uint4* q, const F& r) {
#pragma unroll
    for (int i = 0; i < Store<F>::U4; ++i) {
        uint4 a;
        a.x = 4 * i + 0 < F::NL ? r.v[4 * i + 0] : 0u;
        a.y = 4 * i + 1 < F::NL ? r.v[4 * i + 1] : 0u;
        a.z = 4 * i + 2 < F::NL ? r.v[4 * i + 2] : 0u;
        a.w = 4 * i + 3 < F::NL ? r.v[4 * i + 3] : 0u;
        q[i] = a;
    }
}
template <class F>
ZK_D AffineU<F> ld_affine(const void* bases, uint64_t idx) {
    const uint4* q = reinterpret_cast<const uint4*>(bases) + idx * (2 * Store<F>::U4);
    AffineU<F> p;
    p.x = ld_fu<F>(q);
    p.y = ld_fu<F>(q + Store<F>::U4);
    return p;
}
template <class F>
ZK_D XYZZu<F> ld_xyzz(const void* arr, uint64_t idx) {
    const uint4* q = reinterpret_cast<const uint4*>(arr) + idx * (4 * Store<F>::U4);
    XYZZu<F> p;
    p.x = ld_fu<F>(q);
    p.y = ld_fu<F>(q + Store<F>::U4);
    p.zz = ld_fu<F>(q + 2 * Store<F>::U4);
    p.zzz = ld_fu<F>(q + 3 * Store<F>::U4);
    return p;
}
template <class F>
ZK_D void st_xyzz(void* arr, uint64_t idx, const XYZZu<F>& p) {
    uint4* q = reinterpret_cast<uint4*>(arr) + idx * (4 * Store<F>::U4);
    st_fu<F>(q, p.x);
    st_fu<F>(q + Store<F>::U4, p.y);
    st_fu<F>(q + 2 * Store<F>::U4, p.zz);
    st_fu<F>(q + 3 * Store<F>::U4, p.zzz);
}

// one coordinate (role 0..3 = X, Y, ZZ, ZZZ) of a stored XYZZ point: the quad-cooperative kernels (ecq.cuh)
template <class F>
ZK_D F ld_coord(const void* arr, uint64_t idx, uint32_t role) {
    return ld_fu<F>(reinterpret_cast<const uint4*>(arr) + idx * (4 * Store<F>::U4) + role * Store<F>::U4);
}
template <class F>
ZK_D void st_coord(void* arr, uint64_t idx, uint32_t role, const F& c) {
    st_fu<F>(reinterpret_cast<uint4*>(arr) + idx * (4 * Store<F>::U4) + role * Store<F>::U4, c);
}

}  // namespace zkmsm
