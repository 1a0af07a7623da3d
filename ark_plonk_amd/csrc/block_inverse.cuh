// 1 / z for every lane of a workgroup with ONE field inversion (Montgomery's trick): inclusive prefix and suffix products of z over
// the workgroup in LDS (Hillis-Steele, log2(W) steps each), one Fermat inversion of the total in lane 0, and
// 1 / z_t = prefix_{t-1} * suffix_{t+1} / total.  The one definition: the gadget witness kernels (gadget_witness.hip, W = 256, Fr),
// the key fold of the inner-product argument (ipa.hip, W = 128, the signed-limb Fq) and the verifier's scalars (verify.hip, W = 64,
// computed in Called<Fr> and stored as Fr) all call it.
//
// The contract:
//   * z is non-zero in every one of the W lanes (a lane with nothing to invert passes one());
//   * all W lanes of the workgroup call it, and blockDim.x == W;
//   * it ends by READING lds, so a caller that calls it again on the same lds puts its own barrier between the calls.
#pragma once
#include "zk_common.h"

// S: the type the products are stored as.  Declared __shared__ once in every kernel that calls block_inverse (alone or as a member
// of the kernel's LDS struct).  Aligned for 128-bit LDS access where S is a whole number of such words (Fr: 32 bytes); the 52- and
// 36-byte signed-limb Fq keeps its own alignment, so the struct takes no more LDS than its arrays.
template <class S, uint32_t W>
struct alignas(sizeof(S) % 16 == 0 ? 16 : alignof(S)) BlockInverseLds {
    S pre[W], suf[W], inv_total;
};
// F: the type the products are computed in: S itself, or a type derived from S that converts from it (verify.hip's Called<Fr>)
template <class F, class S, uint32_t W>
ZK_D F block_inverse(const F& z, BlockInverseLds<S, W>& lds) {
    S *const pre = lds.pre, *const suf = lds.suf, *const inv_total = &lds.inv_total;
    const uint32_t t = threadIdx.x;
    F p = z, s = z;
    pre[t] = p;
    suf[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < W; d <<= 1) {
        const F pl = t >= d ? pre[t - d] : S::one();
        const F sr = t + d < W ? suf[t + d] : S::one();
        __syncthreads();
        if (t >= d) p = F::mul(p, pl);
        if (t + d < W) s = F::mul(s, sr);
        pre[t] = p;
        suf[t] = s;
        __syncthreads();
    }
    if (t == 0) *inv_total = F::inverse(pre[W - 1]);
    __syncthreads();
    F zi = *inv_total;
    if (t > 0) zi = F::mul(zi, pre[t - 1]);
    if (t + 1 < W) zi = F::mul(zi, suf[t + 1]);
    return zi;
}
