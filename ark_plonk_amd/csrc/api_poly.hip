// Pass-throughs of the C ABI: argument checks and the ctx guard in front of the NTT, field, grand-product, lookup, quotient and
// polynomial units.
#include "api_internal.h"
#include "domain.cuh"

// ------------------------------------------------------------------------------------------- a1
template <class C>
static int domain_new(uint64_t num_coeffs, zk_domain_info* out) {
    typedef typename C::Fr Fr;
    uint64_t size = 1;
    uint32_t lg = 0;
    while (size < num_coeffs) {
        size <<= 1;
        ++lg;
        if (lg > 63) return ZK_ERR_DOMAIN_TOO_LARGE;
    }
    if (!domain_log_ok<C>(lg)) return ZK_ERR_DOMAIN_TOO_LARGE;
    memset(out, 0, sizeof *out);
    out->size = size;
    out->log_size_of_group = lg;
    Fr root = domain_root<C>(lg);
    Fr gen = coset_gen<C>();
    Fr size_inv = Fr::inverse(Fr::from_u64(size));
    Fr root_inv = Fr::inverse(root);
    Fr gen_inv = Fr::inverse(gen);
    memcpy(out->size_inv, size_inv.v, 32);
    memcpy(out->group_gen, root.v, 32);
    memcpy(out->group_gen_inv, root_inv.v, 32);
    memcpy(out->generator, gen.v, 32);
    memcpy(out->generator_inv, gen_inv.v, 32);
    return ZK_OK;
}

extern "C" {

int zk_domain_new(int curve_id, uint64_t num_coeffs, zk_domain_info* out) {
    if (!out) return ZK_ERR_BAD_ARG;
    return zk_on_curve(curve_id, ZK_ERR_BAD_ARG, [&](auto cv) { return domain_new<decltype(cv)>(num_coeffs, out); });
}

// ---------------------------------------------------------------------------------------- a2-a5
int zk_ntt_dev(zk_ctx* c, int curve_id, int kind, uint32_t log_n, const void* d_in, size_t in_len, void* d_out) {
    if (!c || !d_out || (!d_in && in_len)) return ZK_ERR_BAD_ARG;
    if (log_n > 63) return ZK_ERR_DOMAIN_TOO_LARGE;
    Guard g(c);
    return ntt_run_dev(c, curve_id, kind, log_n, d_in, in_len, d_out);
}

int zk_ntt_batch_dev(zk_ctx* c, int curve_id, int kind, uint32_t log_n, uint32_t n_polys, const void* const* d_ins,
                     const size_t* in_lens, void* const* d_outs) {
    if (!c || (n_polys && (!d_ins || !in_lens || !d_outs))) return ZK_ERR_BAD_ARG;
    if (log_n > 63) return ZK_ERR_DOMAIN_TOO_LARGE;
    for (uint32_t i = 0; i < n_polys; ++i)
        if (!d_outs[i] || (!d_ins[i] && in_lens[i])) return ZK_ERR_BAD_ARG;
    for (uint32_t i = 0; i < n_polys; ++i)
        for (uint32_t j = 0; j < i; ++j)
            if (d_outs[i] == d_outs[j]) return ZK_ERR_BAD_ARG;     // two results in one buffer
    Guard g(c);
    return ntt_run_batch_dev(c, curve_id, kind, log_n, n_polys, d_ins, in_lens, d_outs);
}

int zk_ntt_prepare(zk_ctx* c, int curve_id, uint32_t log_n) {
    if (!c) return ZK_ERR_BAD_ARG;
    if (log_n > 63) return ZK_ERR_DOMAIN_TOO_LARGE;
    Guard g(c);
    return ntt_prepare(c, curve_id, log_n);
}

int zk_fr_from_mont_dev(zk_ctx* c, int curve_id, const void* d_in, size_t n, void* d_out) {
    if (!c || (n && (!d_in || !d_out))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return fr_convert_dev(c, curve_id, 0, d_in, n, d_out);
}
int zk_fr_to_mont_dev(zk_ctx* c, int curve_id, const void* d_in, size_t n, void* d_out) {
    if (!c || (n && (!d_in || !d_out))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return fr_convert_dev(c, curve_id, 1, d_in, n, d_out);
}
int zk_fr_mul_dev(zk_ctx* c, int curve_id, const void* d_a, const void* d_b, size_t n, void* d_out) {
    if (!c || (n && (!d_a || !d_b || !d_out))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return fr_mul_dev(c, curve_id, d_a, d_b, n, d_out);
}

int zk_lookup_query_dev(zk_ctx* c, int curve_id, size_t n, const void* d_q_lookup, size_t q_len, const void* const d_wires[4], const uint64_t* zeta_mont,
                        const void* d_table_compressed, void* d_out) {
    if (!c || !zeta_mont) return ZK_ERR_BAD_ARG;
    if (n && (!d_wires || !d_wires[0] || !d_wires[1] || !d_wires[2] || !d_wires[3] || !d_table_compressed || !d_out || (q_len && !d_q_lookup)))
        return ZK_ERR_BAD_ARG;
    Guard g(c);
    return lookup_query_dev(c, curve_id, n, d_q_lookup, q_len, d_wires, zeta_mont, d_table_compressed, d_out);
}

int zk_lookup_combine_split_dev(zk_ctx* c, int curve_id, const void* d_t, size_t n_t, const void* d_f, size_t n_f, void* d_h1, void* d_h2,
                                size_t* len_h1, size_t* len_h2) {
    if (!c || !len_h1 || !len_h2 || !zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if ((n_t && !d_t) || (n_f && !d_f) || ((n_t + n_f) && (!d_h1 || !d_h2))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return lookup_combine_split_dev(c, d_t, n_t, d_f, n_f, d_h1, d_h2, len_h1, len_h2);
}

int zk_poly_evaluate_dev(zk_ctx* c, int curve_id, uint32_t n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* points_mont,
                         uint64_t* out_mont) {
    if (!c || (n_polys && (!d_polys || !lens || !points_mont || !out_mont))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return poly_evaluate_dev(c, curve_id, n_polys, d_polys, lens, points_mont, out_mont);
}

int zk_poly_lincomb_dev(zk_ctx* c, int curve_id, uint32_t n_terms, const void* const* d_polys, const size_t* lens, const uint64_t* coeffs_mont,
                        void* d_out, size_t out_len) {
    if (!c || (n_terms && (!d_polys || !lens || !coeffs_mont)) || (out_len && !d_out)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return poly_lincomb_dev(c, curve_id, n_terms, d_polys, lens, coeffs_mont, d_out, out_len);
}

// ------------------------------------------------------------------------------------- utilities
int zk_g1_fixed_base_batch_dev(zk_ctx* c, int curve_id, const void* d_scalars, size_t n, void* d_out_xy) {
    if (!c || (n && (!d_scalars || !d_out_xy))) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return msm_ops(curve_id)->fixed_base(c, d_scalars, n, d_out_xy);
}

// ------------------------------------------------------------------------------ N2: grand products
int zk_perm_product_dev(zk_ctx* c, int curve_id, uint32_t log_n, const void* const* d_wires, const void* const* d_sigmas,
                        const uint64_t* beta_mont, const uint64_t* gamma_mont, void* d_out, uint64_t* last_mont) {
    if (!c || !d_wires || !d_sigmas || !beta_mont || !gamma_mont || !d_out) return ZK_ERR_BAD_ARG;
    if (!zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (log_n > 32) return ZK_ERR_DOMAIN_TOO_LARGE;
    for (int k = 0; k < 4; ++k)
        if (!d_wires[k] || !d_sigmas[k]) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return perm_product_dev(c, curve_id, log_n, d_wires, d_sigmas, beta_mont, gamma_mont, d_out, last_mont);
}

int zk_lookup_product_dev(zk_ctx* c, int curve_id, size_t n, const void* d_f, const void* d_t, const void* d_h1, const void* d_h2,
                          const uint64_t* delta_mont, const uint64_t* epsilon_mont, void* d_out, uint64_t* last_mont) {
    if (!c || !n || !d_f || !d_t || !d_h1 || !d_h2 || !delta_mont || !epsilon_mont || !d_out) return ZK_ERR_BAD_ARG;
    if (!zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    Guard g(c);
    return lookup_product_dev(c, curve_id, n, d_f, d_t, d_h1, d_h2, delta_mont, epsilon_mont, d_out, last_mont);
}

// ------------------------------------------------------------------------------ N1: quotient
int zk_quotient_evals_dev(zk_ctx* c, int curve_id, uint32_t log_n, const zk_quotient_args* args, void* d_out) {
    if (!c || !args || !d_out) return ZK_ERR_BAD_ARG;
    if (!zk_curve_ok(curve_id)) return ZK_ERR_BAD_ARG;
    if (log_n > 30) return ZK_ERR_DOMAIN_TOO_LARGE;
    Guard g(c);
    return quotient_evals_dev(c, curve_id, log_n, args, d_out);
}

// ------------------------------------------------------------------------------ device self-test
int zk_selftest_quad_dev(zk_ctx* c, int curve_id, uint32_t n_quads, uint32_t* mismatches, uint32_t* case_mask) {
    if (!c || !mismatches) return ZK_ERR_BAD_ARG;
    Guard g(c);
    uint32_t out[2] = {0, 0};
    int rc = quad_selftest_dev(c, curve_id, n_quads, out);
    if (rc) return rc;
    *mismatches = out[0];
    if (case_mask) *case_mask = out[1];
    return ZK_OK;
}

}  // extern "C"
