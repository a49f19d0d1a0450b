// linear_abi.cpp -- libprovekit_whir_linear.so: the C names of the linear statement's entry points (include/provekit_whir_linear.h).
// The functions themselves are libprovekit_whir.so's (pcs.hpp: pkw::open_linear in pcs.cpp, pkw::verify_linear and
// pkw::io_pattern_linear in verify_host.cpp, pkw::weighted_sums in linear.hip); that library keeps the export list it had, so the
// additive C ABI is this companion, which links it and adds nothing but the names.  Nothing throws across: the callees catch.
#include "pcs.hpp"

extern "C" {

#ifndef PKW_HOST_ONLY  // the sanitizer build of the host verifier has no device half
int pkw_weighted_sums(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* const* d_weights, unsigned l,
                      uint64_t* out) {
    return pkw::weighted_sums(ctx, d_evals, batch, n_vars, d_weights, l, out);
}

int pkw_open_linear(pkw_scheme* s, const pkw_commitment* com, const uint64_t* points, unsigned q, const uint64_t* const* d_weights, const uint64_t* tags,
                    unsigned l, uint64_t* evals_out, uint64_t* sums_out, uint8_t* proof_out, size_t cap, size_t* len) {
    return pkw::open_linear(s, com, points, q, d_weights, tags, l, evals_out, sums_out, proof_out, cap, len);
}
#endif

int pkw_io_pattern_linear(const pk_whir_config* cfg, unsigned q, unsigned l, uint8_t* buf, size_t cap, size_t* len) {
    return pkw::io_pattern_linear(cfg, q, l, buf, cap, len);
}

int pkw_verify_linear(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                      const uint64_t* points, unsigned q, const uint64_t* tags, const uint64_t* const* weights, unsigned l, const uint8_t* proof, size_t len,
                      uint64_t* evals_out, uint64_t* sums_out, uint64_t* fold_point_out, uint64_t* deferred_out, unsigned* unchecked_out,
                      pkv_result* result) {
    return pkw::verify_linear(cfg, io_pattern, io_pattern_len, hash_version, expected_root, points, q, tags, weights, l, proof, len, evals_out, sums_out,
                              fold_point_out, deferred_out, unchecked_out, result);
}

}  // extern "C"
