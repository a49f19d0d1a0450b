// sparse_abi.cpp -- libprovekit_whir_sparse.so: the C names of the sparse weights' entry points (include/provekit_whir_sparse.h).  The
// functions themselves are libprovekit_whir.so's (pcs.hpp: pkw::sparse_sums, pkw::sparse_accumulate and pkw::sparse_evaluate in
// sparse.hip, pkw::open_sparse in pcs.cpp, pkw::verify_sparse in verify_host.cpp); that library and libprovekit_whir_linear.so keep
// the export lists they had, so this second companion links the first and adds nothing but the names.  Nothing throws across.
#include "../../../include/provekit_whir_sparse.h"
#include "pcs.hpp"

extern "C" {

#ifndef PKW_HOST_ONLY  // the sanitizer build of the host verifier has no device half
int pkw_sparse_sums(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index,
                    const uint64_t* d_value, unsigned l, uint64_t* out) {
    return pkw::sparse_sums(ctx, d_evals, batch, n_vars, offsets, d_index, d_value, l, out);
}

int pkw_sparse_accumulate(pk_ctx* ctx, uint64_t* d_table, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index, const uint64_t* d_value,
                          unsigned l, const uint64_t* scales) {
    return pkw::sparse_accumulate(ctx, d_table, n_vars, offsets, d_index, d_value, l, scales);
}

int pkw_sparse_evaluate(pk_ctx* ctx, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index, const uint64_t* d_value, unsigned l,
                        const uint64_t* point, uint64_t* out) {
    return pkw::sparse_evaluate(ctx, n_vars, offsets, d_index, d_value, l, point, out);
}

int pkw_open_sparse(pkw_scheme* s, const pkw_commitment* com, const uint64_t* points, unsigned q, const uint64_t* offsets, const uint32_t* d_index,
                    const uint64_t* d_value, const uint64_t* tags, unsigned l, uint64_t* evals_out, uint64_t* sums_out, uint8_t* proof_out, size_t cap,
                    size_t* len) {
    return pkw::open_sparse(s, com, points, q, offsets, d_index, d_value, tags, l, evals_out, sums_out, proof_out, cap, len);
}
#endif

int pkw_verify_sparse(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                      const uint64_t* points, unsigned q, const uint64_t* tags, const uint64_t* offsets, const uint32_t* index, const uint64_t* value,
                      unsigned l, const uint8_t* proof, size_t len, uint64_t* evals_out, uint64_t* sums_out, uint64_t* fold_point_out, uint64_t* deferred_out,
                      pkv_result* result) {
    return pkw::verify_sparse(cfg, io_pattern, io_pattern_len, hash_version, expected_root, points, q, tags, offsets, index, value, l, proof, len, evals_out,
                              sums_out, fold_point_out, deferred_out, result);
}

}  // extern "C"
