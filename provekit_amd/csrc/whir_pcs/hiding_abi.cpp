// hiding_abi.cpp -- libprovekit_whir_hiding.so: the C names of the hiding commitments' entry points (include/provekit_whir_hiding.h).
// The functions themselves are libprovekit_whir.so's (pcs.hpp: the scheme, the commitment and pkw::open_hiding in pcs.cpp over
// hiding.hip's stage kernel, pkw::io_pattern_hiding and pkw::verify_hiding in verify_host.cpp); that library and its two companions
// keep the export lists they had, so this third companion links the first and adds nothing but the names.  Nothing throws across.
#include "../../../include/provekit_whir_hiding.h"
#include "pcs.hpp"

extern "C" {

#ifndef PKW_HOST_ONLY  // the sanitizer build of the host verifier has no device half
int pkw_hiding_scheme_create(pk_ctx* ctx, const pk_whir_config* cfg, pkw_scheme** out) { return pkw::hiding_scheme_create(ctx, cfg, out); }

int pkw_commit_hiding(pkw_scheme* s, const uint64_t* const* d_evals, const uint8_t* rng_seed32, pkw_hiding_commitment** out) {
    return pkw::commit_hiding(s, d_evals, rng_seed32, out);
}

int pkw_hiding_commitment_root(const pkw_hiding_commitment* com, uint8_t root[32]) { return pkw::hiding_commitment_root(com, root); }

int pkw_hiding_commitment_destroy(pkw_hiding_commitment* com) { return pkw::hiding_commitment_destroy(com); }

int pkw_open_hiding(pkw_scheme* s, pkw_hiding_commitment* com, const uint64_t* points, unsigned q, uint64_t* evals_out, uint8_t* proof_out, size_t cap,
                    size_t* len) {
    return pkw::open_hiding(s, com, points, q, evals_out, proof_out, cap, len);
}
#endif

int pkw_io_pattern_hiding(const pk_whir_config* cfg, unsigned q, uint8_t* buf, size_t cap, size_t* len) {
    return pkw::io_pattern_hiding(cfg, q, buf, cap, len);
}

int pkw_verify_hiding(const pk_whir_config* cfg, const uint8_t* io_pattern, size_t io_pattern_len, int hash_version, const uint8_t* expected_root,
                      const uint64_t* points, unsigned q, const uint8_t* proof, size_t len, uint64_t* evals_out, pkv_result* result) {
    return pkw::verify_hiding(cfg, io_pattern, io_pattern_len, hash_version, expected_root, points, q, proof, len, evals_out, result);
}

}  // extern "C"
