// whir_sparse.hip -- libprovekit_whir.so's sparse-weight code (csrc/whir_pcs/sparse.hip, sparse.hpp) where the C ABI does not reach:
// the sums kernel on a grid of the caller's choice (the result must not depend on it; a small grid reaches the stride loop at a
// small size), and two pieces of arithmetic run on the HOST for the CPU suite: the lane's accumulate / flush / result code of the
// sums kernel, and the chunked eq tables the verifier evaluates a sparse weight with.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pk_probes.h"
#include "whir_pcs/sparse.hpp"

extern "C" {

unsigned pk_probe_whir_sparse_threads(void) { return pkw::SPARSE_THREADS; }
unsigned pk_probe_whir_sparse_chunk_bits(void) { return pkw::SPARSE_CHUNK_BITS; }
unsigned pk_probe_whir_sparse_grid(unsigned n_vars, size_t nnz, unsigned steps) { return pkw::sparse_grid(n_vars, nnz, steps); }

// pkw_sparse_sums with the grid as a parameter (0: the library's own); the lists are validated like there
int pk_probe_whir_sparse_sums(pk_ctx* ctx, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const uint64_t* offsets, const uint32_t* d_index,
                              const uint64_t* d_value, unsigned l, unsigned grid, uint64_t* out) {
    std::string why;
    if (!ctx || !d_evals || !offsets || !out || batch < 1 || batch > pkw::SPARSE_MAX_BATCH || n_vars > 30 || l < 1 || l > PKW_MAX_WEIGHTS) return PK_ERR_BAD_ARG;
    if (!pkw::sparse_offsets_ok(offsets, l, n_vars, why) || (offsets[l] && (!d_index || !d_value))) return PK_ERR_BAD_ARG;
    const size_t part = pkw::sparse_partial_fes(batch, n_vars), res = (size_t)batch * l;
    void* d = nullptr;
    int rc = pk_malloc(ctx, 32 * (part + res + 1), &d);
    if (rc) return rc;
    uint64_t* d_part = (uint64_t*)d;
    uint64_t* d_res = d_part + 4 * part;
    const pkw::SparseWeights w{offsets, d_index, d_value, l};
    size_t bad = 0;
    uint32_t at = 0, prev = 0;
    rc = pk_ctx_sync(ctx);
    if (!rc) rc = pkw::sparse_validate(ctx, nullptr, w, n_vars, d_res + 4 * res, &bad, &at, &prev);
    if (!rc && bad != ~(size_t)0) rc = PK_ERR_BAD_ARG;
    if (!rc) rc = pkw::sparse_sums_launch(nullptr, d_evals, batch, n_vars, w, d_part, d_res, grid);
    if (!rc && hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    if (!rc) rc = pk_memcpy_d2h(ctx, out, d_res, 32 * res);
    pk_free(ctx, d);
    return rc;
}

// the sums kernel's lanes on the host: `terms` entries, f = 4 polynomials' gathered elements [4][terms], w = the entries' values
// [terms]; out = 4 elements.  As on the device, four polynomials are two slices of SPARSE_TILE_B = 2
int pk_probe_sparse_tile_host(const uint64_t* f, const uint64_t* w, unsigned terms, uint64_t* out) {
    if (!f || !w || !out) return PK_ERR_BAD_ARG;
    constexpr int B = pkw::SPARSE_TILE_B;
    for (unsigned b0 = 0; b0 < pkw::SPARSE_MAX_BATCH; b0 += B) {
        pkw::SparseTile<B> t;
        pkw::wsum_tile_init(t);
        for (unsigned s = 0; s < terms; s++) {
            pk::fe fv[B], v;
            for (int u = 0; u < B; u++) memcpy(fv[u].v, f + 4 * ((size_t)(b0 + u) * terms + s), 32);
            memcpy(v.v, w + 4 * (size_t)s, 32);
            pkw::sparse_tile_step(t, fv, v);
        }
        for (int u = 0; u < B; u++) {
            const pk::fe r = pkw::wsum_tile_result(t, u, 0);
            memcpy(out + 4 * (b0 + u), r.v, 32);
        }
    }
    return PK_OK;
}

// out = sum_k value[k] * eq(index[k], point) by the host verifier's chunked tables; every index < 2^n_vars (checked)
int pk_probe_sparse_eq_host(unsigned n_vars, const uint64_t* point, const uint32_t* index, const uint64_t* value, size_t nnz, uint64_t* out) {
    if (n_vars > 30 || (n_vars && !point) || (nnz && (!index || !value)) || !out) return PK_ERR_BAD_ARG;
    for (size_t k = 0; k < nnz; k++)
        if (((uint64_t)index[k] >> n_vars) != 0) return PK_ERR_BAD_ARG;
    std::vector<pk::fe> pt(n_vars ? n_vars : 1);
    for (unsigned j = 0; j < n_vars; j++) pt[j] = pk::h_load(point + 4 * (size_t)j);
    const pkw::SparseEqTables eq(pt.data(), n_vars);
    pk::h_store(out, eq.weight_at(index, value, nnz));
    return PK_OK;
}

}  // extern "C"
