// bitwise.hip -- libprovekit_bitwise.so where its C ABI does not reach.  Its decomposition pass by itself over tables the caller holds,
// with the grid the library's rule would choose itself, and its device time, so that tools/bitwise_bench.py can time the hot pass alone.
// And a prover's knob and profile (csrc/bitwise/prover.hpp): the grid of every kernel of its calls, and where its last calls' time went.
#include <hip/hip_runtime.h>

#include "pk_probes.h"
#include "bitwise/prover.hpp"

extern "C" {

int pk_probe_bitwise_decompose(pk_ctx* ctx, unsigned n, unsigned op, unsigned d, unsigned L, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, int c_given,
                               uint64_t* const* d_digits, uint32_t* d_counts, unsigned long long* d_bad, uint64_t* d_m, unsigned grid, float* ms) {
    if (!ctx || !d_digits) return PK_ERR_BAD_ARG;
    const pkb_statement st{n, op, d, L, 0};
    std::string why;
    if (!pkb::statement_ok(&st, why)) return PK_ERR_BAD_ARG;
    int rc = pk_ctx_sync(ctx);  // also selects the context's device
    if (rc) return rc;
    hipEvent_t ev[2];
    for (hipEvent_t& e : ev)
        if (hipEventCreate(&e) != hipSuccess) return PK_ERR_HIP;
    (void)hipEventRecord(ev[0], nullptr);
    rc = pkb::decompose_launch(nullptr, n, op, d, L, d_a, d_b, d_c, c_given != 0, d_digits, d_counts, d_bad, d_m, grid);
    (void)hipEventRecord(ev[1], nullptr);
    if (hipStreamSynchronize(nullptr) != hipSuccess) rc = PK_ERR_HIP;
    float t_ms = 0;
    if (!rc && hipEventElapsedTime(&t_ms, ev[0], ev[1]) != hipSuccess) rc = PK_ERR_HIP;
    if (ms) *ms = t_ms;
    for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
    return rc;
}

int pk_probe_bitwise_set_grid(pkb_prover* p, unsigned grid) {
    if (!p || grid > PKB_MAX_GRID) return PK_ERR_BAD_ARG;
    p->grid = grid;
    return PK_OK;
}

int pk_probe_bitwise_profile(const pkb_prover* p, double* decompose_ms, double* lookup_ms) {
    if (!p || !decompose_ms || !lookup_ms) return PK_ERR_BAD_ARG;
    *decompose_ms = p->prof.decompose_ms, *lookup_ms = p->prof.lookup_ms;
    return PK_OK;
}

// the workgroups the library's rule gives each kernel at a statement: decompose, table, m
int pk_probe_bitwise_grids(unsigned n, unsigned op, unsigned d, unsigned L, unsigned* grids3) {
    const pkb_statement st{n, op, d, L, 0};
    std::string why;
    if (!grids3 || !pkb::statement_ok(&st, why)) return PK_ERR_BAD_ARG;
    grids3[0] = pkb::rows_grid((size_t)1 << n, pkb::DECOMPOSE_ITEMS);
    grids3[1] = grids3[2] = pkb::rows_grid((size_t)1 << (2 * d), pkb::PLAIN_ITEMS);
    return PK_OK;
}

unsigned pk_probe_bitwise_decompose_items(void) { return pkb::DECOMPOSE_ITEMS; }

}  // extern "C"
