// r1cs.hip -- csrc/r1cs.hip's thresholds (csrc/r1cs_shape.hpp), the two entry points of it that only the sharded prover calls
// (csrc/internal.hpp: witness_bounds_strided, external_row_range), and the grouped dot product every R1CS line goes through
// (csrc/fe29.hpp dot29) run on the HOST, for tests/r1cs_edge_cases.py, tests/test_r1cs_edge_cases_host.py and
// tests/test_gpu_r1cs_edges.py.
#include <hip/hip_runtime.h>

#include <cstring>

#include "internal.hpp"
#include "fe29.hpp"
#include "reduce.hpp"
#include "pk_probes.h"
#include "r1cs_shape.hpp"

extern "C" {

unsigned pk_probe_r1cs_heavy_degree(void) { return pk::r1cs_shape::HEAVY_DEGREE; }
unsigned pk_probe_r1cs_heavy_chunk(void) { return pk::r1cs_shape::HEAVY_CHUNK; }
unsigned pk_probe_dot29_group(void) { return (unsigned)pk::DOT29_GROUP; }
unsigned pk_probe_reduction_threads(void) { return (unsigned)pk::RED_THREADS; }

int pk_probe_r1cs_witness_bounds_strided(pk_ctx* ctx, const pk_r1cs* r, const uint64_t* d_z, unsigned m0, unsigned stride, unsigned offset, uint64_t* d_a,
                                         uint64_t* d_b, uint64_t* d_c) {
    PK_ENTER(ctx);
    return pk::witness_bounds_strided(ctx, r, d_z, m0, stride, offset, d_a, d_b, d_c);
}
int pk_probe_r1cs_external_row_range(pk_ctx* ctx, const pk_r1cs* r, const uint64_t* d_eq, size_t first, size_t last, uint64_t* d_out) {
    PK_ENTER(ctx);
    return pk::external_row_range(ctx, r, d_eq, first, last, d_out);
}

// the loop of sparse_row_dot on the host: out = sum_t a[t] * b[t] * 2^-256 mod p, a = the first factors (the interned values' place)
int pk_probe_dot29_host(const uint64_t* a, const uint64_t* b, unsigned terms, uint64_t* out) {
    if (!out || (terms && (!a || !b))) return PK_ERR_BAD_ARG;
    pk::dot29 d;
    pk::dot29_init(d);
    for (unsigned t = 0; t < terms; t++) {
        pk::fe x, y;
        memcpy(x.v, a + 4 * (size_t)t, 32);
        memcpy(y.v, b + 4 * (size_t)t, 32);
        pk::dot29_add(d, pk::unpack29<0>(x), pk::unpack29<5>(y));
    }
    const pk::fe s = pk::dot29_result(d);
    memcpy(out, s.v, 32);
    return PK_OK;
}

}  // extern "C"
