// witness.hip -- csrc/witness.hip's thresholds and the shape of a levelled builder list, for tests that aim at the sizes where the
// solver changes path (tests/witness_edge_cases.py): host only, no device is touched.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "internal.hpp"
#include "pk_probes.h"
#include "witness_shape.hpp"

extern "C" {

unsigned pk_probe_witness_narrow(void) { return pk::wb::NARROW; }
unsigned pk_probe_witness_sum_heavy(void) { return pk::wb::SUM_HEAVY; }
unsigned pk_probe_witness_sum_chunk(void) { return pk::wb::SUM_CHUNK; }
unsigned pk_probe_witness_n_ops(void) { return pk::wb::N_OPS; }

// *n_phases = the phases of the levelled list (two per level).  With cap >= *n_phases: widths[ph] = its items, op_counts[ph * n_ops
// + op] = its items of variant op, blocks_before[ph] = the Spice blocks and long sums that run right before it.  Any of the three
// may be null.  A list build_program refuses: PK_ERR_BAD_ARG with its message in err.
int pk_probe_witness_phases(const uint8_t* bytes, size_t len, uint32_t* widths, uint32_t* op_counts, uint32_t* blocks_before, size_t cap, size_t* n_phases,
                            char* err, size_t err_cap) {
    if (!bytes || !n_phases) return PK_ERR_BAD_ARG;
    std::vector<uint32_t> w, ops, blocks;
    std::string why;
    const int rc = pk::witness_phase_shape(bytes, len, w, ops, blocks, why);
    if (rc) {
        if (err && err_cap) snprintf(err, err_cap, "%s", why.c_str());
        return rc;
    }
    *n_phases = w.size();
    if (cap < w.size()) return PK_OK;
    if (widths && !w.empty()) memcpy(widths, w.data(), 4 * w.size());
    if (op_counts && !ops.empty()) memcpy(op_counts, ops.data(), 4 * ops.size());
    if (blocks_before && !blocks.empty()) memcpy(blocks_before, blocks.data(), 4 * blocks.size());
    return PK_OK;
}

}  // extern "C"
