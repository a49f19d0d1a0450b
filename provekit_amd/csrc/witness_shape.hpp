// witness_shape.hpp -- the sizes at which witness.hip changes path, in a header of their own so that the lab (tools/probes) reports
// them to the tests: a test that straddles a threshold reads it from the library and fails when a retune moves it.
#pragma once
#include <cstdint>

namespace pk {
namespace wb {
// a phase of at most NARROW items joins a run of consecutive narrow phases: one workgroup of NARROW lanes walks the run, a barrier
// between phases (wb_narrow_run_kernel); a wider phase is a launch of its own (wb_phase_kernel)
constexpr uint32_t NARROW = 1024;
// a Sum of more than SUM_HEAVY terms leaves the item list: a workgroup per SUM_CHUNK terms forms a partial sum, a workgroup per sum
// adds the partials
constexpr uint32_t SUM_HEAVY = 128, SUM_CHUNK = 1024;
// the variants of a work item (WbItem::op): items of one phase are sorted by it
constexpr uint32_t N_OPS = 16;
}  // namespace wb
}  // namespace pk
