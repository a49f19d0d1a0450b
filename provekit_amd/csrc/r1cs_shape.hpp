// r1cs_shape.hpp -- the sizes at which r1cs.hip changes path, in a header of their own so that the lab (tools/probes) reports them to
// the tests: a test that straddles a threshold reads it from the library and fails when a retune moves it.
#pragma once
#include <cstdint>

namespace pk {
namespace r1cs_shape {
// a line (a row, or a column of the CSC copy) of more than HEAVY_DEGREE entries is summed by workgroups before the gather runs
// (heavy_dot_kernel / heavy_sum_kernel), HEAVY_CHUNK entries per workgroup; a shorter line is walked by the gather's own lane
constexpr uint32_t HEAVY_DEGREE = 64;
constexpr uint32_t HEAVY_CHUNK = 2048;
}  // namespace r1cs_shape
}  // namespace pk
