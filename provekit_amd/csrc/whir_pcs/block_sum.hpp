// block_sum.hpp -- the workgroup reduction the kernels of libprovekit_whir.so end in (evaluate.hip, linear.hip).  Device code.
#pragma once
#include "../fe29.hpp"

namespace pkw {

// sum of `v` over the workgroup's 256 lanes; valid in lane 0.  lds: 4 elements of its own
__device__ __forceinline__ pk::fe block_sum(pk::fe v, pk::fe* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pk::fe o;
#pragma unroll
        for (int k = 0; k < 8; k++) o.v[k] = __shfl_down(v.v[k], off, 64);
        v = pk::fe_add(v, o);
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = pk::fe_add(pk::fe_add(lds[0], lds[1]), pk::fe_add(lds[2], lds[3]));
    return v;
}

}  // namespace pkw
