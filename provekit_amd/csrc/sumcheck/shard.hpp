// shard.hpp -- which rank of a device set owns which table index of a sharded product sumcheck (include/provekit_sumcheck_sharded.h),
// stated once: round.hip's sharded kernels, the sharded prover and pkss_plan are compiled from these functions.
//
// Rounds bind the most significant index bit first, so the low index bits outlive every fold.  With G = 2^g ranks and chunks of
// 2^c = 256 elements (8 KiB contiguous: one workgroup's sweep, fully coalesced), rank r owns the indices x whose bits [c, c + g)
// spell r.  Its compacted index drops those bits:  y = (x >> (c + g)) << c | (x & (2^c - 1)).  While the bit a round binds lies
// above them (len / 2 >= 2^(c + g)) the partner x + len/2 of an owned x is owned too and compacts to y + (len / G) / 2: a rank's
// compacted table is an ordinary sumcheck table of length len / G, and the rank runs its rounds on it alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../../include/provekit_sumcheck_sharded.h"

namespace pkss {

constexpr unsigned C = PKSS_CHUNK_LOG2;

__host__ __device__ inline unsigned owner(size_t x, unsigned g) { return (unsigned)(x >> C) & ((1u << g) - 1); }
__host__ __device__ inline size_t compact(size_t x, unsigned g) { return ((x >> (C + g)) << C) | (x & (((size_t)1 << C) - 1)); }
// the index rank r's compacted y stands for
__host__ __device__ inline size_t expand(size_t y, unsigned g, unsigned r) { return ((y >> C) << (C + g)) | ((size_t)r << C) | (y & (((size_t)1 << C) - 1)); }
// round i of n binds bit n - 1 - i; it is sharded iff that bit lies above the rank bits
__host__ __device__ inline bool round_is_sharded(unsigned n, unsigned i, unsigned g) { return i < n && n - 1 - i >= C + g; }
// S: rounds 0 .. S-1 are sharded, S .. n-1 replicated
__host__ __device__ inline unsigned sharded_rounds(unsigned n, unsigned g) { return n > C + g ? n - C - g : 0; }
// the global length of the tables when the ranks hand over to the replicated rounds (entering round S, not yet folded by r_{S-1})
// a rank holds two chunks of each then (y < 2^(c+1): its lower-half chunk, then its upper-half chunk), element y at expand(y, g, r)
__host__ __device__ inline size_t handover_len(unsigned g) { return (size_t)1 << (C + g + 1); }

}  // namespace pkss
