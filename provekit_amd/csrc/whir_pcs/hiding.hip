// hiding.hip -- the stage of a HIDING commitment (include/provekit_whir_hiding.h): the B masks and g drawn from the proof RNG in ONE
// launch, straight into the upper halves of the extended tables f^_b = [f_b || mask_b] and into g.
//
// The index space is the concatenation of the B mask halves (2^n elements each) and g (2^(n+1)), walked in PAIRS as rng.hip's
// random_fe_kernel walks one draw: a lane is a (pair, attempt) state machine that runs one ChaCha block per iteration, whichever
// pair and attempt it is at, so a rejected candidate (probability 0.244) costs its lane one more iteration and never holds a
// wavefront on one pair.  A pair takes its stream word and its local index j from the segment it lies in -- segment sizes are even
// for n >= 1, so no pair straddles two -- and the block is (counter j, nonce {stream, attempt}): the bits depend on (key, stream,
// index) only, never on the launch shape.  The cipher block and the accept rule are rng_core.hpp's, shared with rng.hip.
// A lane stores an accepted element as two 16-byte vector stores (fe_store); lane t's pair is the 64 bytes after lane t - 1's.
// No LDS, no atomics.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../rng_core.hpp"
#include "hiding.hpp"

using namespace pk;

namespace pkw {

namespace {

struct HidingTables {
    fe* t[HIDING_MAX_POLYS + 1];  // f^_0 .. f^_{B-1}, then g (slot B)
};

__global__ __launch_bounds__(HIDING_THREADS) void hiding_fill_kernel(HidingTables a, unsigned polys, unsigned n, RngKey key) {
    const size_t seg = (size_t)1 << (n - 1);  // the pairs of one mask half; g has two segments' worth
    const size_t pairs = (size_t)(polys + 2) * seg, stride = (size_t)gridDim.x * HIDING_THREADS;
    size_t t = (size_t)blockIdx.x * HIDING_THREADS + threadIdx.x;
    u32 attempt = 0;
    bool done0 = false, done1 = false;
    while (t < pairs) {
        const unsigned at = (unsigned)(t >> (n - 1));
        const unsigned s = at < polys ? at : polys;  // the segment: mask s, or g
        const size_t j = t - (size_t)s * seg;        // the pair inside its stream
        const u32 stream = s < polys ? PKW_RNG_MASK0 + s : PKW_RNG_G;
        fe* base = a.t[0];
#pragma unroll
        for (unsigned i = 1; i <= HIDING_MAX_POLYS; i++) base = s == i ? a.t[i] : base;
        fe* out = base + (s < polys ? 2 * seg : 0) + 2 * j;  // a mask is the upper half of its table
        u32 blk[16];
        chacha_block(key, (u64)j, stream, attempt, PK_RNG_ROUNDS, blk);
        fe x;
        if (!done0 && rng_candidate(blk, 0, x)) {
            fe_store(out, x);
            done0 = true;
        }
        if (!done1 && rng_candidate(blk, 1, x)) {
            fe_store(out + 1, x);
            done1 = true;
        }
        if (done0 && done1) {
            t += stride;
            attempt = 0;
            done0 = done1 = false;
        } else {
            attempt++;
        }
    }
}

}  // namespace

size_t hiding_pairs(unsigned polys, unsigned n) { return (size_t)(polys + 2) << (n - 1); }

unsigned hiding_grid(unsigned polys, unsigned n) {
    const size_t per_wg = (size_t)HIDING_THREADS * HIDING_PAIRS_PER_LANE;
    const size_t blocks = (hiding_pairs(polys, n) + per_wg - 1) / per_wg;
    return (unsigned)(blocks ? blocks : 1);
}

int hiding_fill_launch(hipStream_t stream, uint64_t* const* d_tables, unsigned polys, unsigned n, const uint8_t key32[32], unsigned grid, hipError_t* launch_error) {
    if (!d_tables || !key32 || polys < 1 || polys > HIDING_MAX_POLYS || n < 1 || n > 29) return PK_ERR_BAD_ARG;
    HidingTables a{};
    for (unsigned b = 0; b <= polys; b++) {
        if (!d_tables[b]) return PK_ERR_BAD_ARG;
        a.t[b] = reinterpret_cast<fe*>(d_tables[b]);
    }
    RngKey key;
    memcpy(key.k, key32, 32);
    hiding_fill_kernel<<<grid ? grid : hiding_grid(polys, n), HIDING_THREADS, 0, stream>>>(a, polys, n, key);
    const hipError_t e = hipGetLastError();
    if (launch_error) *launch_error = e;
    return e == hipSuccess ? PK_OK : PK_ERR_HIP;
}

}  // namespace pkw
