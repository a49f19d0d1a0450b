// rng_core.hpp -- the proof RNG's cipher block and accept rule, stated once for every kernel that draws from it: rng.hip's
// (pk_prove's blinding draws, the witness fill), mle.hip's (pk_prove's mask and g, drawn inside the first to_coeffs sweep of the
// tables they fill) and whir_pcs/hiding.hip's (the masks and g of a hiding commitment).
//
// The ChaCha block function (RFC 8439 quarter rounds and state layout: words 12, 13 = counter, 14, 15 = nonce), PK_RNG_ROUNDS
// rounds.  Elements 2j and 2j+1 of draw `stream` share the blocks (counter = j, nonce = {stream, attempt}): a block holds two
// 254-bit candidates, the first for element 2j, the second for 2j+1, each accepted iff < p (what ark-ff's Fp::rand does, so every
// element is uniform on [0, p)); an element whose candidate was rejected takes its candidate of the next attempt.  The accepted
// word is stored as it is.  Stream numbers: internal.hpp's RNG_* for the draws of one proof, PKW_RNG_* below for a commitment's.
#pragma once
#include "fe.hpp"

namespace pk {

struct RngKey {
    uint32_t k[8];
};

// the draws of one hiding commitment (whir_pcs/hiding.hip): mask_b takes PKW_RNG_MASK0 + b, b < 3.  Clear of internal.hpp's RNG_*
// for tidiness only: a commitment's key is never a proof's key
enum { PKW_RNG_MASK0 = 16, PKW_RNG_G = 24 };

constexpr int PK_RNG_ROUNDS = 12;
#define PK_QR(a, b, c, d)                    \
    a += b; d ^= a; d = (d << 16) | (d >> 16); \
    c += d; b ^= c; b = (b << 12) | (b >> 20); \
    a += b; d ^= a; d = (d << 8) | (d >> 24);  \
    c += d; b ^= c; b = (b << 7) | (b >> 25)
__host__ __device__ __forceinline__ void chacha_block(const RngKey& key, u64 counter, u32 n0, u32 n1, int rounds, u32 (&out)[16]) {
    u32 s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                 key.k[4],    key.k[5],    key.k[6],    key.k[7],    (u32)counter, (u32)(counter >> 32), n0, n1};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll 1
    for (int r = 0; r < rounds / 2; r++) {
        PK_QR(x[0], x[4], x[8], x[12]);
        PK_QR(x[1], x[5], x[9], x[13]);
        PK_QR(x[2], x[6], x[10], x[14]);
        PK_QR(x[3], x[7], x[11], x[15]);
        PK_QR(x[0], x[5], x[10], x[15]);
        PK_QR(x[1], x[6], x[11], x[12]);
        PK_QR(x[2], x[7], x[8], x[13]);
        PK_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
#undef PK_QR

// candidate `half` (0 or 1) of a block: its 8 words with the top two bits cleared (< 2^254); true iff it is < p: accepted
__host__ __device__ __forceinline__ bool rng_candidate(const u32 (&blk)[16], int half, fe& x) {
#pragma unroll
    for (int w = 0; w < 8; w++) x.v[w] = blk[8 * half + w];
    x.v[7] &= 0x3fffffffu;
    u32 borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) (void)__builtin_subc(x.v[k], kPlimb(k), borrow, &borrow);
    return borrow != 0;
}

// The draw itself, for every kernel that makes one: a lane walks the pairs j = first, first + stride, ... < pairs_end of a draw of n
// elements as a state machine (pair, attempt) -- one ChaCha block per loop iteration, whichever pair and attempt the lane is at -- and
// hands element i's accepted word to put(i, x).  (Until round 5 the retry loop sat INSIDE the loop over pairs, so a wavefront repeated a
// pair's block until its unluckiest lane -- 128 candidates, each rejected with probability 0.244 -- was done: ~4 blocks per pair instead of
// the 1.43 a lane needs.  Now the waiting averages out over a lane's pairs: with ~8 pairs per lane a wavefront runs ~17 blocks for 8 pairs.)
template <class Put>
__device__ __forceinline__ void rng_draw_pairs(const RngKey& key, u32 stream, size_t first, size_t stride, size_t pairs_end, size_t n, Put put) {
    size_t j = first;
    u32 attempt = 0;
    bool done0 = false, done1 = 2 * j + 1 >= n;
    while (j < pairs_end) {
        u32 blk[16];
        chacha_block(key, (u64)j, stream, attempt, PK_RNG_ROUNDS, blk);
#pragma unroll
        for (int half = 0; half < 2; half++) {
            if (half == 0 ? done0 : done1) continue;
            fe x;
            if (rng_candidate(blk, half, x)) {  // x < p: accepted
                put(2 * j + half, x);
                if (half == 0) done0 = true;
                else done1 = true;
            }
        }
        if (done0 && done1) {
            j += stride;
            attempt = 0;
            done0 = false;
            done1 = 2 * j + 1 >= n;
        } else {
            attempt++;
        }
    }
}

}  // namespace pk
