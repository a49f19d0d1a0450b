// rng_core.hpp -- the proof RNG's cipher block and accept rule, stated once for every kernel that draws from it: rng.hip's
// (pk_prove's mask, g and blinding draws, the witness fill) and whir_pcs/hiding.hip's (the masks and g of a hiding commitment).
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

}  // namespace pk
