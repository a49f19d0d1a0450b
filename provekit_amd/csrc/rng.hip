// rng.hip -- the proof RNG: a device CSPRNG keyed once per proof, and the draws made from it.
//
// The cipher block and the accept rule are rng_core.hpp's (whir_pcs/hiding.hip draws from the same cipher); here are the kernels.
// The reference draws the ZK mask, the random polynomial g and the Spartan blinding univariates from thread_rng
// (provekit/common/src/utils/zk_utils.rs:13-22, provekit/prover/src/whir_r1cs.rs:197,212-221): rand's ThreadRng, i.e. ChaCha12
// seeded from the OS.  Here: one 256-bit key per proof (getrandom(2) inside pk_prove unless the caller injects a seed -- a test
// hook), expanded on the device with the same cipher -- the ChaCha block function (RFC 8439 quarter rounds and state layout),
// 12 rounds.  Elements 2j and 2j+1 of draw `stream` share the blocks (counter = j, nonce = {stream, attempt}): a block holds
// two 254-bit candidates, the first for element 2j, the second for 2j+1, each accepted iff < p (what ark-ff's Fp::rand does,
// so every element is uniform on [0, p)); an element whose candidate was rejected takes its candidate of the next attempt.
#include <sys/random.h>

#include <cerrno>

#include "internal.hpp"
#include "fe29.hpp"

using namespace pk;

namespace {

// A lane walks its pairs j = g, g + stride, ... (rng_core.hpp rng_draw_pairs; launched with ~8 pairs per lane)
__global__ __launch_bounds__(256) void random_fe_kernel(fe* __restrict__ out, size_t n, RngKey key, u32 stream) {
    PK_LATENCY_PRIO();
    rng_draw_pairs(key, stream, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, (n + 1) / 2, n,
                   [&](size_t i, const fe& x) { fe_store(out + i, x); });
}
// ~8 pairs per lane (see the kernel), at least one wavefront per SIMD's worth of workgroups when the draw is long enough
inline unsigned random_fe_grid(const pk_ctx* ctx, size_t n) {
    const size_t pairs = (n + 1) / 2;
    size_t blocks = (pairs + 256 * 8 - 1) / (256 * 8);
    const size_t cap = (size_t)ctx->num_cus * 8;
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks < cap ? blocks : cap);
}

// fill_witness (provekit/prover/src/witness/mod.rs:15-30): every None entry takes FieldElement::from(rng.random::<u128>()).
// Entry i reads the (i mod 4)-th 128-bit word of ChaCha block i / 4 of stream RNG_FILL, so the result does not depend on the
// launch shape.  *n_filled counts them (the reference logs the count).
__global__ __launch_bounds__(256) void fill_witness_kernel(fe* __restrict__ w, const uint8_t* __restrict__ is_set, size_t n, RngKey key, u32 stream,
                                                           unsigned long long* n_filled) {
    PK_LATENCY_PRIO();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned mine = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (is_set[i]) continue;
        u32 blk[16];
        chacha_block(key, (u64)(i >> 2), stream, 0, PK_RNG_ROUNDS, blk);
        fe x = fe_zero();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u32 v = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) v = (i & 3) == (size_t)q ? blk[4 * q + k] : v;
            x.v[k] = v;
        }
        fe_store(w + i, fe_to_montx(x));
        mine++;
    }
    if (mine) atomicAdd(n_filled, (unsigned long long)mine);  // n_filled is DEVICE memory: agent-scope atomics are exact there
}

}  // namespace

namespace pk {

// one draw: n uniform field elements of stream `stream` under `key` into d_out (launch only)
int random_fe(pk_ctx* ctx, uint64_t* d_out, size_t n, const RngKey& key, uint32_t stream) {
    random_fe_kernel<<<random_fe_grid(ctx, n), 256, 0, ctx->stream>>>((fe*)d_out, n, key, stream);
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}

// 256-bit key of one proof's random draws: fresh from the OS CSPRNG (the reference's thread_rng) unless injected.  One proof
// sharded over a device set: every rank must mask with the SAME polynomials -- rank 0's key goes to everybody.
int proof_key(pk_ctx* ctx, const uint8_t* rng_seed32, RngKey& key) {
    if (rng_seed32) {
        memcpy(key.k, rng_seed32, 32);
        return PK_OK;
    }
    size_t got = 0;
    while (got < 32) {
        ssize_t r = getrandom((char*)key.k + got, 32 - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return set_err(ctx, PK_ERR_HIP, "getrandom failed: %s", strerror(errno));
        }
        got += (size_t)r;
    }
    if (comm_world(ctx) > 1) {
        int rc = ensure_scratch(ctx, ((size_t)1 << 19) + 32 * (size_t)(PK_MAX_RANKS + 1));
        if (rc) return rc;
        char* d_key = (char*)ctx->d_scratch + ((size_t)1 << 19);  // clear of the reduction area (head) and the PoW words (tail)
        PK_HIP(ctx, hipMemcpyAsync(d_key, key.k, 32, hipMemcpyHostToDevice, ctx->stream));
        rc = comm_all_gather(ctx, d_key, d_key + 32, 32);
        if (rc) return rc;
        PK_HIP(ctx, hipMemcpyAsync(key.k, d_key + 32, 32, hipMemcpyDeviceToHost, ctx->stream));
        PK_WAIT(ctx);
    }
    return PK_OK;
}

}  // namespace pk

extern "C" {

// host-only: one block of the proof RNG's cipher (RFC 8439 layout: words 12,13 = counter, 14,15 = nonce); rounds = 20 for
// the RFC's vectors, 12 (PK_RNG_ROUNDS) for what random_fe_kernel runs
int pk_selftest_chacha(const uint8_t key[32], uint64_t counter, uint32_t n0, uint32_t n1, int rounds, uint8_t out[64]) {
    if (!key || !out || rounds < 2 || (rounds & 1)) return PK_ERR_BAD_ARG;
    RngKey k;
    memcpy(k.k, key, 32);
    u32 blk[16];
    chacha_block(k, counter, n0, n1, rounds, blk);
    memcpy(out, blk, 64);
    return PK_OK;
}
// the device draw itself: n uniform field elements of stream `stream` under `seed32` (what pk_prove fills the mask with)
int pk_selftest_random_fe(pk_ctx* ctx, const uint8_t seed32[32], uint32_t stream, uint64_t* d_out, size_t n) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, seed32 && (n == 0 || d_out), "null pointer");
    if (!n) return PK_OK;
    RngKey k;
    memcpy(k.k, seed32, 32);
    return random_fe(ctx, d_out, n, k, stream);
}

int pk_witness_fill(pk_ctx* ctx, uint64_t* d_witness, const uint8_t* d_is_set, size_t n, const uint8_t* rng_seed32, size_t* n_filled) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, n == 0 || (d_witness && d_is_set), "null pointer");
    if (n_filled) *n_filled = 0;
    if (!n) return PK_OK;
    RngKey key;
    int rc = proof_key(ctx, rng_seed32, key);
    if (rc) return rc;
    // the count lives in device memory (the first word of the transient workspace; the stream is in order): atomics on the pinned
    // host mailbox would need PCIe atomics, which not every host link provides
    rc = ensure_ws(ctx, 256);
    if (rc) return rc;
    unsigned long long* d_count = (unsigned long long*)ctx->d_ws;
    PK_HIP(ctx, hipMemsetAsync(d_count, 0, 8, ctx->stream));
    fill_witness_kernel<<<grid_for(ctx, n, 256), 256, 0, ctx->stream>>>((fe*)d_witness, d_is_set, n, key, RNG_FILL, d_count);
    PK_LAUNCH_CHECK(ctx);
    if (n_filled) {
        unsigned long long h = 0;
        PK_HIP(ctx, hipMemcpyAsync(&h, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));
        rc = sync_stream(ctx);
        if (rc) return rc;
        *n_filled = (size_t)h;
    }
    return PK_OK;
}

}  // extern "C"
