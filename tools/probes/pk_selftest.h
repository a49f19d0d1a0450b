/* pk_selftest.h -- test entry points EXPORTED BY libprovekit_hip.so that are not part of the drop-in's API: the host build of the
 * library's __host__ __device__ arithmetic (the very source the kernels compile, so the CPU suite checks it against the oracle without
 * a GPU), the two host-only pieces of the transcript, and the proof RNG.  Declared here, next to the probes, so that
 * include/provekit_hip.h holds only what a binder needs (tests/test_abi.py: product header + this header == the library's exports). */
#ifndef PK_SELFTEST_H
#define PK_SELFTEST_H
#include "provekit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* self-test (host only, no device)
 * Runs the library's __host__ __device__ arithmetic (the same source the kernels compile) on the CPU:
 * op 0: a*b*2^-256 mod p (ark-ff mul)   1: Skyscraper v2 compress   2: v1 compress   3: from Montgomery
 * 4/5: the lazy 29-bit product / square followed by exact reduction.  n elements of 4 x u64 each.
 * 27..38: the carry chains of fe.hpp -- 27 fe_add  28 fe_sub  29 fe_neg  30 fe_dbl  31 {a < b, a == b, b < a} in words 0..2
 * 32/33/34 cond_sub_kp<1/2/4>  35 fe_reduce_any  36 fe_fold(a, b, one)  37 fe_fold(a, b, a)  38 pack_canon29(unpack29(a))
 * 39..43: the consumers of a stored hash-ready codeword element (a, b = 32 * value as plain integers below 8p/5) -- 39/40 Skyscraper
 * v2/v1 compress as the leaf fold enters it  41 a fold of three  42/43 the canonical / Montgomery opening
 * (the whole table: csrc/selftest_ops.hpp) */
/* host-only pieces of the transcript: domain-separator tag, one sponge permutation on canonical (l, r) */
int pk_selftest_keccak_tag(const uint8_t *data, size_t len, uint8_t tag[32]);
int pk_selftest_permute(uint64_t l[4], uint64_t r[4]);
int pk_selftest_arith(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);
/* the parts of the safegcd inverse (csrc/feinv.hpp) one at a time, where whole inversions of chosen operands cannot steer the state:
 * part 0 divsteps30  1 divsteps30_var  2 update_de  3 update_fg  4 normalize  5 to_s30  6 from_s30, on n records of 32 words in and
 * 32 words out (the packing: csrc/selftest_inv30.hpp; operands and expected values: tests/feinv_refs.py).  Any other part
 * is refused. */
int pk_selftest_inv30(int part, const int32_t *in, int32_t *out, size_t n);
/* the proof RNG: one ChaCha block (host; RFC 8439 state layout, words 12-13 = counter, 14-15 = nonce; `rounds` = 20 for the
 * RFC's vectors, 12 is what the library runs -- rand's ThreadRng cipher) and the device draw of n uniform field elements
 * for (seed32, stream): elements 2j, 2j+1 take the first / second 254-bit candidate of blocks (counter j, nonce {stream,
 * attempt}), attempt = 0, 1, ... until the candidate is < p */
int pk_selftest_chacha(const uint8_t key[32], uint64_t counter, uint32_t n0, uint32_t n1, int rounds, uint8_t out[64]);
int pk_selftest_random_fe(pk_ctx *ctx, const uint8_t seed32[32], uint32_t stream, uint64_t *d_out, size_t n);
/* the NTT's register butterfly network (csrc/ntt_regs.hpp dft_regs<le, d>: a lane's 2^le values, le = 2 | 3; radix-2^d DIF over the top d
 * bits of the register index, d <= le; Shoup products by the powers of w_8) on the host: n_groups x 2^le values (any value below 1.2p:
 * the network's input contract) -> the outputs of each group, reduced exactly.  Output order is the network's own (bit-reversed
 * frequency digit).  tw (may be NULL): one multiplier below p per value, applied to the UNREDUCED outputs as the pass kernel applies its
 * twiddles. */
int pk_selftest_dft(const uint64_t *in, const uint64_t *tw, uint64_t *out, int le, int d, size_t n_groups);
/* ntt_regs.hpp pre_load_sum (an NTT pass carrying pass 1 in its load): n outputs from `terms` inputs and multipliers each, rows
 * >= live past the nonzero inputs; out = the lazy result (selftest.hip). */
int pk_selftest_pre_load(const uint64_t *x, const uint64_t *tw, uint64_t *out, int terms, int live, size_t n);

/* the routes of the prover's two sumcheck loops that do without redundant work, one step per call (csrc/mle.hip):
 * the suffix equality tables of r[0, n): the levels E_i = eq(r[i+1 .. n), .), i = 0 .. n-1, back to back in d_out (2^n elements, E_i at
 * 2^n - 2^(n-i), variable 0 <-> the most significant index bit);
 * round `round` of the n-variable cubic sumcheck on a, b, c as they stand after the earlier rounds: folds by alphas[round - 1] (round > 0), sums
 * against the level E_round of d_tables and applies the host scalars: out = what pk_sumcheck_cubic_round returns for the eq array;
 * pk_sumcheck_quadratic_round by the two-sum kernels: out = h(0), claim - h(0), h(2) */
int pk_selftest_eq_suffix_tables(pk_ctx *ctx, const uint64_t *r, unsigned n, uint64_t *d_out);
int pk_selftest_sumcheck_cubic_spliteq(pk_ctx *ctx, uint64_t *d_a, uint64_t *d_b, uint64_t *d_c, const uint64_t *d_tables, unsigned n, unsigned round,
                                       const uint64_t *r, const uint64_t *alphas, uint64_t out[12]);
int pk_selftest_sumcheck_quadratic_claim(pk_ctx *ctx, const uint64_t *d_f, const uint64_t *d_w, size_t len, const uint64_t *fold_or_null,
                                         uint64_t *d_f_out, uint64_t *d_w_out, const uint64_t claim[4], uint64_t out[12]);

/* hooks of the GPU suite (process-wide, 0 = off; the library reads no test switch from the environment): which = 0 the spin bound of a
 * latency-mode gated kernel (to reach its give-up path in milliseconds), 1 microseconds the host sleeps before publishing each gate's
 * challenge (a stalled host thread), 2 non-zero = pk_ctx_create_set takes the RCCL branch for a repeated device (with PK_RCCL_LIB naming the
 * in-process stand-in tests/stub_rccl: real RCCL refuses two ranks on one GPU) */
int pk_selftest_set_hook(int which, long value);

/* The host tail's threshold of one context (csrc/host_tail.hpp), for the suite and for threshold sweeps; the build's default
 * (PK_HOST_TAIL_DEFAULT_LOG2, csrc/ctx.hpp) applies where this is never called.  Once the tables of one of pk_prove's sumchecks are no longer
 * than 2^log2_len entries they are brought to the calling thread once and the remaining rounds, the closing fold and the equality weights
 * that join them run there; an opening whose polynomial is that short (the blinding proof) forms its tables there from the start.  The
 * proof's bytes do not change.  log2_len = 0: off, exactly the device path; 1 .. 11 otherwise (anything else is refused).  A context that is
 * a rank of a device set ignores the setting. */
int pk_selftest_set_host_tail(pk_ctx *ctx, unsigned log2_len);
/* The host grinder's bound of one context (csrc/host_whir.hpp pow_grind, csrc/prover.hip pow_round): where the host tail is on, a proof of
 * work of at most max_bits bits is searched on the calling thread instead of by a launch and a synchronisation; the nonce is the same, the
 * smallest valid one.  0: every grind on the device; 1 .. 8 otherwise (anything else is refused: the witness opening's 11 bits are 2^11
 * host compressions).  The build's default is PK_HOST_POW_MAX_BITS (csrc/ctx.hpp). */
int pk_selftest_set_host_pow(pk_ctx *ctx, unsigned max_bits);
/* The host restatement of a commitment and of the grinder (csrc/host_whir.hpp; host memory in and out, no device): what pk_prove runs for a
 * blinding polynomial within the host tail's threshold.  host_commit: `batch` (1 .. 4) coefficient vectors of 2^n_vars Montgomery elements,
 * back to back -> the column-major leaf matrix (rows x width, Montgomery) and the heap of 2 * rows canonical digests that pk_commit_into
 * leaves on the device, rows = 2^(n_vars + log_inv_rate - fold) <= 2^11.  host_pow: the nonce pk_pow_solve returns, bits <= 8. */
int pk_selftest_host_commit(int hash_version, const uint64_t *coeffs, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold,
                            uint64_t *leaves_out, uint64_t *nodes_out);
int pk_selftest_host_pow(const uint8_t challenge[32], double bits, uint64_t *nonce);

#ifdef __cplusplus
}
#endif
#endif /* PK_SELFTEST_H */
