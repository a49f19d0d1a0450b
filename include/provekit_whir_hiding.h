/*
 * provekit_whir_hiding.h -- HIDING commitments and openings for libprovekit_whir.so (provekit_whir.h; its conventions hold).
 * provekit_whir.h does not include this header: include it yourself.
 *
 * libprovekit_whir.so exports the seven C names below.  Link -lprovekit_whir -lprovekit_hip.
 *
 * ---- the construction ---------------------------------------------------------------------------------------------------------
 * What pk_prove does to its witness (the reference: provekit/common/src/utils/zk_utils.rs:3-22,
 * provekit/prover/src/whir_r1cs.rs:182-208), as a commitment mode for any B = 1..3 polynomials of n variables.
 *
 * The config describes what is COMMITTED: cfg.n_vars = n + 1, cfg.batch_size = B + 1 (so 2 <= batch_size <= 4).  A hiding
 * commitment under a 32-byte key K commits, through pkw_commit's path, to the batch (f^_0 .. f^_{B-1}, g):
 *   f^_b   the evaluation table [f_b || mask_b]: indices below 2^n are f_b, the rest mask_b.  Variable 0 is the most significant
 *          index bit, so f^_b(0, z) = f_b(z).
 *   mask_b 2^n uniform field elements: stream PKW_RNG_MASK0 + b of the proof RNG under K
 *   g      2^(n+1) uniform field elements: stream PKW_RNG_G
 * Element i of a stream is what the proof RNG defines (csrc/rng_core.hpp, where the two stream constants live; oracle/prover_ref.py
 * random_fe(key, stream, n)): pair j = i / 2 uses the ChaCha12 block (counter j, nonce {stream, attempt}); its two 254-bit
 * candidates are each accepted iff < p; the accepted word is stored as it is.  K belongs to the commitment and is never a proof's key.
 *
 * Opening at points z_0 .. z_{q-1} (n coordinates each, 1 <= q <= PKW_MAX_POINTS) is pkw_open of that batch at the points
 * (0, z_i): the operations of pkw_io_pattern(cfg, q) in the same order under the domain label "provekit-hip/whir-pcs-hiding/v1";
 * all n + 1 coordinates are absorbed, the leading zero included, and all (B + 1) * q evaluations -- g(0, z_i) is on the
 * transcript, as the reference reveals g's sum.  WHIR then runs over sum_b beta^b f^_b + beta^B g.  So a hiding proof is a valid
 * plain proof of the extended statement: pkw_verify accepts it under cfg, the points (0, z_i) and this pattern.
 *
 * WHAT IS CLAIMED.  This is the reference's masking construction plus one counting condition, and no more than that: it is not a
 * proof of zero knowledge.  The construction: everything the WHIR proof reveals beyond the claimed evaluations is a value of
 * f^ + beta g with g uniform, or a value of some f^_b or of g that left through the committed codeword's openings and the
 * out-of-domain answers.  The counting condition: each of the latter is an evaluation of the univariate
 * F(a) + a^(2^n) (M(a) - F(a)) (F, M: f_b's and mask_b's coefficient forms) at a distinct a, and with M uniform of 2^n
 * coefficients up to 2^n such values are jointly uniform.  Two rules keep a commitment inside that count; both are enforced:
 *   MASK BUDGET    commitment_ood_samples + num_queries[0] * 2^folding_factor <= 2^n  (final_queries in place of
 *                  num_queries[0] for a config without WHIR rounds).  pkw_hiding_scheme_create, pkw_commit_hiding,
 *                  pkw_io_pattern_hiding and pkw_verify_hiding refuse other configs: PK_ERR_BAD_ARG with a reason.
 *   ONE OPENING    per commitment.  beta is drawn before the points, so a second opening would reveal more of the same
 *                  f^ + beta g; the reference opens once.  The second pkw_open_hiding that would hand out a proof is
 *                  PK_ERR_BAD_ARG ("already opened").  A refused call hands out nothing and does not count.
 * DEVICE SETS (provekit_whir.h, "Device sets").  A hiding scheme may sit on a context of a device set under the rule stated there.
 * The ranks must commit to ONE extended batch: with rng_seed32 == NULL every rank draws a key from the OS, the keys travel in one
 * 32-byte-per-rank all-gather before the draw, and every rank takes RANK 0's (the others' are discarded and wiped).  A given seed
 * is an input like any other: the same on every rank.  The one-opening flag and the mask budget are per-rank state that agrees
 * by construction, so "already opened" is a refusal every rank makes alike, before any collective.
 * Out of scope: linear and sparse statements on hiding commitments, a device verifier.
 */
#ifndef PROVEKIT_WHIR_HIDING_H
#define PROVEKIT_WHIR_HIDING_H

#include "provekit_whir.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pkw_hiding_commitment pkw_hiding_commitment; /* not a pkw_commitment: plain pkw_open cannot take it */

/* pkw_scheme_create plus the two config rules: 2 <= batch_size <= 4 (n_vars >= 2) and the mask budget.  The reason of a refusal
 * is in pkw_create_error.  The scheme is an ordinary pkw_scheme: pkw_scheme_destroy, pkw_last_error. */
int pkw_hiding_scheme_create(pk_ctx *ctx, const pk_whir_config *cfg, pkw_scheme **out);

/* The operation list of a hiding proof that opens q points: pkw_io_pattern(cfg, q)'s operations under the hiding label.  Host only;
 * buf == NULL queries the length. */
int pkw_io_pattern_hiding(const pk_whir_config *cfg, unsigned q, uint8_t *buf, size_t cap, size_t *len);

/* d_evals: HOST array of B = batch_size - 1 DEVICE pointers, each 2^n = 2^(n_vars - 1) evaluations (Montgomery); they are copied.
 * The masks and g are drawn on the device in one launch (csrc/whir_pcs/hiding.hip).  rng_seed32 == NULL: the key comes from
 * getrandom(2); otherwise these 32 bytes are the key -- a TEST HOOK, two commitments under one key share their masks.  A scheme
 * whose config breaks a hiding rule (one made by pkw_scheme_create) is refused with the reason in pkw_last_error. */
int pkw_commit_hiding(pkw_scheme *scheme, const uint64_t *const *d_evals, const uint8_t *rng_seed32, pkw_hiding_commitment **out);
int pkw_hiding_commitment_root(const pkw_hiding_commitment *commitment, uint8_t root[32]);
int pkw_hiding_commitment_destroy(pkw_hiding_commitment *commitment);

/* Open at q points of n = n_vars - 1 coordinates each (points = q * n HOST elements).  evals_out (B * q elements,
 * evals_out[b * q + i] = f_b(z_i); may be NULL) and the proof.  Errors, cap / *len and NULL rules are pkw_open's; a second
 * opening of one commitment is PK_ERR_BAD_ARG. */
int pkw_open_hiding(pkw_scheme *scheme, pkw_hiding_commitment *commitment, const uint64_t *points, unsigned q, uint64_t *evals_out,
                    uint8_t *proof_out, size_t cap, size_t *len);

/* Host only, no device: pkw_verify under the hiding pattern with every point prefixed by 0.  io_pattern == NULL:
 * pkw_io_pattern_hiding(cfg, q).  evals_out (B * q elements, may be NULL) receives the first B rows of the evaluations the proof
 * binds -- f_b(z_i), PROVEN only when result->accepted.  A proof whose bound points do not start with 0 is PKW_CHECK_POINTS.
 * The verdicts are pkw_verify's; none is added. */
int pkw_verify_hiding(const pk_whir_config *cfg, const uint8_t *io_pattern, size_t io_pattern_len, int hash_version,
                      const uint8_t *expected_root, const uint64_t *points, unsigned q, const uint8_t *proof, size_t len,
                      uint64_t *evals_out, pkv_result *result);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_WHIR_HIDING_H */
