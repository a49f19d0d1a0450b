/*
 * provekit_whir.h -- C ABI of libprovekit_whir.so: WHIR as a polynomial commitment scheme.
 *
 * Commit to `batch_size` multilinear polynomials, open them at points the caller chooses, verify the opening: what the `whir`
 * crate is used for outside WhirR1CSScheme (a lookup argument, a GR1CS variant, ...).  A fourth library above the product's C
 * ABI (like libprovekit_engine.so and libprovekit_verify.so): it links libprovekit_hip.so, calls only what provekit_hip.h
 * declares, and adds HIP kernels of its own for gfx950 (csrc/whir_pcs/evaluate.hip, linear.hip, sparse.hip, hiding.hip).
 *
 * PLAIN OPENINGS ARE NOT HIDING.  pkw_commit / pkw_open use no mask and no blinding polynomial: the proof contains openings of the
 * committed codeword and the evaluations themselves, and nothing here draws randomness: the same polynomials, points and
 * configuration give the same bytes.  Where an opening must not leak them, see provekit_whir_hiding.h: pkw_commit_hiding /
 * pkw_open_hiding / pkw_verify_hiding mask the polynomials as pk_prove masks its witness (a header of their own, which
 * states the construction and what it claims; the same library).
 *
 * One proof = one spongefish transcript (pkw_io_pattern lists its operations):
 *   root; commitment_ood_samples OOD points; their answers per polynomial; beta when batch_size > 1;
 *   the q * n_vars point coordinates (absorbed); the batch_size * q evaluations (absorbed, polynomial-major);
 *   whir::Prover::prove over sum_b beta^b poly_b with the q linear statements  <eq(point_i, .), poly> = sum_b beta^b v_{b,i},
 *   ending in the deferred_weight_evaluations hint (eq(point_i, folding point), which the verifier recomputes).
 *
 * A statement in WHIR is a list of constraints of two kinds, evaluation and linear.  pkw_open / pkw_verify state evaluations only;
 * pkw_open_linear / pkw_verify_linear state q evaluations and l LINEAR constraints  <w_i, poly_b> = s_{b,i}  for dense weight
 * tables w_i (the second half of this header).
 *
 * Conventions: those of provekit_hip.h (Montgomery 4 x u64 field elements, d_* = device pointers, PK_OK or a negative PK_ERR_*)
 * and of provekit_verify.h ("rejected" is a VERDICT in a pkv_result, not a call status; every count inside a proof is bounded
 * by the bytes that remain).  A point is n_vars field elements, variable 0 <-> the MOST significant index bit, as pk_eq_table.
 * A pkw_scheme is single-caller and belongs to the context it was created on (which must not be part of a device set).
 */
#ifndef PROVEKIT_WHIR_H
#define PROVEKIT_WHIR_H

#include "provekit_hip.h"
#include "provekit_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pkw_scheme pkw_scheme;
typedef struct pkw_commitment pkw_commitment;

#define PKW_MAX_POINTS 64

/* Verdicts of pkw_verify: the PKV_CHECK_* of the WHIR walk (provekit_verify.h), and three of the statement around it. */
#define PKW_CHECK_POINTS (PKV_CHECK_COUNT + 0)   /* the points the proof binds are not the caller's */
#define PKW_CHECK_ROOT (PKV_CHECK_COUNT + 1)     /* the root the proof binds is not expected_root */
#define PKW_CHECK_DEFERRED (PKV_CHECK_COUNT + 2) /* a deferred weight evaluation is not the weight's extension at the folding point */
#define PKW_CHECK_COUNT (PKV_CHECK_COUNT + 3)

int pkw_abi_version(void);
const char *pkw_check_name(int check); /* every PKV_CHECK_* and PKW_CHECK_* */

/* The configs of this library: what pk_whir_r1cs_io_pattern accepts (the prover's bounds) and the verifier core accepts
 * (folding_factor <= 4, n_vars + starting_log_inv_rate <= 28, ...).  PK_ERR_BAD_ARG otherwise; pkw_create_error says why
 * (the calling thread's last failed pkw_scheme_create / pkw_io_pattern / pkw_verify). */
const char *pkw_create_error(void);

/* The scheme owns a device arena sized once for one opening (about (4 + 2 R (1 + 2/F)) 2^n_vars elements at rate 1/R, fold
 * log2 F), so pkw_open allocates nothing.  pkw_scheme_arena_bytes: that size, host only. */
int pkw_scheme_create(pk_ctx *ctx, const pk_whir_config *cfg, pkw_scheme **out);
int pkw_scheme_destroy(pkw_scheme *scheme);
int pkw_scheme_arena_bytes(const pk_whir_config *cfg, size_t *bytes);
const char *pkw_last_error(const pkw_scheme *scheme);

/* The spongefish operation list (= domain separator) of a proof that opens q points, 1 <= q <= PKW_MAX_POINTS.  Host only;
 * buf == NULL queries the length.  The prover enforces it while writing, the verifier holds every operation against it. */
int pkw_io_pattern(const pk_whir_config *cfg, unsigned q, uint8_t *buf, size_t cap, size_t *len);

/* d_evals: HOST array of batch_size DEVICE pointers, each 2^n_vars evaluations over the hypercube (Montgomery); they are
 * copied, the caller may free them afterwards.  The commitment keeps both forms of the polynomials, the codeword and its
 * tree (allocated here, freed by pkw_commitment_destroy), and can be opened any number of times: the points need not be known
 * yet.  Hash version: the context's (pk_ctx_set_hash_version) at the time of the call. */
int pkw_commit(pkw_scheme *scheme, const uint64_t *const *d_evals, pkw_commitment **out);
int pkw_commitment_root(const pkw_commitment *commitment, uint8_t root[32]);
int pkw_commitment_destroy(pkw_commitment *commitment);

/* All q evaluations of all `batch` polynomials, each polynomial read from device memory once per 8 points:
 * out[b * q + i] = MLE(d_evals[b])(points[i]).  points = q * n_vars host elements; any q >= 1; n_vars <= 30.  Blocking.
 * pkw_evaluate_low_vars: the number of low variables one workgroup tile spans (the kernel's `b`); smaller n_vars take the
 * same kernel with the tile clamped to 2^n_vars. */
int pkw_evaluate(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *points, unsigned q,
                 uint64_t *out);
unsigned pkw_evaluate_low_vars(void);

/* Open `commitment` at q points: evals_out (batch_size * q elements, as pkw_evaluate; may be NULL) and the proof.  cap too
 * small: PK_ERR_BAD_ARG, *len = the size needed.  A commitment of another scheme: PK_ERR_BAD_ARG. */
int pkw_open(pkw_scheme *scheme, const pkw_commitment *commitment, const uint64_t *points, unsigned q, uint64_t *evals_out,
             uint8_t *proof_out, size_t cap, size_t *len);

/* Host only, no device.  io_pattern == NULL: pkw_io_pattern(cfg, q).  A caller's pattern may spell the labels otherwise; it must
 * declare the operations of pkw_io_pattern(cfg, q) -- another config's pattern is PKV_CHECK_IO_PATTERN before the proof is read.
 * expected_root (canonical 32 bytes) may be NULL: the
 * proof's own root is then taken as the commitment.  evals_out (batch_size * q, may be NULL) receives the evaluations the proof
 * binds, whenever the walk got past them -- they are PROVEN only when result->accepted. */
int pkw_verify(const pk_whir_config *cfg, const uint8_t *io_pattern, size_t io_pattern_len, int hash_version,
               const uint8_t *expected_root, const uint64_t *points, unsigned q, const uint8_t *proof, size_t len,
               uint64_t *evals_out, pkv_result *result);

#ifdef __cplusplus
}
#endif

/* The linear statements: pkw_weighted_sums, pkw_io_pattern_linear, pkw_open_linear, pkw_verify_linear.  Their declarations are a
 * header of their own; this header brings them along.  Whichever headers a caller includes, the library is this one:
 * -lprovekit_whir -lprovekit_hip. */
#include "provekit_whir_linear.h"

#endif /* PROVEKIT_WHIR_H */
