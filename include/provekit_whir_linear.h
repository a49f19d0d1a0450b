/*
 * provekit_whir_linear.h -- the LINEAR statements of libprovekit_whir.so (provekit_whir.h includes this header; its conventions hold).
 *
 * libprovekit_whir.so exports the four C names below.  Link -lprovekit_whir -lprovekit_hip.
 */
#ifndef PROVEKIT_WHIR_LINEAR_H
#define PROVEKIT_WHIR_LINEAR_H

#include "provekit_whir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- linear statements -------------------------------------------------------------------------------------------------------
 * A weight is a dense table of 2^n_vars elements (Montgomery, < p) indexed like an evaluation table, and
 * <w, f> = sum_x w[x] * f[x] over the evaluation form.  One proof = one transcript under the domain label
 * provekit-hip/whir-pcs-linear/v1 (pkw_io_pattern_linear lists its operations):
 *   root; OOD points; their answers per polynomial; beta when batch_size > 1; the q * n_vars point coordinates (absorbed); the
 *   l TAGS (absorbed); the batch_size * q evaluations (absorbed, polynomial-major); the batch_size * l sums (absorbed,
 *   polynomial-major); whir::Prover::prove over sum_b beta^b poly_b with the q + l constraints eq(point_i, .) then w_i (the
 *   combination randomness runs over [OOD..., points..., weights...]); the deferred_weight_evaluations hint with q + l values:
 *   eq(point_i, folding point), then the multilinear extension of w_i at the folding point.  A count of zero drops its operation.
 *
 * TAGS AND SOUNDNESS.  A dense table is NOT absorbed into the transcript: 2^n_vars sponge permutations on the host would cost more
 * than the proof.  `tags` holds l field elements the caller chooses (a hash of the table, an index into a public list, ...); they
 * are absorbed, and they are how the caller binds the weights under Fiat-Shamir.  The proof is sound for the weights ONLY AS FAR
 * AS the tags, plus whatever the caller absorbed before, fix them: a prover free to pick w_i after seeing the challenges can
 * prove a false sum. */
#define PKW_MAX_WEIGHTS 16

/* out[b * l + i] = sum_x d_weights[i][x] * d_evals[b][x]: all batch * l inner products, each polynomial read from device memory
 * ceil(l / 2) times and each weight ceil(batch / 2) times (a 2 x 2 register tile; a single polynomial takes a 1 x 4 tile instead
 * and is read ceil(l / 4) times; the public route, batch * l calls of pk_dot, reads them l and batch times).  d_evals / d_weights: HOST arrays of DEVICE pointers, 2^n_vars elements each; weights < p.
 * batch 1..4, n_vars 0..30, any l >= 1 (PK_ERR_BAD_ARG for l = 0).  Fully reduced, bit-exact.  Blocking. */
int pkw_weighted_sums(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *const *d_weights,
                      unsigned l, uint64_t *out);

/* The operation list of a proof that opens q points and l weights: q in 0..PKW_MAX_POINTS, l in 1..PKW_MAX_WEIGHTS
 * (PK_ERR_BAD_ARG with a reason in pkw_create_error otherwise).  Host only; buf == NULL queries the length. */
int pkw_io_pattern_linear(const pk_whir_config *cfg, unsigned q, unsigned l, uint8_t *buf, size_t cap, size_t *len);

/* Open `commitment` at q points (0..PKW_MAX_POINTS; points may be NULL when q = 0) and l weights (1..PKW_MAX_WEIGHTS).
 * d_weights: HOST array of l DEVICE tables, none NULL; tags: l host elements.  evals_out (batch_size * q, as pkw_open) and
 * sums_out (batch_size * l, as pkw_weighted_sums) may be NULL.  The weights are read three times: for the sums, for the sumcheck's
 * weight table (one pass over all l), and once at the folding point for the deferred values.  Allocates nothing: the scratch is
 * the arena's, pkw_scheme_arena_bytes is what it was.  Refusals (PK_ERR_BAD_ARG, reason in pkw_last_error) leave the scheme, the
 * commitment and the context usable. */
int pkw_open_linear(pkw_scheme *scheme, const pkw_commitment *commitment, const uint64_t *points, unsigned q,
                    const uint64_t *const *d_weights, const uint64_t *tags, unsigned l, uint64_t *evals_out, uint64_t *sums_out,
                    uint8_t *proof_out, size_t cap, size_t *len);

/* Host only, no device.  io_pattern == NULL: pkw_io_pattern_linear(cfg, q, l).  A tag on the transcript that is not the caller's
 * is PKW_CHECK_POINTS: the statement the proof binds is not the caller's.
 * weights: l HOST tables of 2^n_vars elements (Montgomery); the array or single entries may be NULL.  For a given table the
 * verifier computes its multilinear extension at the folding point itself -- 2^n_vars products and a copy of half the table PER
 * WEIGHT, the dominant cost of the call -- and a mismatch is PKW_CHECK_DEFERRED.  With weights == NULL or weights[i] == NULL that
 * one relation is NOT judged and *unchecked_out counts such weights: result->accepted then means "accepted PROVIDED
 * deferred_out[i] is the multilinear extension of weight i at fold_point_out".  A caller with structure computes that
 * succinctly; pkw_evaluate(ctx, &d_w, 1, n_vars, fold_point_out, 1, .) gives the value for a dense table.
 * fold_point_out (n_vars elements, a point in this header's convention) and deferred_out (l elements) are written whenever the
 * walk got that far; evals_out / sums_out (may be NULL) whenever it got past them.  Any output pointer may be NULL. */
int pkw_verify_linear(const pk_whir_config *cfg, const uint8_t *io_pattern, size_t io_pattern_len, int hash_version,
                      const uint8_t *expected_root, const uint64_t *points, unsigned q, const uint64_t *tags,
                      const uint64_t *const *weights, unsigned l, const uint8_t *proof, size_t len, uint64_t *evals_out, uint64_t *sums_out,
                      uint64_t *fold_point_out, uint64_t *deferred_out, unsigned *unchecked_out, pkv_result *result);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_WHIR_LINEAR_H */
