/*
 * provekit_whir_sparse.h -- SPARSE weights for the linear statements of libprovekit_whir.so (provekit_whir_linear.h; its
 * conventions hold).  provekit_whir.h does not include this header: include it yourself.
 *
 * libprovekit_whir.so exports the five C names below.  Link -lprovekit_whir -lprovekit_hip.
 */
#ifndef PROVEKIT_WHIR_SPARSE_H
#define PROVEKIT_WHIR_SPARSE_H

#include "provekit_whir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the representation ------------------------------------------------------------------------------------------------------
 * A sparse weight is a second way to write down the SAME statement as a dense table: the transcript, the IO pattern
 * (pkw_io_pattern_linear) and the proof bytes are those of the densified tables, and tags bind the weights as they do there.
 * l weights, 0 <= l <= PKW_MAX_WEIGHTS, are given CSR-style:
 *   offsets  l + 1 HOST uint64_t; offsets[0] == 0, non-decreasing; weight i owns entries offsets[i] .. offsets[i + 1]
 *   index    one uint32_t per entry: the position in the evaluation table (a dense weight's indexing); STRICTLY INCREASING within
 *            a weight, each < 2^n_vars
 *   value    4 x uint64_t per entry: Montgomery, < p
 * Weight i stands for the table that is value[k] at index[k] and 0 elsewhere.  A weight without entries is the zero table; the
 * index rule bounds a weight at 2^n_vars entries.  For the prover's entry points index and value are DEVICE arrays (NULL allowed
 * when offsets[l] == 0), for the verifier HOST arrays.
 *
 * VALIDATION.  No index is dereferenced before it was checked.  Bad offsets are refused on the host.  Each device entry point
 * first runs a pass over index[0 .. offsets[l]) only, and the first entry that is >= 2^n_vars or not above the entry before it
 * in its weight makes the call return PK_ERR_BAD_ARG with a reason naming the weight and the entry, before any gather or scatter
 * is enqueued; the context, the scheme and the commitment stay usable.  The reason is in pkw_create_error for the three
 * pk_ctx entry points and pkw_verify_sparse, in pkw_last_error(scheme) for pkw_open_sparse.  The prover does not check
 * value < p, as it does not for a dense table. */

/* out[b * l + i] = sum_k value_i[k] * d_evals[b][index_i[k]]: pkw_weighted_sums on the densified tables, bit for bit, from
 * nnz gathers per polynomial.  d_evals: HOST array of `batch` DEVICE pointers, 2^n_vars elements each.  batch 1..4, n_vars 0..30.
 * Fully reduced.  Blocking. */
int pkw_sparse_sums(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *offsets,
                    const uint32_t *d_index, const uint64_t *d_value, unsigned l, uint64_t *out);

/* d_table[index_i[k]] += scales[i] * value_i[k] over the 2^n_vars elements of d_table (each < p); scales: l HOST elements
 * (Montgomery, < p).  Positions no entry names are not touched.  Several weights may name one position: the weights are applied
 * one after the other, and inside a weight the indexes are distinct.  Blocking. */
int pkw_sparse_accumulate(pk_ctx *ctx, uint64_t *d_table, unsigned n_vars, const uint64_t *offsets, const uint32_t *d_index,
                          const uint64_t *d_value, unsigned l, const uint64_t *scales);

/* out[i] = sum_k value_i[k] * eq(index_i[k], point): the multilinear extension of weight i at `point` (n_vars HOST elements, a
 * point in provekit_whir.h's convention), what pkw_evaluate gives on the densified table -- with no table: n_vars goes up to 30
 * and the cost is one product per 8 index bits and entry.  Blocking. */
int pkw_sparse_evaluate(pk_ctx *ctx, unsigned n_vars, const uint64_t *offsets, const uint32_t *d_index, const uint64_t *d_value,
                        unsigned l, const uint64_t *point, uint64_t *out);

/* pkw_open_linear with the l weights (1..PKW_MAX_WEIGHTS) as lists: its counts, tags, outputs, refusals and BYTES.  The lists are
 * validated once, then read three times (sums, sumcheck weight table, folding point), O(nnz) each.  Allocates nothing;
 * pkw_scheme_arena_bytes is what it was.  Dense and sparse weights cannot be mixed in one proof. */
int pkw_open_sparse(pkw_scheme *scheme, const pkw_commitment *commitment, const uint64_t *points, unsigned q, const uint64_t *offsets,
                    const uint32_t *d_index, const uint64_t *d_value, const uint64_t *tags, unsigned l, uint64_t *evals_out,
                    uint64_t *sums_out, uint8_t *proof_out, size_t cap, size_t *len);

/* Host only, no device: pkw_verify_linear's walk, except that the deferred relation of EVERY weight is judged from the entries,
 * sum_k value[k] * eq(index[k], folding point), in O(nnz) products per weight plus four tables of 2^8 elements; nothing of size
 * 2^n_vars is allocated.  So there is no unchecked count and `accepted` is unconditional; a mismatch is PKW_CHECK_DEFERRED naming
 * the weight.  index / value: HOST arrays.  Offsets or indexes that break the rules above, and values >= p, are PK_ERR_BAD_ARG
 * with a reason naming the weight and the entry.  Outputs as pkw_verify_linear's; any may be NULL. */
int pkw_verify_sparse(const pk_whir_config *cfg, const uint8_t *io_pattern, size_t io_pattern_len, int hash_version,
                      const uint8_t *expected_root, const uint64_t *points, unsigned q, const uint64_t *tags, const uint64_t *offsets,
                      const uint32_t *index, const uint64_t *value, unsigned l, const uint8_t *proof, size_t len, uint64_t *evals_out,
                      uint64_t *sums_out, uint64_t *fold_point_out, uint64_t *deferred_out, pkv_result *result);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_WHIR_SPARSE_H */
