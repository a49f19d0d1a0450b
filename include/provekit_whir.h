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
 * A pkw_scheme is single-caller and belongs to the context it was created on.
 *
 * DEVICE SETS.  The context may belong to a device set (provekit_hip.h, "device sets": RCCL, the in-process transport or the host
 * transport).  Each rank of the G creates its own scheme on its own context and drives it from its own host thread, and -- as for
 * pk_prove -- EVERY RANK MAKES THE SAME CALLS WITH THE SAME INPUTS IN THE SAME ORDER: that is the caller's duty, the library cannot
 * establish it.  Every rank then gets the root, the evaluations, the sums and the proof bytes a lone scheme gives for those inputs.
 *   What is divided by G: the committed and the per-round codewords and trees (pk_commit_into / pk_commit_open, under the layouts
 *   they report), and the two ALU-bound reductions of the statement -- the evaluations of pkw_open / pkw_open_hiding, the sums of
 *   pkw_open_linear and the deferred values of dense weights: rank g runs the workgroups [g n_wg / G, (g + 1) n_wg / G) of the
 *   kernel's grid, one pk_comm_all_gather per pass exchanges the partial sums, every rank adds them.  A pass whose grid has fewer
 *   workgroups than ranks, or that G does not divide, runs whole on every rank.  Everything else of an opening is replicated:
 *   the sumcheck rounds, the weight tables, the sparse kernels, proof of work, the host side.
 *   What takes a bare pk_ctx stays whole on the calling rank: pkw_evaluate, pkw_weighted_sums, pkw_sparse_*.
 *   No rank is left waiting.  A refusal that every rank makes identically (null pointers, counts, "already opened", a sparse list
 *   that fails validation, a proof buffer that is too small) is made before any collective or after the last one, and leaves the
 *   communicator usable.  After every step that can fail on one rank alone (the allocation and copies of pkw_commit, the sparse
 *   validation's readback, a launch in a sliced pass) the ranks exchange their status in a small all-gather -- the sliced passes
 *   carry it in the gather they make anyway -- and all of them return the first non-zero status in rank order before the next
 *   sharded call.  Once per opening, after the statement is absorbed, the ranks compare 32 bytes squeezed from a copy of the
 *   sponge: ranks that were handed different points, tags or polynomials all return PK_ERR_BAD_ARG ("ranks disagree on the
 *   statement") before the first STIR opening, and the set stays usable.  A failure INSIDE a sharded call of the product library is
 *   that library's (PK_ERR_RCCL and a poisoned communicator, see provekit_hip.h).  pkw_scheme_create makes no collective.
 *   World size 1 and contexts without a communicator behave as before: nothing is exchanged, nothing is enqueued for it.
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
 * log2 F), so pkw_open allocates nothing.  pkw_scheme_arena_bytes: that size, host only -- it has no context, so it is the size
 * outside a device set and the UPPER BOUND inside one, where the arena is sized by pk_commit_sizes under the context's set (a rank
 * keeps 1 / G of every sharded codeword).  The bound carries one allowance, checked at creation and not assumed: the product's
 * sharded commit stages local and gathered digests in its scratch, which at G = 2 (and for codewords two elements wide at G = 4)
 * is up to 1.5 elements per row MORE than the lone commit's; a set's arena never exceeds pkw_scheme_arena_bytes by more than 64
 * bytes per row of the committed codeword (2^(n_vars + starting_log_inv_rate - folding_factor) rows), or creation is refused.  A
 * scheme in a set also owns the buffer its exchanges go through: under 2^14 + 2 G elements. */
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
