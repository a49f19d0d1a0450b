/*
 * provekit_verify.h -- C ABI of libprovekit_verify.so: WhirR1CSVerifier::verify for the proofs pk_prove writes.
 *
 * A third library above the product's C ABI (like libprovekit_engine.so): it links libprovekit_hip.so, calls only what
 * provekit_hip.h declares, and adds two HIP kernels of its own for gfx950 (csrc/verify/verify.hip).
 *
 * What is verified: the byte string pk_prove / pke_prove_many / pk_noir_prove return (WhirR1CSProof::transcript), under the
 * STATEMENT it was made for: m, m_0, the two pk_whir_configs, the IO-pattern bytes in force (pk_whir_r1cs_io_pattern's, or the
 * caller's: what pk_scheme_set_io_pattern took), the Skyscraper version, and -- optionally -- the R1CS, which enables the
 * matrix-evaluation check of the deferred weights (deferred_k == eq(alpha)^T M_k eq(point) (1 - point_0); the reference leaves
 * it to recursive-verifier/app/circuit/matrix_evaluation.go).
 *
 * The checks and their order are those of provekit/verifier/src/whir_r1cs.rs:38-90,110-172 and of whir's verifier as the Go
 * circuit spells it (recursive-verifier/app/circuit/whir.go:51-220, whir_utilities.go, mtUtilities.go).
 *
 * Conventions
 *   - Every call returns PK_OK (0) or a negative PK_ERR_* of provekit_hip.h: an error of the CALL (null pointer, a statement
 *     that is no statement, no memory, a HIP failure).  "Rejected" is a VERDICT, not an error: pkv_verify returns PK_OK and
 *     says so in the pkv_result.
 *   - Nothing throws or aborts across the boundary.  Every length prefix and count inside a proof is attacker-controlled and is
 *     bounded by the bytes that remain before anything is reserved: verifying a proof allocates O(its length).
 *   - A pkv_verifier is single-caller (not thread-safe); distinct verifiers may be used from distinct threads.
 *   - Field elements are Montgomery 4 x u64 unless a parameter says canonical, as in provekit_hip.h.
 */
#ifndef PROVEKIT_VERIFY_H
#define PROVEKIT_VERIFY_H

#include "provekit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pkv_verifier pkv_verifier;

/* The check a rejected proof failed.  The numbers are stable; pkv_check_name gives the identifier as a string. */
#define PKV_CHECK_NONE 0             /* accepted */
#define PKV_CHECK_TRANSCRIPT_SHORT 1 /* the proof ends before the operation that reads it */
#define PKV_CHECK_NON_CANONICAL 2    /* a scalar on the transcript is >= p */
#define PKV_CHECK_IO_PATTERN 3       /* an absorb / squeeze / hint that the IO pattern does not declare next */
#define PKV_CHECK_HINT_FORMAT 4      /* a hint's counts, widths or length do not describe what the statement expects */
#define PKV_CHECK_OPENING_COUNT 5    /* leaves, siblings, paths and indexes of a MultiPath differ in number */
#define PKV_CHECK_MERKLE 6           /* an opening does not reach the committed root */
#define PKV_CHECK_ZK_SUMCHECK 7      /* Spartan's cubic sumcheck: h(0) + h(1) != the running claim */
#define PKV_CHECK_WHIR_SUMCHECK 8    /* WHIR's quadratic sumcheck: h(0) + h(1) != the running claim */
#define PKV_CHECK_POW 9              /* proof of work below the round's difficulty */
#define PKV_CHECK_STIR_INDICES 10    /* the opened leaves are not the challenge set */
#define PKV_CHECK_FINAL_POLY 11      /* the final polynomial disagrees with a folded opening */
#define PKV_CHECK_WHIR_FINAL 12      /* the last sumcheck claim != W(r) * final(r) (computeWPoly) */
#define PKV_CHECK_BLINDING_WEIGHT 13 /* the deferred evaluation of the blinding weight is not its MLE */
#define PKV_CHECK_TRAILING_BYTES 14  /* bytes or declared operations left after the proof */
#define PKV_CHECK_SPARTAN 15         /* the last sumcheck value != (a b - c) eq(r, alpha) */
#define PKV_CHECK_WITNESS_FIT 16     /* the attached R1CS has more witnesses than 2^(m-1) */
#define PKV_CHECK_MATRIX_EVAL 17     /* a deferred weight evaluation is not the R1CS matrix's */
#define PKV_CHECK_COUNT 18

typedef struct pkv_result {
    int accepted;      /* 1: every check passed; 0: rejected */
    int check;         /* PKV_CHECK_*: the first check that failed (PKV_CHECK_NONE when accepted) */
    uint64_t offset;   /* bytes of the proof consumed when the verdict was reached */
    char message[160]; /* the reason, NUL-terminated ("" when accepted) */
} pkv_result;

int pkv_abi_version(void);
const char *pkv_check_name(int check);

/* The statement.  io_pattern == NULL: the library's own restatement for this shape (pk_whir_r1cs_io_pattern).  hash_version: 2 or 1
 * (pk_ctx_set_hash_version).  PK_ERR_BAD_ARG: a shape no prover of this library accepts (pkv_create_error says why);
 * PK_ERR_IO_PATTERN: bytes that DomainSeparator::finalize refuses.  Host only. */
int pkv_verifier_create(unsigned m, unsigned m_0, const pk_whir_config *whir_witness, const pk_whir_config *whir_for_hiding_spartan,
                        const uint8_t *io_pattern, size_t io_pattern_len, int hash_version, pkv_verifier **out);
const char *pkv_create_error(void); /* why the calling thread's last pkv_verifier_create failed */
int pkv_verifier_destroy(pkv_verifier *v);
const char *pkv_last_error(const pkv_verifier *v);
/* Attach the R1CS in the form pk_r1cs_create takes (copied; the arrays are checked: offsets non-decreasing, columns and value
 * indexes in range).  Enables PKV_CHECK_WITNESS_FIT and PKV_CHECK_MATRIX_EVAL.  Call it before pkv_verifier_attach_device. */
int pkv_verifier_set_r1cs(pkv_verifier *v, size_t num_constraints, size_t num_witnesses, const pk_sparse_matrix mats[3],
                          const uint64_t *interner, size_t n_interned);

/* The host core: the complete verification on the calling thread, no device. */
int pkv_verify(pkv_verifier *v, const uint8_t *proof, size_t len, pkv_result *result);

/* The device path.  pkv_verifier_attach_device binds a context (borrowed: destroy the verifier, or attach NULL, before the
 * context) and uploads the attached R1CS once.  pkv_verify_many then verifies n proofs per call: the host replays each
 * transcript's Fiat-Shamir and checks every scalar relation that needs no opening; the Merkle openings and their fold values of
 * ALL proofs run as one kernel launch, the 3 n bilinear forms eq(alpha)^T M eq(y) as one pass over the matrices per 16 proofs;
 * the host finishes each proof with the kernels' outputs.  Verdict and failing check equal pkv_verify's for every proof; a proof
 * rejected before its first opening costs no device work and does not disturb the others.  Blocking. */
int pkv_verifier_attach_device(pkv_verifier *v, pk_ctx *ctx);
int pkv_verify_many(pkv_verifier *v, const uint8_t *const *proofs, const size_t *lens, size_t n, pkv_result *results);

/* The two kernels by themselves (tests, benchmarks).
 * pkv_openings_check: k openings of `width` canonical leaf elements each (leaves: k*width FEs, any 256-bit value is taken mod p
 * as the hash does), sibling digest, `depth` path digests in root->leaf order (paths: k*depth FEs), leaf index and expected
 * root per opening.  reached[i] = 1 when opening i's walk ends in roots[i].  weights (width Montgomery FEs, or NULL) gives
 * folds[i] = sum_j leaf_i[j] * weights[j], canonical: with weights[b*2^k + j] = beta^b prod_t r_t^bit_t(j) that is
 * MultivarPoly(leaf combined by beta, r) (utilities.go:15-22, mtUtilities.go:98-114).
 * pkv_matrix_evaluations: for K (alpha, point) pairs (m_0 resp. m-1 Montgomery FEs each) the 3 K sums
 * sum_nnz v eq(alpha_k)[row] eq(point_k)[col], out[3k + matrix], Montgomery.  Needs an attached R1CS and device. */
int pkv_openings_check(pk_ctx *ctx, int hash_version, const uint64_t *leaves, size_t k, size_t width, const uint64_t *siblings,
                       const uint64_t *paths, size_t depth, const uint64_t *indices, const uint64_t *roots,
                       const uint64_t *weights, uint8_t *reached, uint64_t *folds);
int pkv_matrix_evaluations(pkv_verifier *v, const uint64_t *alphas, const uint64_t *points, size_t K, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_VERIFY_H */
