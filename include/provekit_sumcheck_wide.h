/*
 * provekit_sumcheck_wide.h -- the wide product sumcheck of libprovekit_sumcheck.so: up to 16 tables, 16 terms, and powers of a table
 * up to degree 5.  A sibling of provekit_sumcheck.h (pks_*) in the same library, under its own prefix, as pkss_* is.
 *
 * The statement: m tables f_0 .. f_{m-1} of 2^n evaluations each (1 <= m <= 16, 1 <= n <= 28; device memory, Montgomery form;
 * variable 0 <-> the most significant index bit), T terms (1 <= T <= 16), term t a coefficient c_t (a host element below p,
 * Montgomery) and a list of 1 .. 5 table indices, and optionally a point tau of n host elements.  A repeated index is a power: the
 * list {0, 0, 1} is f_0^2 f_1.  The list must be non-decreasing, so that a term has one spelling.  The claim is
 *
 *     sum_{x in {0,1}^n} eq(tau, x) * sum_t c_t * prod_i f_{t,i}(x) = s          (without tau the eq factor is 1)
 *
 * A vanilla Plonk gate eq * (qL a + qR b + qM a b + qO c + qC) is m = 8, T = 5; a Poseidon S-box x^5 is m = 1, T = 1, the list
 * {0, 0, 0, 0, 0}.  D, the longest list, is the degree of what is sent.
 *
 * The protocol and the bytes are provekit_sumcheck.h's, rule for rule: round i binds variable i and pairs x with x + len/2, all D + 1
 * values h_i(0) .. h_i(D) are sent, the same claim updates hold with and without tau, m final values are sent, and the proof is
 *     s | n x (D + 1) round values | m final values,     32-byte canonical little-endian each.
 * The IO pattern's label is "provekit-hip/sumcheck-wide/v1/n<n>/m<m>/T<T>/tau<0|1>/terms" followed by the terms, each its indices
 * joined by '.', the terms joined by '-'; then pks_io_pattern's operations in its order (bind, tau, coefficients, sum, per round
 * D + 1 values and a challenge, final values).  A statement pks_* can also express has ANOTHER transcript here: the two interfaces are
 * not interchangeable on the wire.  When both fit, pks_prove is the faster one: its kernel keeps every table in registers.
 *
 * WHAT "ACCEPTED" MEANS: accepted provided f_j(point_out) = finals_out[j] for every j, as in provekit_sumcheck.h.
 *
 * Out of scope: hiding; device sets (a pkss-style sharding of this prover); more than 16 tables or a degree above 5.
 *
 * Conventions: provekit_hip.h's and provekit_sumcheck.h's.  The checks are PKS_CHECK_*, their names pks_check_name's.  A pksw_prover is
 * single-caller.
 */
#ifndef PROVEKIT_SUMCHECK_WIDE_H
#define PROVEKIT_SUMCHECK_WIDE_H

#include "provekit_sumcheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKSW_MAX_TABLES 16
#define PKSW_MAX_TERMS 16
#define PKSW_MAX_DEGREE 5

typedef struct pksw_statement {
    unsigned n;                                          /* variables: tables of 2^n evaluations */
    unsigned m;                                          /* tables */
    unsigned T;                                          /* terms */
    unsigned has_tau;                                    /* 0 or 1 */
    unsigned n_bind;                                     /* caller elements absorbed first, 0 .. PKS_MAX_BIND */
    unsigned lens[PKSW_MAX_TERMS];                       /* factors of term t, 1 .. PKSW_MAX_DEGREE */
    unsigned factors[PKSW_MAX_TERMS][PKSW_MAX_DEGREE];   /* the first lens[t]: table indices, non-decreasing */
    uint64_t coeffs[PKSW_MAX_TERMS][4];                  /* Montgomery, below p */
} pksw_statement;

typedef struct pksw_prover pksw_prover;

int pksw_abi_version(void);
const char *pksw_create_error(void); /* why the calling thread's last pksw call was refused with PK_ERR_BAD_ARG before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: counts out of range, a list that is empty, longer than 5 or not non-decreasing, an index
 * >= m, a table no term uses, a coefficient >= p.  *len is always set to the full length; bytes are copied where they fit. */
int pksw_io_pattern(const pksw_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pksw_proof_bytes(const pksw_statement *stmt, size_t *len);
/* Host only: the device memory pksw_prover_create allocates for this statement (m folded copies of half length, one round's partial
 * sums, the split eq tables).  An allocation the device cannot make is pksw_prover_create's PK_ERR_OOM, not a crash. */
int pksw_arena_bytes(const pksw_statement *stmt, size_t *len);

/* ctx is borrowed: destroy the prover first. */
int pksw_prover_create(pk_ctx *ctx, const pksw_statement *stmt, pksw_prover **out);
int pksw_prover_destroy(pksw_prover *p);
const char *pksw_last_error(const pksw_prover *p);

/* pks_prove's contract: d_tables are m device pointers (a host array) and are never written; tau: n elements or NULL as the statement
 * says; bind: n_bind elements; *len = pksw_proof_bytes also when cap is too small (PK_ERR_BAD_ARG, nothing proved, the prover stays
 * usable); point_out (n) and finals_out (m) may be NULL.  Allocates no device memory.  Blocking. */
int pksw_prove(pksw_prover *p, const uint64_t *const *d_tables, const uint64_t *tau_or_null, const uint64_t *bind, uint8_t *proof_out,
               size_t cap, size_t *len, uint64_t *point_out, uint64_t *finals_out);

/* Host only, no device; pks_verify's parameters and verdicts (PKS_CHECK_ROUND, PKS_CHECK_FINAL, PKS_CHECK_SUM and the walk's own, with
 * the byte offset in the proof).  Accepted PROVIDED f_j(point_out) = finals_out[j]. */
int pksw_verify(const pksw_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *tau_or_null,
                const uint64_t *bind, const uint64_t *expected_sum_or_null, const uint8_t *proof, size_t len, uint64_t *point_out,
                uint64_t *finals_out, pkv_result *result);

/* The wide round kernel by itself, with pks_round's parameters: ONE round on tables of current length len = 2^k >= 2 (4 with a fold);
 * fold given: the tables are folded by it to length len/2 into d_out_tables first (which may equal d_tables).  tau_rest: the
 * coordinates of tau after the round's own variable, or NULL for weight 1.  Without tau_rest, len may be any multiple of 2 (of 4 with a
 * fold) up to 2^n -- the pairs are still x and x + len/2 (the quarters, with a fold) -- so that a test can fill a workgroup partly.
 * grid: 1 .. PKS_MAX_GRID; 0: the library's rule.  The bits of out (D + 1 elements) do not depend on it. */
int pksw_round(pk_ctx *ctx, const pksw_statement *stmt, const uint64_t *const *d_tables, size_t len, const uint64_t *tau_rest_or_null,
               const uint64_t *fold_or_null, uint64_t *const *d_out_tables, unsigned grid, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_SUMCHECK_WIDE_H */
