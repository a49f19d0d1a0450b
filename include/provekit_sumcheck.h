/*
 * provekit_sumcheck.h -- C ABI of libprovekit_sumcheck.so: product sumchecks over device-resident tables.
 *
 * A fifth library above the product's C ABI (like libprovekit_verify.so and libprovekit_whir.so): it links libprovekit_hip.so, calls
 * only what provekit_hip.h declares, and adds one HIP kernel family of its own for gfx950 (csrc/sumcheck/round.hip).
 *
 * The statement: m tables f_0 .. f_{m-1} of 2^n evaluations each (1 <= m <= 4, 1 <= n <= 28; device memory, Montgomery form;
 * variable 0 <-> the most significant index bit, as in pk_eq_table and pkw_open), T terms (1 <= T <= 4), term t a coefficient c_t
 * (a host element below p, Montgomery) and a non-empty set S_t of at most 3 distinct tables given as a bitmask, and optionally a
 * point tau of n host elements.  The claim is
 *
 *     sum_{x in {0,1}^n} eq(tau, x) * sum_t c_t * prod_{j in S_t} f_j(x) = s          (without tau the eq factor is 1)
 *
 * <a, b> is m = 2, T = 1, masks = {3}; the R1CS relation eq * (a b - c) is m = 3, T = 2, masks = {3, 4}, coefficients {1, -1},
 * tau given; an evaluation claim eq * f is m = 1, T = 1, masks = {1}, tau given.  D = max |S_t| is the degree of what is sent.
 *
 * The protocol: round i = 0 .. n-1 binds variable i (it pairs x with x + len/2).  With r_{<i} the earlier challenges and
 * e_i = eq(tau_{<i}, r_{<i}) (1 without tau), the prover sends the D + 1 values h_i(0) .. h_i(D) of
 *     h_i(X) = sum_{x'} eq(tau_{>i}, x') * G(r_{<i}, X, x'),        G = the sum of the terms;
 * all D + 1 are sent (recovering one would divide by tau_i, which may be 0).  The verifier checks
 *     e_i * ((1 - tau_i) h_i(0) + tau_i h_i(1)) = claim_i       (without tau: h_i(0) + h_i(1) = claim_i),
 * draws r_i, and goes on with claim_{i+1} = e_i * eq(tau_i, r_i) * h_i(r_i) (without tau: h_i(r_i)).  After round n-1 the prover
 * sends the m final values v_j = f_j(r), and the verifier checks eq(tau, r) * sum_t c_t prod_{j in S_t} v_j against the last claim.
 *
 * The transcript is the product's spongefish duplex sponge.  pks_io_pattern writes its pattern: the label
 * "provekit-hip/sumcheck/v1" with n, m, T, the presence of tau and every mask spelled in decimal, then: absorb n_bind caller
 * elements (0 .. 16; commitment roots and whatever else the caller must bind; none: no operation), absorb tau if given, absorb the T
 * coefficients, absorb s, per round absorb D + 1 values and squeeze one challenge, absorb the m final values.  The bind elements,
 * tau and the coefficients are the statement: both sides absorb them, they are not part of the proof.  The proof is
 *     s | n x (D + 1) round values | m final values,     32-byte canonical little-endian each.
 *
 * WHAT "ACCEPTED" MEANS: accepted provided f_j(point_out) = finals_out[j] for every j.  The sumcheck reduces the claim about the sum to
 * those m evaluation claims and proves nothing about them.  pkw_open / pkw_verify (provekit_whir.h) at point_out is the way to
 * establish them for committed tables: point_out's coordinate order is already pkw_open's.
 *
 * Out of scope: hiding / zero knowledge of the round polynomials; a batched device verifier.  More than 4 tables or terms, and powers
 * of one table in a term, are provekit_sumcheck_wide.h's (pksw_*: 16 tables, 16 terms, degree 5; another label).  Device sets: a
 * prover of pks_prover_create on a context of a set runs whole on its rank; provekit_sumcheck_sharded.h shards the same proof over
 * the set's ranks (pkss_prover_create, pkss_prove).
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64 unless a parameter says canonical.  A pks_prover is single-caller.
 */
#ifndef PROVEKIT_SUMCHECK_H
#define PROVEKIT_SUMCHECK_H

#include "provekit_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKS_MAX_TABLES 4
#define PKS_MAX_TERMS 4
#define PKS_MAX_TERM_TABLES 3
#define PKS_MAX_VARS 28
#define PKS_MAX_BIND 16
#define PKS_MAX_GRID 1024

/* The verifier core's check numbers keep their values (PKV_CHECK_*); this library's own follow them. */
#define PKS_CHECK_ROUND 18 /* a round's values do not add up to the running claim */
#define PKS_CHECK_FINAL 19 /* the terms of the final values != the last claim */
#define PKS_CHECK_SUM 20   /* the proof's s is not the sum the caller expects */
#define PKS_CHECK_COUNT 21

typedef struct pks_statement {
    unsigned n;                          /* variables: tables of 2^n evaluations */
    unsigned m;                          /* tables */
    unsigned T;                          /* terms */
    unsigned has_tau;                    /* 0 or 1 */
    unsigned n_bind;                     /* caller elements absorbed first */
    unsigned masks[PKS_MAX_TERMS];       /* bit j: table j is a factor of the term */
    uint64_t coeffs[PKS_MAX_TERMS][4];   /* Montgomery, below p */
} pks_statement;

typedef struct pks_prover pks_prover;

int pks_abi_version(void);
const char *pks_check_name(int check);
const char *pks_create_error(void); /* why the calling thread's last call was refused with PK_ERR_BAD_ARG before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: counts out of range, an empty mask or one that names a table >= m, a table no term
 * uses, a term of more than 3 tables, a coefficient >= p.  *len is always set to the full length; bytes are copied where they fit. */
int pks_io_pattern(const pks_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pks_proof_bytes(const pks_statement *stmt, size_t *len);

/* The prover owns one device arena, sized here: m tables of 2^(n-1) for the folded copies, the partial sums and the split eq
 * tables.  ctx is borrowed: destroy the prover first. */
int pks_prover_create(pk_ctx *ctx, const pks_statement *stmt, pks_prover **out);
int pks_prover_destroy(pks_prover *p);
const char *pks_last_error(const pks_prover *p);

/* d_tables: m device pointers (a host array).  tau: n elements or NULL as the statement says; bind: n_bind elements.  The proof goes
 * to proof_out (cap bytes; *len = pks_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG, nothing proved, the prover stays
 * usable).  point_out: the n challenges; finals_out: the m values f_j(point_out); either may be NULL.  s, the first element of the
 * proof, is computed by round 0.  Allocates no device memory and never writes the caller's tables.  Blocking. */
int pks_prove(pks_prover *p, const uint64_t *const *d_tables, const uint64_t *tau_or_null, const uint64_t *bind, uint8_t *proof_out,
              size_t cap, size_t *len, uint64_t *point_out, uint64_t *finals_out);

/* Host only, no device.  io_pattern NULL: pks_io_pattern's bytes for stmt.  expected_sum NULL: any s is taken (result "accepted" then
 * holds for the s the proof states, its first 32 bytes).  point_out (n) and finals_out (m) are written when the proof is accepted:
 * accepted provided f_j(point_out) = finals_out[j]. */
int pks_verify(const pks_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *tau_or_null,
               const uint64_t *bind, const uint64_t *expected_sum_or_null, const uint8_t *proof, size_t len, uint64_t *point_out,
               uint64_t *finals_out, pkv_result *result);

/* The round kernel by itself (tests, benchmarks): ONE round on tables of current length len = 2^k >= 2 (4 with a fold).
 * fold NULL: out = h(0) .. h(D) of the tables as they stand (pairs x, x + len/2); d_out_tables is not used.
 * fold given: the tables are first folded by it to length len/2 into d_out_tables (m device pointers; may equal d_tables: each
 * lane reads what it writes), and the round is that of the folded tables.
 * tau_rest: the coordinates of tau after the round's own variable (log2 of the round's length, less one), or NULL for weight 1.
 * grid: workgroups, 1 .. PKS_MAX_GRID; 0: the library's rule.  The bits of out do not depend on it.  out: D + 1 elements. */
int pks_round(pk_ctx *ctx, const pks_statement *stmt, const uint64_t *const *d_tables, size_t len, const uint64_t *tau_rest_or_null,
              const uint64_t *fold_or_null, uint64_t *const *d_out_tables, unsigned grid, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_SUMCHECK_H */
