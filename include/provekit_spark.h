/*
 * provekit_spark.h -- C ABI of libprovekit_spark.so: sparse-matrix evaluation proofs (Spark, from Spartan) over device tables.
 *
 * An eleventh library above the product's C ABI: it links libprovekit_hip.so, libprovekit_sumcheck.so, libprovekit_fracsum.so
 * (transitively) and libprovekit_tuplelookup.so, calls pks_* and pkt_* through their C ABI and of the product only pk_malloc, pk_free,
 * pk_ctx_sync and pk_eq_table, and adds HIP kernels of its own for gfx950 (csrc/spark/spark.hip): the per-query gather, the matrix's
 * columns and the indices' histograms.  It links neither libprovekit_whir.so nor the verify library: committing and opening the
 * columns is the caller's composition (examples/spark_pcs_demo.cpp).
 *
 * WHY: every proof pk_prove writes ends in three deferred values which pkv_verify checks by evaluating the R1CS matrices itself,
 * deferred_k = eq(alpha)^T M_k eq(point) = sum_nnz v eq(alpha)[row] eq(point)[col] (PKV_CHECK_MATRIX_EVAL): O(nnz) per proof, the only
 * part of verification that grows with the circuit.  Here the matrix is committed once, as dense columns, and M~(rx, ry) = v is proved
 * with one product sumcheck and two ROM lookups into eq tables; the verifier pays O(log) and a few openings.
 *
 * THE STATEMENT: n, s, t, n_bind: 2^n entries of a matrix of 2^s rows and 2^t columns; 1 <= n, s, t <= 28; n_bind is 0 .. 16.  Variable
 * 0 is the most significant index bit (pks's, pkt's, pk_eq_table's and pkw_open's convention).  Entries beyond the real non-zeros are
 * padding (row 0, col 0, val 0); duplicates of one (row, col) add.  The device tables, Montgomery form, below p:
 *   fixed by the matrix, committed once by the caller before any query:
 *     row, col: 2^n elements each -- the indices as field elements;    val: 2^n elements;
 *     m_row: 2^s elements, m_col: 2^t elements -- the multiplicities of the indices: m_row[j] = how many entries have row j;
 *   per query (rx, ry), rx of s and ry of t host elements:
 *     e_row[k] = eq(rx, row[k]),  e_col[k] = eq(ry, col[k]): 2^n elements each.  pkx_begin builds them; the caller commits them and
 *     binds their root before any challenge is drawn.
 * THE CLAIM: M~(rx, ry) = sum_k val[k] eq(rx, row[k]) eq(ry, col[k]) = v.
 *
 * THE PROTOCOL
 *   1. the outer transcript has the label "provekit-hip/spark/v1/n<n>/s<s>/t<t>"; it absorbs the n_bind caller elements (the root of
 *      the matrix's commitment and the root of {e_row, e_col}; none: no operation), absorbs rx, then ry -- the statement, absorbed by
 *      both sides and not proof bytes, as pks treats tau -- and squeezes three seeds.  The outer IO pattern: the label, then
 *      A<n_bind>bind, A<s>rx, A<t>ry, S3seeds;
 *   2. side VAL is a pks proof (provekit_sumcheck.h) of the statement (n, m = 3, T = 1, masks = {7}, coefficient 1, no tau,
 *      n_bind = 1) that binds seed 0, over the tables (val, e_row, e_col).  Its s is the claimed value v; it yields the point z_V and
 *      three final values;
 *   3. side ROW is a pkt proof (provekit_tuplelookup.h) of (n, k = s, w = 2, c = 1, n_bind = 1) that binds seed 1: the rows
 *      f = (row, e_row) in the table t = (I_s, eq(rx, .)) under m = m_row, I_s the column 0 .. 2^s - 1: a ROM read of eq(rx, .);
 *   4. side COL is the same of (n, k = t) with (col, e_col), (I_t, eq(ry, .)), m_col, seed 2;
 *   5. the proof is  VAL | ROW | COL,  three whole inner proofs: pks_proof_bytes and the two pkt_proof_bytes, summed, is the length;
 *   6. the verifier runs pks_verify (its expected_sum the expected value: PKS_CHECK_SUM on side VAL) and pkt_verify twice, and adds
 *      one check of its own, numbered after PKF_CHECK_COUNT:
 *        PKX_CHECK_TABLE (side ROW, side COL): the lookup's table claim t_value at its point y equals I(y) + beta eq(rx, y) (ry on
 *            side COL), beta the lookup's own compression challenge and I(y) = sum_j y_j 2^(k-1-j).  The verifier evaluates both
 *            terms itself, O(s): nothing is opened for the table.
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED nine evaluations at five points hold (pkx_claims):
 *     val(z_V), e_row(z_V), e_col(z_V)       = the three final values of side VAL;
 *     row(z_R) + beta_R e_row(z_R)           = the lookup's f_value of side ROW;        m_row(y_R) = its m_value;
 *     col(z_C) + beta_C e_col(z_C)           = the lookup's f_value of side COL;        m_col(y_C) = its m_value.
 * pkx_claims carries the points, the coefficients and the required values; pkx_check_claims forms the combinations from the nine
 * opened evaluations and names the first that fails, so no caller re-derives a coefficient.  e_row and e_col are opened at two points
 * each: one pkw_open with three points (z_V, z_R, z_C) when {e_row, e_col} were committed as one batch.
 *
 * SOUNDNESS.  (a) Side ROW accepted with its claims means every (row[k], e_row[k]) is a row (j, eq(rx, j)) of the table, j < 2^s:
 * e_row[k] = eq(rx, j) for the j < 2^s with row[k] = j in the field -- row[k] is forced to be an index, and e_row[k] the value the
 * sumcheck needs.  Its error is the lookup's (provekit_tuplelookup.h): compression (w - 1) 2^n 2^s / p = 2^(n+s) / p, LogUp
 * (2^n + 2^s) / p, and the two chains: per layer d the layer's sumcheck error 3 d / p and 1 / p for each of lambda_d and rho, over
 * n - 1 and s - 1 layers.  (b) Side COL the same with (n, t): 2^(n+t) / p, (2^n + 2^t) / p, chains of n - 1 and t - 1 layers.  (c) Side
 * VAL: a product sumcheck of degree 3 over n rounds, 3 n / p.  The seeds only separate the three transcripts; rx, ry and the bind
 * elements enter every challenge through them.  The table check is exact: the verifier computes the table's extension itself.
 *
 * ONE QUERY FOR THE THREE R1CS MATRICES: pkx_entries_from_r1cs flattens A, B, C of a pk_r1cs_create input into ONE stacked entry list
 * of 2^(s+2) rows, stacked row = matrix 2^s + row, the fourth block empty.  A verifier that holds three deferred values v_0, v_1, v_2
 * for (rx, ry) draws u (2 elements) AFTER they are fixed and checks the one claim
 *     sum_{g < 3} eq(u, g) v_g = M_stack~((u, rx), ry),     eq(u, g) = prod_i (g's bit (1 - i) ? u_i : 1 - u_i),
 * with one pkx proof of (n, s + 2, t): three wrong values pass with probability at most 2 / p over u (Schwartz-Zippel in u).
 *
 * Out of scope: hiding / zero knowledge; device sets (on a context of a set the prover runs whole on its rank); a device verifier;
 * wiring the query into pk_prove / pkv_verify's wire format; batching several queries in one proof; deriving the indices on the device.
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  The caller's tables are never written.
 */
#ifndef PROVEKIT_SPARK_H
#define PROVEKIT_SPARK_H

#include "provekit_tuplelookup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKX_MAX_VARS 28
#define PKX_MAX_BIND 16
#define PKX_MAX_GRID 1024

/* pks's and pkf's check numbers keep their values; this library's own follows them */
#define PKX_CHECK_TABLE PKF_CHECK_COUNT /* a lookup's table claim is not I(y) + beta eq(rx, y): its table is not (I, eq(rx, .)) */
#define PKX_CHECK_COUNT (PKF_CHECK_COUNT + 1)

/* pkx_verify's side_out */
#define PKX_SIDE_VAL 0
#define PKX_SIDE_ROW 1
#define PKX_SIDE_COL 2

/* the seven device columns of pkx_prove's cols, in this order */
#define PKX_COL_ROW 0
#define PKX_COL_COL 1
#define PKX_COL_VAL 2
#define PKX_COL_M_ROW 3
#define PKX_COL_M_COL 4
#define PKX_COL_E_ROW 5
#define PKX_COL_E_COL 6
#define PKX_COLUMNS 7

/* pkx_check_claims' which_out */
#define PKX_CLAIM_NONE 0 /* all seven combinations of the nine evaluations hold */
#define PKX_CLAIM_VAL 1
#define PKX_CLAIM_E_ROW 2
#define PKX_CLAIM_E_COL 3
#define PKX_CLAIM_ROW 4
#define PKX_CLAIM_M_ROW 5
#define PKX_CLAIM_COL 6
#define PKX_CLAIM_M_COL 7

typedef struct pkx_statement {
    unsigned n;      /* 2^n entries */
    unsigned s;      /* 2^s rows */
    unsigned t;      /* 2^t columns */
    unsigned n_bind; /* caller elements absorbed first */
} pkx_statement;

/* What an accepted proof is accepted PROVIDED of; Montgomery.  Index 0 of the two-sided fields is side ROW, index 1 side COL. */
typedef struct pkx_claims {
    uint64_t value[4];                   /* v: the proof's claimed M~(rx, ry) */
    uint64_t z_val[PKX_MAX_VARS][4];     /* n coordinates, pkw_open's order: z_V, where val, e_row and e_col are opened */
    uint64_t val_values[3][4];           /* val(z_V), e_row(z_V), e_col(z_V) must be these */
    uint64_t beta[2][4];                 /* the two lookups' compression challenges */
    uint64_t z_f[2][PKX_MAX_VARS][4];    /* n coordinates each: z_R, where row and e_row are opened; z_C, for col and e_col */
    uint64_t f_coeff[2][2][4];           /* [side] = (1, beta[side]) */
    uint64_t f_value[2][4];              /* row(z_R) + beta_R e_row(z_R) must be [0]; col(z_C) + beta_C e_col(z_C) must be [1] */
    uint64_t z_m[2][PKX_MAX_VARS][4];    /* s coordinates: y_R, where m_row is opened; t coordinates: y_C, for m_col */
    uint64_t m_value[2][4];              /* m_row(y_R) must be [0]; m_col(y_C) must be [1] */
} pkx_claims;

typedef struct pkx_prover pkx_prover;

int pkx_abi_version(void);
const char *pkx_check_name(int check); /* pkf_check_name's names (which are pks_check_name's, then pkf's own), and "TABLE" */
const char *pkx_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n, s or t outside 1 .. 28, n_bind above 16.  *len is always set to the full length; bytes
 * are copied where they fit. */
int pkx_io_pattern(const pkx_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkx_proof_bytes(const pkx_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds: its own arena (the two eq tables, 2^s + 2^t elements; the index
 * column, 2^max(s, t) elements; 2^s + 2^t u32 counts; the cell of the first bad entry) and the three inner provers' (the pks prover's
 * folded copies, scratch and weights; pkt_prover_arena_bytes of both lookups). */
int pkx_prover_arena_bytes(const pkx_statement *stmt, size_t *bytes);
/* Host only: index ranges of up to 2^this are counted in a workgroup's LDS histogram, larger ones with device-memory atomics. */
unsigned pkx_count_lds_max(void);

/* The prover owns one device arena, sized here, the one pks prover and the two pkt provers (their statements are constant); the
 * index column is written here: its first 2^s entries serve side ROW, its first 2^t side COL.  A proof allocates no device memory.
 * ctx is borrowed: destroy the prover first. */
int pkx_prover_create(pk_ctx *ctx, const pkx_statement *stmt, pkx_prover **out);
int pkx_prover_destroy(pkx_prover *p);
const char *pkx_last_error(const pkx_prover *p);

/* Preprocessing, once per matrix: from the entries' indices d_row_idx, d_col_idx (2^n uint32_t each, device) it writes the caller's
 * device tables d_row_out, d_col_out (2^n elements) and d_m_row_out (2^s), d_m_col_out (2^t).  Every index is validated first: an
 * entry whose row is >= 2^s or whose column is >= 2^t returns PK_ERR_BAD_ARG with *first_bad (may be NULL) = the smallest such entry,
 * also named in the reason, and NOTHING is written to the four outputs: the counting pass, which validates, works in the prover's
 * arena, and the passes that write follow it only when it found no bad entry.  PK_OK: *first_bad = UINT64_MAX.  The inputs are never
 * written.  Blocking. */
int pkx_matrix(pkx_prover *p, const uint32_t *d_row_idx, const uint32_t *d_col_idx, uint64_t *d_row_out, uint64_t *d_col_out, uint64_t *d_m_row_out,
               uint64_t *d_m_col_out, uint64_t *first_bad);

/* Per query: builds eq(rx, .) and eq(ry, .) in the arena (pk_eq_table) and gathers d_e_row_out[k] = eq(rx, row_idx[k]),
 * d_e_col_out[k] = eq(ry, col_idx[k]) (2^n elements each).  rx: s host elements, ry: t, below p.  The indices may come from anywhere
 * and are validated again, in the gather itself, before they are followed: a bad entry returns PK_ERR_BAD_ARG as pkx_matrix does, is
 * read as index 0, and the outputs are not meaningful then (nothing is written outside them).  Blocking. */
int pkx_begin(pkx_prover *p, const uint32_t *d_row_idx, const uint32_t *d_col_idx, const uint64_t *rx, const uint64_t *ry, uint64_t *d_e_row_out,
              uint64_t *d_e_col_out, uint64_t *first_bad);

/* cols: PKX_COLUMNS device pointers on the host, in the order of PKX_COL_*, from pkx_matrix and pkx_begin or anywhere else; bind:
 * n_bind elements.  The eq tables are rebuilt from rx and ry: no state of pkx_begin is kept.  All three sides are proved into host
 * staging the prover owns, and only then is the proof copied out.  An e_row or e_col that is not the gather, a row or col that is no
 * index, or a wrong m is PK_ERR_UNSATISFIED with a reason that names the side and carries pkt_prove's reason ("a row is not in t" with
 * its index, "m is wrong", "a denominator is zero"); it writes nothing and leaves the prover usable.  *len = pkx_proof_bytes, also
 * when cap is too small: PK_ERR_BAD_ARG, nothing proved, the prover stays usable.  value_out (one element: v) and claims_out may be
 * NULL.  Blocking. */
int pkx_prove(pkx_prover *p, const uint64_t *const *cols, const uint64_t *rx, const uint64_t *ry, const uint64_t *bind, uint8_t *proof_out, size_t cap,
              size_t *len, uint64_t *value_out, pkx_claims *claims_out);

/* Host only, no device.  io_pattern NULL: pkx_io_pattern's bytes for stmt.  It checks the framing and the outer transcript, runs
 * pks_verify on VAL (expected_value NULL: any v is taken, and "accepted" holds for the v the proof states, claims_out->value) and
 * pkt_verify on ROW and COL, each followed by PKX_CHECK_TABLE at the end of its side's bytes.  claims_out is written when the proof is
 * accepted.  side_out: PKX_SIDE_*; layer_out: the layer of that side the verdict is about, as pkt_verify's (0 for side VAL, the
 * framing, the outer transcript and this library's own check).  result carries pks's and pkf's check numbers unchanged, and
 * PKX_CHECK_TABLE; its offset counts bytes of the whole proof.  Any of claims_out, side_out, layer_out may be NULL. */
int pkx_verify(const pkx_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *rx, const uint64_t *ry,
               const uint64_t *bind, const uint64_t *expected_value_or_null, const uint8_t *proof, size_t len, pkx_claims *claims_out, int *side_out,
               unsigned *layer_out, pkv_result *result);

/* Host only: the seven combinations of the nine evaluations.  val_evals: 3 elements, (val, e_row, e_col)(z_val); row_evals: 2 elements,
 * (row, e_row)(z_f[0]); m_row_eval: m_row(z_m[0]); col_evals: (col, e_col)(z_f[1]); m_col_eval: m_col(z_m[1]); all Montgomery, below
 * p.  PK_OK with *which_out = PKX_CLAIM_NONE when all hold, else the first that does not, in the order of PKX_CLAIM_*.  PK_ERR_BAD_ARG
 * with a reason: a bad statement, a null pointer, an element not below p. */
int pkx_check_claims(const pkx_statement *stmt, const pkx_claims *claims, const uint64_t *val_evals, const uint64_t *row_evals, const uint64_t *m_row_eval,
                     const uint64_t *col_evals, const uint64_t *m_col_eval, int *which_out);

/* Host only: the three CSR matrices and the interner of a pk_r1cs_create input as ONE stacked entry list (see above): entry k of
 * matrix g's row r with column c and value index i becomes (g 2^s + r, c, interner[i]), matrices in order, each in CSR order; the
 * rest up to 2^n is padding (0, 0, 0).  2^s >= num_constraints, 2^t >= num_witnesses, 2^n >= the three nnz summed: anything else, a
 * row offset that decreases or exceeds nnz, a column >= num_witnesses or a value index >= n_interned is PK_ERR_BAD_ARG with a reason.
 * row_idx_out, col_idx_out: 2^n uint32_t each; val_out: 2^n elements; all host memory.  The statement of the query is (n, s + 2, t). */
int pkx_entries_from_r1cs(size_t num_constraints, size_t num_witnesses, const pk_sparse_matrix mats[3], const uint64_t *interner, size_t n_interned, unsigned n,
                          unsigned s, unsigned t, uint32_t *row_idx_out, uint32_t *col_idx_out, uint64_t *val_out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_SPARK_H */
