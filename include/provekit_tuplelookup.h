/*
 * provekit_tuplelookup.h -- C ABI of libprovekit_tuplelookup.so: tuple and multi-column LogUp-GKR lookups.
 *
 * A ninth library above the product's C ABI: it links libprovekit_hip.so, libprovekit_sumcheck.so (transitively) and
 * libprovekit_fracsum.so, calls only what provekit_hip.h and provekit_fracsum.h declare (of the product: pk_malloc, pk_free,
 * pk_ctx_sync), and adds one HIP kernel family of its own for gfx950 (csrc/tuplelookup/tuple.hip).  It links neither
 * libprovekit_whir.so nor the verify, lookup or grandproduct libraries: committing and opening the columns is the caller's
 * composition (examples/tuplelookup_pcs_demo.cpp).
 *
 * THE STATEMENT: n, k, w, c, n_bind.  w (1 .. 4) is the number of columns of a row; c (1, 2 or 4) the number of column groups looked
 * up in the one table; n and k are 1 .. 28 with n + log2 c <= 28; n_bind is 0 .. 16.  The device tables, Montgomery form, below p:
 *     f[g][j], g < c, j < w: 2^n elements each -- group g's column j;
 *     t[j], j < w: 2^k elements each -- the table's column j;
 *     m: 2^k elements -- m[y] = how many rows of all c groups equal row y of t.
 * The claim: every row (f[g][0][x], .., f[g][w-1][x]) is a row (t[0][y], .., t[w-1][y]) of t.  A ROM read is w = 2, rows
 * (addr, value); a binop table is w = 3, rows (a, b, a op b); c columns range-checked against one table are w = 1 and c groups.
 *
 * THE PROTOCOL (LogUp over rows compressed by a challenge, proved by two GKR fractional sums of provekit_fracsum.h):
 *   1. the outer transcript has the label "provekit-hip/tuple-lookup/v1/n<n>/k<k>/w<w>/c<c>";
 *   2. it absorbs the n_bind caller elements (the roots of the commitments to f, t and m; none: no operation);
 *   3. it squeezes alpha; when w > 1 it squeezes beta, and beta = 1 without an operation when w = 1 (as pkg_multiset does); it
 *      squeezes two seeds.  The outer IO pattern: the label, then A<n_bind>bind, S1alpha, [S1beta], S2seeds;
 *   4. the leaves:   leafF[g 2^n + x] = alpha - sum_j beta^j f[g][j][x],  the c groups stacked into ONE table of 2^(n + log2 c) entries,
 *                    leafT[y]         = alpha - sum_j beta^j t[j][y];
 *   5. the proof is  side F | side T:  side F is a pkf fractional sum of the statement (n + log2 c, unit = 1) over q = leafF, side T
 *      one of (k, unit = 0) with p = m and q = leafT; each side has n_bind = 1 and binds its seed.  Both are whole pkf proofs:
 *      pkf_proof_bytes of the two statements, summed, is the length;
 *   6. the verifier requires P_F Q_T = P_T Q_F: PKF_CHECK_FRACTION, reported on side T.  There are no new check numbers:
 *      pkt_check_name answers pkf_check_name's names.
 * Variable 0 is the most significant index bit (pks's, pkf's and pkw_open's convention), so the first log2 c coordinates of side F's
 * point select the group: z_F = (z_hi, z_lo), z_hi of log2 c coordinates and z_lo of n, and
 *     leafF~(z_F) = alpha - sum_{g, j} eq(z_hi, g) beta^j f[g][j]~(z_lo),    eq(z_hi, g) = prod_i (g's bit (log2 c - 1 - i) ? z_hi[i] : 1 - z_hi[i]).
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED three claims hold (pkt_claims), cq_F, cq_T and cp_T being the two chains' last claims:
 *     sum_{g, j} eq(z_hi, g) beta^j f[g][j](z_lo) = alpha - cq_F,
 *     sum_j beta^j t[j](z_T) = alpha - cq_T,
 *     m(z_T) = cp_T.
 * pkt_claims carries alpha, beta, z_lo, z_T, the c x w coefficients eq(z_hi, g) beta^j, the w coefficients beta^j and the three
 * required values.  One pkw_open (provekit_whir.h) per committed group at z_lo and one of {t[0], .., t[w-1], m} at z_T give the
 * evaluations; pkt_check_claims forms the three combinations, so no caller re-derives a coefficient.  All columns are committed in
 * ONE phase, before alpha and beta.
 *
 * SOUNDNESS.  (a) Compression: two different rows of w columns compress to the same value for at most w - 1 values of beta, so over
 * the c 2^n + 2^k rows of both sides some row outside t collides with a row of t with probability at most
 * (w - 1) c 2^n 2^k / p (a union over pairs; nothing at w = 1).  (b) LogUp: when the multiset of compressed rows of f is not inside
 * that of t under m, the rational identity sum_x 1 / (X - leafF'[x]) = sum_y m[y] / (X - leafT'[y]) fails as an identity and holds at
 * a random alpha with probability at most (c 2^n + 2^k) / p -- the term over c 2^n + 2^k rows.  A zero denominator (alpha is a
 * compressed row) is rejected, not divided by.  (c) The two chains: per layer d of each side the layer's sumcheck error 3 d / p and
 * 1 / p for each of lambda_d and rho (provekit_fracsum.h), over n + log2 c - 1 and k - 1 layers.  The seeds only separate the two
 * chains' transcripts.
 *
 * Out of scope: hiding / zero knowledge; device sets (on a context of a set the prover runs whole on its rank); deriving idx on the
 * device (the caller knows where its rows are); rows wider than 4 columns or more than 4 groups; tables of different widths in one
 * proof; a device verifier; proving the small layers on the host.
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  The caller's tables are never written.
 */
#ifndef PROVEKIT_TUPLELOOKUP_H
#define PROVEKIT_TUPLELOOKUP_H

#include "provekit_fracsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKT_MAX_VARS 28
#define PKT_MAX_BIND 16
#define PKT_MAX_WIDTH 4
#define PKT_MAX_GROUPS 4
#define PKT_MAX_GRID 1024

/* pkt_verify's side_out: provekit_fracsum.h's */
#define PKT_SIDE_F PKF_SIDE_F
#define PKT_SIDE_T PKF_SIDE_T

/* pkt_check_claims' which_out */
#define PKT_CLAIM_NONE 0 /* all three hold */
#define PKT_CLAIM_F 1
#define PKT_CLAIM_T 2
#define PKT_CLAIM_M 3

typedef struct pkt_statement {
    unsigned n;      /* a column of a group: 2^n entries */
    unsigned k;      /* a column of the table, and m: 2^k entries */
    unsigned w;      /* columns of a row, 1 .. 4 */
    unsigned c;      /* column groups, 1, 2 or 4 */
    unsigned n_bind; /* caller elements absorbed first */
} pkt_statement;

/* What an accepted proof is accepted PROVIDED of; Montgomery.  The required values are already alpha - cq. */
typedef struct pkt_claims {
    uint64_t alpha[4];
    uint64_t beta[4];                                    /* 1 when w = 1 */
    uint64_t z_lo[PKT_MAX_VARS][4];                      /* n coordinates, pkw_open's order: where every f[g][j] is opened */
    uint64_t z_t[PKT_MAX_VARS][4];                       /* k coordinates: where every t[j] and m are opened */
    uint64_t f_coeff[PKT_MAX_GROUPS][PKT_MAX_WIDTH][4];  /* [g][j] = eq(z_hi, g) beta^j for g < c, j < w; 0 elsewhere */
    uint64_t t_coeff[PKT_MAX_WIDTH][4];                  /* [j] = beta^j for j < w; 0 elsewhere */
    uint64_t f_value[4];                                 /* sum_{g, j} f_coeff[g][j] f[g][j](z_lo) must be this */
    uint64_t t_value[4];                                 /* sum_j t_coeff[j] t[j](z_t) must be this */
    uint64_t m_value[4];                                 /* m(z_t) must be this */
} pkt_claims;

typedef struct pkt_prover pkt_prover;

int pkt_abi_version(void);
const char *pkt_check_name(int check); /* pkf_check_name's names: no check of this library's own */
const char *pkt_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n or k outside 1 .. 28, w outside 1 .. 4, c not 1, 2 or 4, n + log2 c above 28, n_bind
 * above 16.  *len is always set to the full length; bytes are copied where they fit. */
int pkt_io_pattern(const pkt_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkt_proof_bytes(const pkt_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds: its own arena (the two leaf tables, 2^(n + log2 c) + 2^k elements,
 * 2^k u32 counts and the cell of the first bad row) and the two pkf provers' (pkf_prover_arena_bytes of both sides). */
int pkt_prover_arena_bytes(const pkt_statement *stmt, size_t *bytes);
/* Host only: tables of up to 2^this entries are counted in a workgroup's LDS histogram, larger ones with device-memory atomics. */
unsigned pkt_count_lds_max_k(void);

/* The prover owns one device arena, sized here, and the two pkf provers (their statements are constant).  A proof allocates no
 * device memory.  ctx is borrowed: destroy the prover first. */
int pkt_prover_create(pk_ctx *ctx, const pkt_statement *stmt, pkt_prover **out);
int pkt_prover_destroy(pkt_prover *p);
const char *pkt_last_error(const pkt_prover *p);

/* The multiplicities of t under the c groups.  d_f: c * w device pointers on the host, d_f[g * w + j] = f[g][j]; d_t: w device
 * pointers; d_idx: c device pointers, idx[g] 2^n uint32_t with row x of group g = row idx[g][x] of t; d_m_out: 2^k elements.  Every
 * index is validated on the device before it is followed (idx[g][x] < 2^k), and every row is compared with the row it names, all w
 * columns, on the stored words.  A failure returns PK_ERR_UNSATISFIED with *first_bad (may be NULL) = the smallest stacked index
 * g 2^n + x that fails; d_m_out is not meaningful then.  PK_OK: *first_bad = UINT64_MAX.  Blocking. */
int pkt_multiplicities(pkt_prover *p, const uint64_t *const *d_f, const uint64_t *const *d_t, const uint32_t *const *d_idx, uint64_t *d_m_out,
                       uint64_t *first_bad);

/* The leaf kernel by itself (tests, benchmarks): d_cols: c * w device pointers on the host, d_cols[g * w + j] 2^n elements;
 * d_leaf_out[g 2^n + x] = alpha - sum_j beta^j d_cols[g * w + j][x], c 2^n elements.  alpha, beta: one host element each.  n 1 .. 28,
 * w 1 .. 4, c 1, 2 or 4 (any c 2^n the caller has room for).  Blocking. */
int pkt_leaves(pk_ctx *ctx, unsigned n, unsigned w, unsigned c, const uint64_t *const *d_cols, const uint64_t *alpha, const uint64_t *beta,
               uint64_t *d_leaf_out);

/* d_f, d_t as for pkt_multiplicities; d_m: 2^k elements, from pkt_multiplicities or anywhere else; bind: n_bind elements.  Both
 * sides are proved into host staging the prover owns and their fractions compared before a byte of proof_out is written.
 * PK_ERR_UNSATISFIED with a reason that names the case -- "a denominator is zero" (alpha is a compressed row of f or of t), "a row is
 * not in t" (with the smallest stacked index of such a row) or "m is wrong" (every row is in t, the fractions differ all the same) --
 * writes nothing and leaves the prover usable.  *len = pkt_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG, nothing proved, the
 * prover stays usable.  claims_out may be NULL.  Blocking. */
int pkt_prove(pkt_prover *p, const uint64_t *const *d_f, const uint64_t *const *d_t, const uint64_t *d_m, const uint64_t *bind, uint8_t *proof_out,
              size_t cap, size_t *len, pkt_claims *claims_out);

/* Host only, no device.  io_pattern NULL: pkt_io_pattern's bytes for stmt.  It checks the framing and the outer transcript, runs
 * pkf_verify on each side and compares the two fractions.  claims_out is written when the proof is accepted.  side_out: PKT_SIDE_*;
 * layer_out: the layer of that side the verdict is about, as pkf_verify's (0 also for the framing, the outer transcript and the
 * comparison of the two fractions, which names side T).  result carries pkf's check numbers unchanged; its offset counts bytes of
 * the whole proof.  Any of claims_out, side_out, layer_out may be NULL. */
int pkt_verify(const pkt_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind, const uint8_t *proof,
               size_t len, pkt_claims *claims_out, int *side_out, unsigned *layer_out, pkv_result *result);

/* Host only: the three combinations.  f_evals: c * w elements, f_evals[g * w + j] = f[g][j](z_lo); t_evals: w elements, t[j](z_t);
 * m_eval: m(z_t); all Montgomery, below p.  PK_OK with *which_out = PKT_CLAIM_NONE when all three hold, else the first that does not
 * (PKT_CLAIM_F, _T, _M).  PK_ERR_BAD_ARG with a reason: a bad statement, a null pointer, an element not below p. */
int pkt_check_claims(const pkt_statement *stmt, const pkt_claims *claims, const uint64_t *f_evals, const uint64_t *t_evals, const uint64_t *m_eval,
                     int *which_out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_TUPLELOOKUP_H */
