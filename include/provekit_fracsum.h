/*
 * provekit_fracsum.h -- C ABI of libprovekit_fracsum.so: GKR fractional sums and LogUp lookups without helper columns.
 *
 * An eighth library above the product's C ABI: it links libprovekit_hip.so and libprovekit_sumcheck.so, calls only what
 * provekit_hip.h and provekit_sumcheck.h declare, and adds one HIP kernel family of its own for gfx950 (csrc/fracsum/tree.hip).
 * It links neither libprovekit_whir.so nor the verify, lookup or grandproduct libraries: committing and opening the tables is the
 * caller's composition (examples/fracsum_pcs_demo.cpp).  A proof costs NO commitment beyond the input tables and NO field inversion.
 *
 * 1. THE FRACTIONAL SUM.  The statement: n (1 .. 28), n_bind (0 .. 16), unit (0 or 1); q a device table of 2^n elements, Montgomery
 * form, below p; p a device table of 2^n elements when unit = 0; with unit = 1 there is no p and every numerator is 1.  The claim is
 *     sum_x p[x] / q[x] = P / Q,
 * stated projectively as the pair (P, Q): nothing divides, zero numerators are legal, a zero denominator anywhere gives Q = 0.
 *
 * The layers of the two trees: (p_n, q_n) = (p, q), and for d = n-1 .. 0 and x < 2^d
 *     p_d[x] = p_{d+1}[x] q_{d+1}[x + 2^d] + p_{d+1}[x + 2^d] q_{d+1}[x],        q_d[x] = q_{d+1}[x] q_{d+1}[x + 2^d];
 * (P, Q) = (p_0[0], q_0[0]).  With variable 0 <-> the most significant index bit (pks's and pkw_open's convention) the two children of
 * a layer are the two contiguous halves of layer d + 1: pL[x] = p_{d+1}[x], pR[x] = p_{d+1}[x + 2^d], likewise qL, qR.  The prover
 * keeps both trees in heap layout, tree[2^d + x] = layer d's entry x (2^n elements each, index 0 unused; layer n is the caller's).
 *
 * The protocol (GKR over a tree of fractions: Papini and Haboeck, "Improving logarithmic derivative lookups using GKR", eprint
 * 2023/1284):
 *   1. the outer transcript has the label "provekit-hip/fracsum/v1/n<n>/u<unit>";
 *   2. it absorbs the n_bind caller elements (none: no operation), then the four values p_1[0], p_1[1], q_1[0], q_1[1] ("top");
 *   3. the verifier forms P = p_1[0] q_1[1] + p_1[1] q_1[0] and Q = q_1[0] q_1[1]; it rejects Q = 0 (PKF_CHECK_DENOMINATOR) and, given an
 *      expected fraction (num, den), requires P den = num Q (PKF_CHECK_FRACTION);
 *   4. it squeezes rho_1; the running claims are cp_1 = (1 - rho_1) p_1[0] + rho_1 p_1[1] and cq_1 likewise, at z_1 = (rho_1);
 *   5. for d = 1 .. n-1: it squeezes lambda_d, then seed_d.  The prover forms u_d[x] = pR[x] + lambda_d qR[x] (2^d elements of its
 *      arena) and makes one pks proof (provekit_sumcheck.h) of the statement n = d, m = 4, T = 2, masks {5, 10} (pL qR and qL u_d),
 *      coefficients {1, 1}, has_tau = 1, n_bind = 1 with tables {pL, qL, qR, u_d}, tau = z_d, bind = {seed_d} and expected sum
 *      cp_d + lambda_d cq_d.  Folding lambda into a table keeps every layer's coefficients constant: the n - 1 pks provers are made
 *      once with the prover.  With that proof's finals (a, b, c, e) -- read from the inner proof, not repeated -- the outer
 *      transcript absorbs the four finals and squeezes rho_{d+1}; the claims become
 *          cp_{d+1} = (1 - rho) a + rho (e - lambda_d c),      cq_{d+1} = (1 - rho) b + rho c      at z_{d+1} = (rho_{d+1}, r_d),
 *      r_d the inner proof's point: the new coordinate comes first, it is the most significant bit of the child layer.
 * unit = 1: the layers d < n-1 are as above.  The last one (d = n-1, its children are the leaves) has m = 3: tables {qL, qR, u} with
 * u = 1 + lambda qR, masks {2, 5}, coefficients {1, 1}; three finals (b, c, e) are absorbed; the verifier requires e = 1 + lambda c
 * (PKF_CHECK_UNIT) and no p claim remains.  At n = 1 both top numerators must be 1 (the same check).
 * The outer IO pattern: the label, then A<n_bind>bind, A4top, S1rho, and per d: S1lambda, S1seed, A4finals (A3finals), S1rho.
 *
 * The proof is   top (128 bytes) | pks proof 1 | .. | pks proof n-1:   128 + (n - 1)(48 n + 160) bytes for unit = 0, and 32 less for
 * unit = 1 with n >= 2 (pks_proof_bytes of every layer's statement, summed).
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED q(z_n) = cq_n and, for unit = 0, p(z_n) = cp_n; z_n in pkw_open's coordinate order.
 * pkf_verify writes P, Q, z_n and the claims; pkw_open / pkw_verify (provekit_whir.h) establish them for committed tables.
 * Soundness: per layer d the sumcheck's error (3 d / p, its zero check's tau included) and 1 / p for each of lambda_d and rho.
 *
 * 2. THE LOOKUP on top of it (LogUp-GKR).  The statement: n, k (1 .. 28 each, independent), n_bind; device tables f (2^n), t (2^k) and
 * m (2^k), m the multiplicities: m[j] = how often t[j] occurs in f.  pkl_multiplicities (provekit_lookup.h) produces and validates
 * them, or the caller makes them any other way; this library neither needs nor reads an index column.  The claim: every entry of f is
 * an entry of t.  The outer transcript: the label "provekit-hip/logup-gkr/v1/n<n>/k<k>", absorb n_bind elements (the roots of f, t,
 * m), squeeze alpha, squeeze two seeds.  Pattern: A<n_bind>bind, S1alpha, S2seeds.  The proof is
 *     fractional sum F of (n, unit = 1), q = alpha - f  |  fractional sum T of (k, unit = 0), p = m, q = alpha - t,
 * each with n_bind = 1 and bind = {its seed}; the verifier requires P_F Q_T = P_T Q_F (PKF_CHECK_FRACTION, side T).  Accepted
 * PROVIDED three claims (pkf_lookup_claims):   f(z_F) = alpha - cq_F,   t(z_T) = alpha - cq_T,   m(z_T) = cp_T:
 * one pkw_open of f at z_F and one of {t, m} at z_T establish them.  f, t and m are committed in ONE phase, before alpha.
 * Soundness: LogUp's (2^n + 2^k) / p, and the two chains' errors.
 *
 * Out of scope: hiding / zero knowledge; device sets (on a context of a set the prover runs whole on its rank); several columns per
 * table or tuple lookups in one chain; a device verifier; proving the small layers on the host; a count-only entry point for m.
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  The caller's tables are never written.
 */
#ifndef PROVEKIT_FRACSUM_H
#define PROVEKIT_FRACSUM_H

#include "provekit_sumcheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKF_MAX_VARS 28
#define PKF_MAX_BIND 16
#define PKF_MAX_GRID 1024

/* The verifier core's and pks's check numbers keep their values; this library's own follow them.  PKF_CHECK_FRACTION has the value
 * PKG_CHECK_PRODUCT has in provekit_grandproduct.h: the two libraries number their own checks independently, use each library's
 * own *_check_name. */
#define PKF_CHECK_FRACTION PKS_CHECK_COUNT          /* P / Q is not the expected fraction / the two sides' fractions differ */
#define PKF_CHECK_DENOMINATOR (PKS_CHECK_COUNT + 1) /* Q = 0: some denominator is zero */
#define PKF_CHECK_UNIT (PKS_CHECK_COUNT + 2)        /* unit = 1: a numerator that must be 1 is not */
#define PKF_CHECK_COUNT (PKS_CHECK_COUNT + 3)

/* pkf_lookup_verify's side_out */
#define PKF_SIDE_F 0
#define PKF_SIDE_T 1

typedef struct pkf_statement {
    unsigned n;      /* the tables: 2^n entries */
    unsigned n_bind; /* caller elements absorbed first */
    unsigned unit;   /* 1: no numerator table, every numerator is 1 */
} pkf_statement;

typedef struct pkf_lookup_statement {
    unsigned n;      /* the column f: 2^n entries */
    unsigned k;      /* the table t and its multiplicities m: 2^k entries */
    unsigned n_bind; /* caller elements absorbed first */
} pkf_lookup_statement;

/* What an accepted lookup proof is accepted PROVIDED of; Montgomery.  The required values are already alpha - cq. */
typedef struct pkf_lookup_claims {
    uint64_t alpha[4];
    uint64_t z_f[PKF_MAX_VARS][4]; /* n coordinates, pkw_open's order */
    uint64_t z_t[PKF_MAX_VARS][4]; /* k coordinates */
    uint64_t f_value[4];           /* f(z_f) must be this */
    uint64_t t_value[4];           /* t(z_t) must be this */
    uint64_t m_value[4];           /* m(z_t) must be this */
} pkf_lookup_claims;

typedef struct pkf_prover pkf_prover;
typedef struct pkf_lookup_prover pkf_lookup_prover;

int pkf_abi_version(void);
const char *pkf_check_name(int check); /* pks_check_name's names, and "FRACTION", "DENOMINATOR", "UNIT" */
const char *pkf_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n outside 1 .. 28, n_bind above 16, unit above 1.  *len is always set to the full length;
 * bytes are copied where they fit. */
int pkf_io_pattern(const pkf_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkf_proof_bytes(const pkf_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds: two trees (2^n elements each), the combined table u (2^(n-1)) and
 * its n - 1 pks provers' arenas. */
int pkf_prover_arena_bytes(const pkf_statement *stmt, size_t *bytes);
/* Host only: t.  Once a layer has at most 2^t entries, one workgroup finishes all remaining layers of both trees out of LDS. */
unsigned pkf_tail_max_n(void);

/* The prover owns one device arena, sized here, and n - 1 pks provers (their statements are constant).  A proof allocates nothing.
 * ctx is borrowed: destroy the prover first. */
int pkf_prover_create(pk_ctx *ctx, const pkf_statement *stmt, pkf_prover **out);
int pkf_prover_destroy(pkf_prover *p);
const char *pkf_last_error(const pkf_prover *p);

/* The tree kernels by themselves (tests, benchmarks): d_p (NULL: unit) and d_q 2^n elements; d_ptree_out and d_qtree_out 2^n
 * elements each, written in heap layout (tree[2^d + x] for d < n; element 0 is not written); fraction_out: P then Q, two host
 * elements.  n 1 .. 28.  Blocking. */
int pkf_tree(pk_ctx *ctx, unsigned n, const uint64_t *d_p_or_null, const uint64_t *d_q, uint64_t *d_ptree_out, uint64_t *d_qtree_out,
             uint64_t *fraction_out);

/* d_p: NULL exactly when unit = 1; bind: n_bind elements.  *len = pkf_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG,
 * nothing proved, the prover stays usable.  Q = 0 returns PK_ERR_UNSATISFIED with a reason: nothing is written and the prover stays
 * usable.  fraction_out (2 elements: P, Q), point_out (n elements: z_n), value_p_out (cp_n; not written when unit = 1) and
 * value_q_out (cq_n) may be NULL.  Blocking. */
int pkf_prove(pkf_prover *p, const uint64_t *d_p_or_null, const uint64_t *d_q, const uint64_t *bind, uint8_t *proof_out, size_t cap, size_t *len,
              uint64_t *fraction_out, uint64_t *point_out, uint64_t *value_p_out, uint64_t *value_q_out);

/* Host only, no device.  io_pattern NULL: pkf_io_pattern's bytes for stmt.  expected_fraction NULL: any P / Q with Q != 0 is taken;
 * else two elements (num, den).  fraction_out (2), point_out (n), value_p_out (unit = 0 only), value_q_out are written when the proof
 * is accepted (each may be NULL).  layer_out (may be NULL): the layer d the verdict is about, 0 for the outer framing, the top and the
 * transcript.  result carries the verifier core's and pks's check numbers unchanged, and PKF_CHECK_*; its offset counts bytes of the
 * whole proof. */
int pkf_verify(const pkf_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind,
               const uint64_t *expected_fraction_or_null, const uint8_t *proof, size_t len, uint64_t *fraction_out, uint64_t *point_out,
               uint64_t *value_p_out, uint64_t *value_q_out, unsigned *layer_out, pkv_result *result);

/* Host only.  PK_ERR_BAD_ARG with a reason: n or k outside 1 .. 28, n_bind above 16. */
int pkf_lookup_io_pattern(const pkf_lookup_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkf_lookup_proof_bytes(const pkf_lookup_statement *stmt, size_t *len);
/* Host only: the two sides' provers (pkf_prover_arena_bytes of (n, unit = 1) and (k, unit = 0)) and their leaf tables (2^n + 2^k). */
int pkf_lookup_prover_arena_bytes(const pkf_lookup_statement *stmt, size_t *bytes);

/* One pkf_prover and one leaf table per side: both sides' trees stand when the two fractions are compared. */
int pkf_lookup_prover_create(pk_ctx *ctx, const pkf_lookup_statement *stmt, pkf_lookup_prover **out);
int pkf_lookup_prover_destroy(pkf_lookup_prover *p);
const char *pkf_lookup_last_error(const pkf_lookup_prover *p);

/* d_f: 2^n elements; d_t, d_m: 2^k elements each; bind: n_bind elements.  Both roots are computed before anything is written: a zero
 * denominator (alpha is an entry of f or t) and P_F Q_T != P_T Q_F (f is not inside t under m, or m is wrong) return
 * PK_ERR_UNSATISFIED with a reason that names which it was, nothing is written and the prover stays usable.  *len as for pkf_prove.
 * claims_out may be NULL.  Blocking. */
int pkf_lookup_prove(pkf_lookup_prover *p, const uint64_t *d_f, const uint64_t *d_t, const uint64_t *d_m, const uint64_t *bind, uint8_t *proof_out,
                     size_t cap, size_t *len, pkf_lookup_claims *claims_out);

/* Host only, no device.  claims_out is written when the proof is accepted.  side_out: PKF_SIDE_*; layer_out as for pkf_verify (0
 * also for the outer transcript of the lookup and for the comparison of the two fractions, which names side T). */
int pkf_lookup_verify(const pkf_lookup_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind,
                      const uint8_t *proof, size_t len, pkf_lookup_claims *claims_out, int *side_out, unsigned *layer_out, pkv_result *result);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_FRACSUM_H */
