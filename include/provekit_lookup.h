/*
 * provekit_lookup.h -- C ABI of libprovekit_lookup.so: LogUp lookup arguments over device-resident tables.
 *
 * A sixth library above the product's C ABI: it links libprovekit_hip.so and libprovekit_sumcheck.so, calls only what provekit_hip.h
 * and provekit_sumcheck.h declare, and adds one HIP kernel family of its own for gfx950 (csrc/lookup/lookup.hip).  It does not link
 * libprovekit_whir.so: committing and opening the tables is the caller's composition, as for pks (examples/sumcheck_pcs_demo.cpp).
 *
 * The statement: a column f of 2^n values and a table t of 2^k values (1 <= n, k <= 28, independent of each other; k may exceed n;
 * entries of t need not be distinct), both in device memory and in CANONICAL Montgomery form (below p).  The claim is
 *
 *     { f[x] } is a subset of { t[y] }.
 *
 * The prover also takes idx, 2^n uint32_t in device memory, with f[x] = t[idx[x]]: a prover-side hint that turns the 2^n inversions
 * of the f side into a gather.  Equality is tested on the stored words, so two representatives of one value (v and v + p) are
 * refused: that errs on the safe side.
 *
 * The protocol is LogUp (Haboeck, eprint 2022/1530) with helper columns, arranged so that both sumcheck statements have constant
 * coefficients:
 *   1. multiplicities: m[y] = #{x : idx[x] = y} (at most 2^n <= 2^28), a table of 2^k field elements.  Every index is validated on
 *      the device first: idx[x] < 2^k and f[x] == t[idx[x]]; the smallest failing x is reported and nothing is proved.
 *   2. the caller commits f, t, m however it likes; the outer transcript absorbs n_bind caller elements (0 .. 16; the roots as field
 *      elements) and squeezes alpha.
 *   3. helper tables: d_t = alpha - t, g = 1 / d_t, h_t = m g (2^k each); h_f[x] = g[idx[x]], d_f[x] = d_t[idx[x]] (2^n each): a
 *      proof costs 2^k inversions, not 2^n.  A zero d_t[y] means alpha hit the table (probability 2^k / p): the call fails with a
 *      reason and the prover stays usable.
 *   4. the caller commits h_f and h_t; the transcript absorbs n_bind2 elements (0 .. 16), absorbs s = sum_y h_t[y] and squeezes
 *      tau_f (n elements), tau_t (k elements) and one seed sigma.
 *   5. two pks proofs (provekit_sumcheck.h), each with bind = {sigma} and its own tau:
 *        F: tables {h_f, d_f}, m = 2, T = 1, mask 3, coefficient 1, expected sum 1:    sum_x eq(tau_f, x) h_f d_f = 1
 *        T: tables {h_t, d_t, m}, m = 3, T = 2, masks {3, 4}, coefficients {1, -1}, expected sum 0:
 *                                                                                      sum_y eq(tau_t, y) (h_t d_t - m) = 0
 *
 * The proof is   s | pks proof F | pks proof T   (pkl_proof_bytes = 32 + pks_proof_bytes of each).
 *
 * The outer IO pattern: the label "provekit-hip/lookup/v1/n<n>/k<k>", then A<n_bind>bind, S1alpha, A<n_bind2>helpers, A1sum,
 * S<n>tau_f, S<k>tau_t, S1seed.  An absorb of zero elements is no operation, as in pks.
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED seven evaluation claims hold, which pkl_verify writes out (pkl_claims) and which
 * pkw_open / pkw_verify (provekit_whir.h) establish for committed tables:
 *     at r_f:                   h_f = v_0  and  f = alpha - v_1            (v: the F proof's finals)
 *     at r_t:                   h_t = w_0,  t = alpha - w_1  and  m = w_2  (w: the T proof's finals)
 *     at (1/2, .., 1/2) in F^n: h_f = s 2^-n
 *     at (1/2, .., 1/2) in F^k: h_t = s 2^-k
 * The last two use sum_x h(x) = 2^n h~(1/2, .., 1/2): the equality of the two sums costs no third sumcheck.  d_f and d_t are never
 * committed: their extensions are alpha minus those of f and t.
 *
 * Soundness: the LogUp identity sum_x 1/(X - f[x]) = sum_y m[y]/(X - t[y]) fails at a random alpha with probability at most
 * (2^n + 2^k) / p when the claim is false; to that add the two sumchecks' errors (n * 2 / p and k * 3 / p over the zero checks' tau).
 * NOT proved: anything about idx, which is a hint only and appears in no claim; that m is a table of small integers (the identity
 * does not need it in a field of characteristic > 2^n).
 *
 * Out of scope: hiding / zero knowledge; several columns against one table in one proof; vector-valued (tuple) lookups; deriving idx
 * on the device; device sets (on a context of a set the prover runs whole on its rank; nothing is sharded); a batched device verifier.
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A pkl_prover is single-caller.  The caller's f, t and idx are never written.
 */
#ifndef PROVEKIT_LOOKUP_H
#define PROVEKIT_LOOKUP_H

#include "provekit_sumcheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKL_MAX_VARS 28
#define PKL_MAX_BIND 16
#define PKL_MAX_GRID 1024

/* pkl_verify's side_out: which part of the proof the verdict is about */
#define PKL_SIDE_OUTER 0 /* framing and the outer transcript */
#define PKL_SIDE_F 1     /* the pks proof of the f side */
#define PKL_SIDE_T 2     /* the pks proof of the t side */

typedef struct pkl_statement {
    unsigned n;       /* the column: 2^n values */
    unsigned k;       /* the table: 2^k values */
    unsigned n_bind;  /* caller elements absorbed before alpha */
    unsigned n_bind2; /* caller elements absorbed after the helper tables exist */
} pkl_statement;

/* What an accepted proof is accepted PROVIDED of; Montgomery.  The derived values (alpha - v, s 2^-n) are already computed. */
typedef struct pkl_claims {
    uint64_t alpha[4];
    uint64_t s[4];
    uint64_t r_f[PKL_MAX_VARS][4]; /* n coordinates, pkw_open's order */
    uint64_t r_t[PKL_MAX_VARS][4]; /* k coordinates */
    uint64_t hf_at_rf[4];          /* h_f(r_f) */
    uint64_t f_at_rf[4];           /* f(r_f) */
    uint64_t ht_at_rt[4];          /* h_t(r_t) */
    uint64_t t_at_rt[4];           /* t(r_t) */
    uint64_t m_at_rt[4];           /* m(r_t) */
    uint64_t hf_at_half[4];        /* h_f(1/2, .., 1/2) */
    uint64_t ht_at_half[4];        /* h_t(1/2, .., 1/2) */
} pkl_claims;

typedef struct pkl_prover pkl_prover;

int pkl_abi_version(void);
const char *pkl_create_error(void); /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n or k outside 1 .. 28, n_bind or n_bind2 above 16.  *len is always set to the full
 * length; bytes are copied where they fit. */
int pkl_io_pattern(const pkl_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkl_proof_bytes(const pkl_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds, its two pks provers' arenas included. */
int pkl_prover_arena_bytes(const pkl_statement *stmt, size_t *bytes);
/* Host only: the largest k whose multiplicities are counted in a workgroup-private LDS histogram; larger tables count in device memory. */
unsigned pkl_count_lds_max_k(void);
/* Host only: the largest k whose two source tables the gather stages in LDS; larger tables are gathered through L2. */
unsigned pkl_gather_lds_max_k(void);

/* The prover owns one device arena, sized here: 2 * 2^n + 3 * 2^k elements (h_f, d_f; d_t, g, h_t), 2^k u32 counts and the partial
 * sums; and the two pks provers.  A proof allocates nothing.  ctx is borrowed: destroy the prover first. */
int pkl_prover_create(pk_ctx *ctx, const pkl_statement *stmt, pkl_prover **out);
int pkl_prover_destroy(pkl_prover *p);
const char *pkl_last_error(const pkl_prover *p);

/* Step 1.  d_f: 2^n elements, d_t: 2^k elements, d_idx: 2^n uint32_t, d_m_out: 2^k elements, written.  PK_ERR_UNSATISFIED: an index
 * failed validation, *first_bad is the smallest such x and d_m_out is not meaningful; otherwise *first_bad = UINT64_MAX.  d_m_out is
 * the T proof's third table: it stays valid and unchanged until pkl_finish.  Blocking. */
int pkl_multiplicities(pkl_prover *p, const uint64_t *d_f, const uint64_t *d_t, const uint32_t *d_idx, uint64_t *d_m_out, uint64_t *first_bad);

/* Steps 2 and 3, after a successful pkl_multiplicities on this prover with the same d_t and d_idx (refused otherwise).  bind: n_bind
 * elements.  alpha_out: one element, may be NULL.  *d_hf_out, *d_ht_out: the arena's h_f (2^n) and h_t (2^k), for the caller to
 * commit; valid until the next pkl_begin.  PK_ERR_UNSATISFIED: alpha is an entry of t; draw another by binding something else. */
int pkl_begin(pkl_prover *p, const uint64_t *d_t, const uint32_t *d_idx, const uint64_t *bind, uint64_t *alpha_out, const uint64_t **d_hf_out,
              const uint64_t **d_ht_out);

/* Steps 4 and 5, after pkl_begin.  bind2: n_bind2 elements.  *len = pkl_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG,
 * nothing proved, the prover stays usable (call again with a larger buffer).  claims_out may be NULL. */
int pkl_finish(pkl_prover *p, const uint64_t *bind2, uint8_t *proof_out, size_t cap, size_t *len, pkl_claims *claims_out);

/* Host only, no device.  io_pattern NULL: pkl_io_pattern's bytes for stmt.  claims_out is written when the proof is accepted.
 * side_out (may be NULL): PKL_SIDE_*.  result carries the verifier core's and pks's check numbers unchanged (pks_check_name); its
 * offset counts bytes of the whole proof. */
int pkl_verify(const pkl_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind, const uint64_t *bind2,
               const uint8_t *proof, size_t len, pkl_claims *claims_out, int *side_out, pkv_result *result);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_LOOKUP_H */
