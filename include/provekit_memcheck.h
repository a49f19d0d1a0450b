/*
 * provekit_memcheck.h -- C ABI of libprovekit_memcheck.so: read-write (offline) memory checking over device tables.
 *
 * A tenth library above the product's C ABI: it links libprovekit_hip.so, libprovekit_sumcheck.so (transitively) and
 * libprovekit_fracsum.so, calls only what provekit_hip.h and provekit_fracsum.h declare (of the product: pk_malloc, pk_free,
 * pk_ctx_sync), and adds HIP kernels of its own for gfx950 (csrc/memcheck/mem.hip): a trace builder and two leaf kernels.  It links
 * neither libprovekit_whir.so nor the verify, lookup, grandproduct or tuplelookup libraries: committing and opening the columns is the
 * caller's composition (examples/memcheck_pcs_demo.cpp).
 *
 * THE STATEMENT: n, k, n_bind: 2^n operations on a memory of 2^k cells; 1 <= n <= 27 and 1 <= k <= 27 (the stacked sides below have
 * one variable more and PKF_MAX_VARS is 28); n_bind is 0 .. 16.  Operation i is a read followed by a write at the global time i + 1.
 * The device tables, Montgomery form, below p, committed by the caller:
 *     a, wv, rv, rt: 2^n elements each -- the address as a field element, the value the operation leaves in the cell, the value it
 *                    found there, the time of the write it read (0: the initial contents);
 *     init, fin, ft: 2^k elements each -- the initial contents, the final contents, the time of the last write to the cell (0: never);
 *     m:             2^n elements      -- the multiplicities of the time check: m[d] = how many operations have i - rt_i = d.
 * The cell index j and the time i + 1 are not columns: prover and verifier form their multilinear extensions themselves.  With
 * variable 0 the most significant index bit (pks's, pkf's and pkw_open's convention), I(z) = sum_j z_j 2^(v-1-j) over v coordinates.
 *
 * THE CLAIM (Blum, Evans, Gemmell, Kannan, Naor, "Checking the correctness of memories"; Spice):
 *   1. as multisets of triples,  {(j, init_j, 0)} u {(a_i, wv_i, i+1)}  =  {(a_i, rv_i, rt_i)} u {(j, fin_j, ft_j)};
 *   2. rt_i <= i for every i (rt_i is an integer of 0 .. i).
 * Part 2 is what makes part 1 mean "every read returns what the last write to that address left there".  Without it a read may take a
 * value from the future: with n = k = 1 and one used cell of init 0, the trace
 *     operation 0 claims (rv, rt) = (7, 2) and writes 7;   operation 1 claims (rv, rt) = (0, 0) and writes 7;   fin = 7, ft = 1
 * has write set {(0,0,0), (0,7,1), (0,7,2)} and read set {(0,7,2), (0,0,0), (0,7,1)} (the other cell adds (1, x, 0) to both): equal
 * multisets, and operation 0 read a 7 that nothing had written yet.  Only part 2 refuses it (rt_0 = 2 > 0).
 * NOT proved here: that a load writes back what it read, wv_i = rv_i on load rows.  That is a row constraint of the caller's circuit,
 * sum_x eq(tau, x) (1 - s)(wv - rv) = 0: four terms over three tables, one pks_prove (the example proves it).
 *
 * THE PROTOCOL
 *   1. the outer transcript has the label "provekit-hip/memcheck/v1/n<n>/k<k>"; it absorbs the n_bind caller elements (the roots of
 *      the commitments; none: no operation), squeezes gamma, then beta, then three seeds.  The outer IO pattern: the label, then
 *      A<n_bind>bind, S1gamma, S1beta, S3seeds;
 *   2. side OPS is a pkf fractional sum (provekit_fracsum.h) of (n + 1, unit = 0, n_bind = 1) that binds seed 0.  Its denominators:
 *          q[i]       = gamma - (a_i + beta wv_i + beta^2 (i + 1))     the write set,
 *          q[2^n + i] = gamma - (a_i + beta rv_i + beta^2 rt_i)        the read set,
 *      its numerators the constant sign table: +1 on the first half, -1 on the second (it depends on n alone: made with the prover);
 *   3. side MEM is one of (k + 1, unit = 0, n_bind = 1) that binds seed 1:
 *          q[j]       = gamma - (j + beta init_j),
 *          q[2^k + j] = gamma - (j + beta fin_j + beta^2 ft_j),          the same signs;
 *   4. side TIME is a pkf_lookup proof of (n, k = n, n_bind = 1) that binds seed 2: the column f_i = i - rt_i (a temporary in the
 *      prover's arena, not committed) in the table t = (0, 1, .., 2^n - 1) (made with the prover) under the caller's m;
 *   5. the proof is  OPS | MEM | TIME:  pkf_proof_bytes of the two stacked statements and pkf_lookup_proof_bytes of TIME's, summed;
 *   6. on top of what pkf_verify and pkf_lookup_verify check the verifier requires, with check numbers after PKF_CHECK_COUNT:
 *        PKM_CHECK_SIGN (once per stacked side): the side's numerator claim cp at its point (z_0, ..) equals 1 - 2 z_0 -- the verifier
 *            evaluates the sign table itself, nothing is opened for it;
 *        PKM_CHECK_BALANCE (named on side MEM): P_OPS Q_MEM + P_MEM Q_OPS = 0 -- the two signed sums cancel;
 *        PKM_CHECK_TIME_TABLE: the lookup's t claim equals I(z_T).
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED four claims (pkm_claims), cq_OPS and cq_MEM being the stacked chains' denominator claims:
 *   at OPS's point (z_0, z_lo):   a(z_lo) + beta ((1 - z_0) wv(z_lo) + z_0 rv(z_lo)) + beta^2 z_0 rt(z_lo)
 *                                     = gamma - cq_OPS - beta^2 (1 - z_0)(I(z_lo) + 1);
 *   at MEM's point (y_0, y):      beta ((1 - y_0) init(y) + y_0 fin(y)) + beta^2 y_0 ft(y) = gamma - cq_MEM - I(y);
 *   for the time check:           rt(z_F) = I(z_F) - f_value,      m(z_T) = m_value.
 * pkm_claims carries gamma, beta, the points z_lo, y, z_F, z_T, the coefficients and the four required values; pkm_check_claims forms
 * the four combinations from the nine opened evaluations (a, wv, rv, rt at z_lo; init, fin, ft at y; rt at z_F; m at z_T), so no
 * caller re-derives a coefficient.  rt is opened at two points: one pkw_open with two points when the operation columns were
 * committed as one batch.  All eight columns are committed in ONE phase, before gamma and beta.
 *
 * SOUNDNESS.  (a) Compression: two different triples give the same value a + beta v + beta^2 t for at most 2 values of beta, so over
 * the 2 (2^n + 2^k) triples of both sets some pair collides with probability at most 2 (2^n + 2^k)^2 / p.  (b) The multiset test: when
 * the compressed multisets differ, sum 1 / (X - w) - sum 1 / (X - r) is a non-zero rational function of degree at most
 * 2 (2^n + 2^k): it vanishes at a random gamma with probability at most 2 (2^n + 2^k) / p.  A zero denominator (gamma is a compressed
 * triple) is rejected, not divided by.  (c) The time side: LogUp's (2^n + 2^n) / p (provekit_fracsum.h); a column entry outside
 * 0 .. 2^n - 1 is a field element i - rt_i that is no small integer, i.e. rt_i > i or rt_i no integer of that range.  (d) The four
 * chains: per layer d the layer's sumcheck error 3 d / p and 1 / p for each of lambda_d and rho, over n, k, n - 1 and n - 1 layers.
 * The seeds only separate the chains' transcripts.
 *
 * Out of scope: hiding / zero knowledge; device sets (on a context of a set the prover runs whole on its rank); a device verifier;
 * per-address (not global) timestamps; byte- or word-granular memories with several cells per operation; the load constraint itself
 * (the example proves it with pks_prove); proving the small layers on the host (provekit_grandproduct.h's follow-up, which would pay
 * four times in this library).
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  pkm_prove never writes the caller's tables.
 */
#ifndef PROVEKIT_MEMCHECK_H
#define PROVEKIT_MEMCHECK_H

#include "provekit_fracsum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKM_MAX_VARS 27
#define PKM_MAX_BIND 16
#define PKM_MAX_GRID 1024

/* pkf's check numbers keep their values; this library's own follow them */
#define PKM_CHECK_SIGN PKF_CHECK_COUNT             /* a stacked side's numerator claim is not 1 - 2 z_0 */
#define PKM_CHECK_BALANCE (PKF_CHECK_COUNT + 1)    /* P_OPS Q_MEM + P_MEM Q_OPS != 0: the two multisets differ */
#define PKM_CHECK_TIME_TABLE (PKF_CHECK_COUNT + 2) /* the time side's table claim is not I(z_T) */
#define PKM_CHECK_COUNT (PKF_CHECK_COUNT + 3)

/* pkm_verify's side_out */
#define PKM_SIDE_OPS 0
#define PKM_SIDE_MEM 1
#define PKM_SIDE_TIME 2

/* pkm_check_claims' which_out */
#define PKM_CLAIM_NONE 0 /* all four hold */
#define PKM_CLAIM_OPS 1
#define PKM_CLAIM_MEM 2
#define PKM_CLAIM_RT 3
#define PKM_CLAIM_M 4

typedef struct pkm_statement {
    unsigned n;      /* 2^n operations */
    unsigned k;      /* 2^k cells */
    unsigned n_bind; /* caller elements absorbed first */
} pkm_statement;

/* the eight device columns of a trace, as pkm_prove reads them */
typedef struct pkm_columns {
    const uint64_t *a, *wv, *rv, *rt; /* 2^n elements each */
    const uint64_t *init, *fin, *ft;  /* 2^k elements each */
    const uint64_t *m;                /* 2^n elements */
} pkm_columns;

/* What an accepted proof is accepted PROVIDED of; Montgomery. */
typedef struct pkm_claims {
    uint64_t gamma[4];
    uint64_t beta[4];
    uint64_t z_ops[PKM_MAX_VARS][4]; /* n coordinates, pkw_open's order: z_lo, where a, wv, rv and rt are opened */
    uint64_t z_mem[PKM_MAX_VARS][4]; /* k coordinates: y, where init, fin and ft are opened */
    uint64_t z_f[PKM_MAX_VARS][4];   /* n coordinates: where rt is opened a second time */
    uint64_t z_t[PKM_MAX_VARS][4];   /* n coordinates: where m is opened */
    uint64_t ops_coeff[4][4];        /* of a, wv, rv, rt: 1, beta (1 - z_0), beta z_0, beta^2 z_0 */
    uint64_t mem_coeff[3][4];        /* of init, fin, ft: beta (1 - y_0), beta y_0, beta^2 y_0 */
    uint64_t ops_value[4];           /* sum_j ops_coeff[j] (a, wv, rv, rt)[j](z_ops) must be this */
    uint64_t mem_value[4];           /* sum_j mem_coeff[j] (init, fin, ft)[j](z_mem) must be this */
    uint64_t rt_value[4];            /* rt(z_f) must be this */
    uint64_t m_value[4];             /* m(z_t) must be this */
} pkm_claims;

typedef struct pkm_prover pkm_prover;

int pkm_abi_version(void);
const char *pkm_check_name(int check); /* pkf_check_name's names, and "SIGN", "BALANCE", "TIME_TABLE" */
const char *pkm_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n or k outside 1 .. 27, n_bind above 16.  *len is always set to the full length; bytes
 * are copied where they fit. */
int pkm_io_pattern(const pkm_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkm_proof_bytes(const pkm_statement *stmt, size_t *len);
/* The device memory a prover of this statement holds: its own arena (the two stacked denominator tables and the two sign tables,
 * 2 (2^(n+1) + 2^(k+1)) elements; f and t of the time side, 2 2^n; the sort's keys, 2 2^n u64, and its temporary storage; 2^n u32
 * counts; the cell of the first bad index) and the three inner provers'.  NOT host only: the sort is asked for the size of its temporary
 * storage and sizes it for the device it would run on; without a device the call returns PK_ERR_HIP for all but the smallest n. */
int pkm_prover_arena_bytes(const pkm_statement *stmt, size_t *bytes);

/* The prover owns one device arena, sized here, and the three inner provers (their statements are constant); the sign tables and t
 * are written here.  A proof allocates no device memory.  ctx is borrowed: destroy the prover first. */
int pkm_prover_create(pk_ctx *ctx, const pkm_statement *stmt, pkm_prover **out);
int pkm_prover_destroy(pkm_prover *p);
const char *pkm_last_error(const pkm_prover *p);

/* The trace builder: from the operations' addresses d_addr (2^n uint32_t), the values they leave d_wv (2^n elements) and the initial
 * contents d_init (2^k elements) it writes the caller's device tables d_a, d_rv, d_rt, d_m (2^n elements) and d_fin, d_ft (2^k).  One
 * radix sort of the keys (addr, i) over their n + k significant bits and a resolve pass in which an operation looks at its two
 * neighbours in sorted order.  Every address is validated on the device before it is followed: one that is >= 2^k returns
 * PK_ERR_BAD_ARG with *first_bad (may be NULL) = the smallest such operation index, also named in the reason; the outputs are not
 * meaningful then.  PK_OK: *first_bad = UINT64_MAX.  The inputs are never written.  Blocking. */
int pkm_trace(pkm_prover *p, const uint32_t *d_addr, const uint64_t *d_wv, const uint64_t *d_init, uint64_t *d_a, uint64_t *d_rv, uint64_t *d_rt,
              uint64_t *d_fin, uint64_t *d_ft, uint64_t *d_m, uint64_t *first_bad);

/* The two leaf kernels by themselves (tests, benchmarks): d_ops_out 2^(n+1) elements, d_mem_out 2^(k+1) elements, the stacked
 * denominator tables of the protocol's steps 2 and 3; d_f_out_or_null 2^n elements, f_i = i - rt_i (written by the pass over the
 * operations).  cols->m is not read.  gamma, beta: one host element each.  Blocking. */
int pkm_leaves(pk_ctx *ctx, unsigned n, unsigned k, const pkm_columns *cols, const uint64_t *gamma, const uint64_t *beta, uint64_t *d_ops_out,
               uint64_t *d_mem_out, uint64_t *d_f_out_or_null);

/* cols: the eight device columns, from pkm_trace or anywhere else; bind: n_bind elements.  All three sides are proved into host
 * staging the prover owns, the balance and the lookup's fractions are checked, and only then is the proof copied out.
 * PK_ERR_UNSATISFIED with a reason that names the case -- "a denominator is zero" (gamma is a compressed triple, or the time side's
 * alpha an entry), "the multisets differ" (the balance fails) or "a read is not older than its operation, or m is wrong" (the time
 * side) -- writes nothing and leaves the prover usable.  *len = pkm_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG, nothing
 * proved, the prover stays usable.  claims_out may be NULL.  Blocking. */
int pkm_prove(pkm_prover *p, const pkm_columns *cols, const uint64_t *bind, uint8_t *proof_out, size_t cap, size_t *len, pkm_claims *claims_out);

/* Host only, no device.  io_pattern NULL: pkm_io_pattern's bytes for stmt.  It checks the framing and the outer transcript, runs
 * pkf_verify on OPS and MEM and pkf_lookup_verify on TIME, and makes the four checks of step 6: SIGN at the end of its side's bytes,
 * BALANCE on side MEM at its top values' end, TIME_TABLE at the proof's end.  claims_out is written when the proof is accepted.
 * side_out: PKM_SIDE_*; layer_out: the layer of that side the verdict is about, as pkf_verify's (0 for the framing, the outer
 * transcript and this library's own checks).  result carries pkf's check numbers unchanged, and PKM_CHECK_*; its offset counts bytes
 * of the whole proof.  Any of claims_out, side_out, layer_out may be NULL. */
int pkm_verify(const pkm_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind, const uint8_t *proof,
               size_t len, pkm_claims *claims_out, int *side_out, unsigned *layer_out, pkv_result *result);

/* Host only: the four combinations.  ops_evals: 4 elements, (a, wv, rv, rt)(z_ops); mem_evals: 3 elements, (init, fin, ft)(z_mem);
 * rt_eval: rt(z_f); m_eval: m(z_t); all Montgomery, below p.  PK_OK with *which_out = PKM_CLAIM_NONE when all four hold, else the
 * first that does not (PKM_CLAIM_OPS, _MEM, _RT, _M).  PK_ERR_BAD_ARG with a reason: a bad statement, a null pointer, an element not
 * below p. */
int pkm_check_claims(const pkm_statement *stmt, const pkm_claims *claims, const uint64_t *ops_evals, const uint64_t *mem_evals, const uint64_t *rt_eval,
                     const uint64_t *m_eval, int *which_out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_MEMCHECK_H */
