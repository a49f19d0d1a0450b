/*
 * provekit_rangecheck.h -- C ABI of libprovekit_rangecheck.so: limb-decomposed range checks of up to 64 bits over device tables.
 *
 * A twelfth library above the product's C ABI: it links libprovekit_hip.so, libprovekit_sumcheck.so, libprovekit_fracsum.so
 * (transitively) and libprovekit_tuplelookup.so, calls pkt_* through their C ABI and of the product only pk_malloc, pk_free and
 * pk_ctx_sync, and adds HIP kernels of its own for gfx950 (csrc/rangecheck/range.hip): the fused decomposition of a column into limb
 * columns and their multiplicities, the scaled top limb and the index table.  It links neither libprovekit_whir.so nor the verify
 * library: committing and opening the columns is the caller's composition.
 *
 * WHY: "every entry of this column is below 2^B" is the most common lookup there is.  The lookup libraries prove one when the range
 * fits in a table, 2^B <= 2^28, and they need an index hint from the prover.  Ranges of 32 or 64 bits -- a VM trace, a u64 ALU, a hash
 * gadget -- are proved by splitting every value into limbs, looking the limbs up in a small identity table and tying the limbs back to
 * the column.  With the libraries below alone a caller splits on the host, builds limb columns and index lists, uploads them, calls
 * pkt_multiplicities and pkt_prove and re-derives the identity that links limbs and column by hand; nothing states the recomposition
 * claim or the bound of the top limb, and nothing stops a caller from looking the limbs up in a table that is not the identity.  Here
 * the composition is stated once, and one fused device pass replaces the host's split, the upload and the gathering count: the table
 * is the identity, so a limb is its own index and nothing is gathered.
 *
 * THE STATEMENT: n, bits, k, n_bind: a column f of 2^n field elements (Montgomery form, below p); the claim: every f[x], as a canonical
 * integer, is < 2^bits; limbs of k bits.  1 <= bits <= 64; 1 <= k <= 28; 1 <= n; n_bind is 0 .. 16.
 *
 * THE PLAN (pkr_plan; one rule, csrc/rangecheck/statement.hpp, shared by prover, verifier, kernels and claims):
 *     L = ceil(bits / k) limbs, limb_i = (f >> k i) mod 2^k;     r = bits - (L - 1) k: the number of bits of the top limb, 1 .. k.
 *   The groups looked up in the identity table I_k = (0, 1, .., 2^k - 1):
 *     group i < L: the limb column i;
 *     when r < k, group L, the TOP CHECK: 2^(k-r) limb_{L-1}.  limb_{L-1} < 2^k and 2^(k-r) limb_{L-1} < 2^k together force
 *       limb_{L-1} < 2^r: the product is below 2^(2k) <= 2^56 < p, so it is the integer product, no wrap-around;
 *     G = L + (r < k) groups.  G > 4 is refused, with a reason that names a k that works (k >= ceil(bits / 3) always does).
 *     c is the smallest of {1, 2, 4} with c >= G.  When G = 3 the spare fourth group is limb 0 again: the same device pointer, counted
 *     twice in m.  n + log2 c <= 28 (pkt's bound).
 *   m[y], y < 2^k: how many entries of all c groups equal y.
 *
 * THE PROTOCOL
 *   1. the outer transcript has the label "provekit-hip/range/v1/n<n>/b<bits>/k<k>"; it absorbs the n_bind caller elements (the
 *      roots of the commitments to f, the limbs and m, all committed before any challenge; none: no operation) and squeezes one seed.
 *      The outer IO pattern: the label, then A<n_bind>bind, S1seed;
 *   2. the proof is ONE whole pkt proof (provekit_tuplelookup.h) of the statement (n, k, w = 1, c, n_bind = 1) that binds the seed, over
 *      the c groups above, the table I_k and m: pkr_proof_bytes is pkt_proof_bytes of that statement;
 *   3. the table is NOT committed.  The verifier runs pkt_verify and adds one check of its own, numbered after PKF_CHECK_COUNT:
 *        PKR_CHECK_TABLE: the lookup's table claim t_value at its point z_T equals I(z_T) = sum_j z_T[j] 2^(k-1-j), which the verifier
 *            evaluates itself, O(k).  Without it a prover may look the limbs up in any table.
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED three claims hold (pkr_claims, pkr_check_claims), of f_eval = f(z_lo),
 * limb_evals[i] = limb_i(z_lo), i < L, and m_eval = m(z_T):
 *     PKR_CLAIM_LIMBS:      sum_i coeff_i limb_evals[i] = the lookup's f_value,   coeff_i = sum over the groups g that the plan maps to
 *                           limb i of eq(z_hi, g) scale_g;  scale_g = 2^(k-r) for the top check and 1 otherwise.  Only committed columns
 *                           are opened: the scaled column and the spare group are never opened, they are multiples of limb columns;
 *     PKR_CLAIM_RECOMPOSE:  f_eval = sum_i 2^(k i) limb_evals[i];
 *     PKR_CLAIM_M:          m_eval = the lookup's m_value.
 * One pkw_open (provekit_whir.h) of {f, limb_0, .., limb_{L-1}} at z_lo and one of m at z_T give the evaluations.
 *
 * SOUNDNESS.  (a) The lookup: pkt's terms for (n, k, 1, c) (provekit_tuplelookup.h): no compression term at w = 1; LogUp
 * (c 2^n + 2^k) / p; the two chains, per layer d the sumcheck error 3 d / p and 1 / p for each of lambda_d and rho, over n + log2 c - 1
 * and k - 1 layers.  Accepted with PKR_CLAIM_LIMBS and PKR_CLAIM_M it means: every limb_i[x] and, when r < k, every
 * 2^(k-r) limb_{L-1}[x] is an entry of the table the proof's t_value belongs to.  (b) The table check is exact: the verifier computes
 * the extension of I_k itself, so that table is I_k, every limb is an integer below 2^k and the top limb below 2^r.  (c) The
 * recomposition: f and sum_i 2^(k i) limb_i are two multilinear polynomials in n variables; z_lo is drawn after the columns are bound,
 * so when they differ they agree at z_lo with probability at most n / p (Schwartz-Zippel).  (d) No wrap-around: the limbs sum to an
 * integer below 2^((L-1)k + r) = 2^bits <= 2^64 < p, so f[x] equals that integer in the field and as a canonical value.
 *
 * Out of scope: bits > 64; bounds that are not powers of two, and signed ranges; several columns in one proof; hiding / zero
 * knowledge; device sets (on a context of a set the prover runs whole on its rank); a device verifier; an LDS histogram above 2^12
 * bins (k = 16 in dynamic LDS, for example).
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  The caller's tables are never written.
 */
#ifndef PROVEKIT_RANGECHECK_H
#define PROVEKIT_RANGECHECK_H

#include "provekit_tuplelookup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKR_MAX_VARS 28
#define PKR_MAX_BIND 16
#define PKR_MAX_BITS 64
#define PKR_MAX_LIMB_BITS 28
#define PKR_MAX_GROUPS 4
#define PKR_MAX_GRID 1024

/* pkf's check numbers keep their values; this library's own follows them */
#define PKR_CHECK_TABLE PKF_CHECK_COUNT /* the lookup's table claim is not I(z_T): its table is not 0 .. 2^k - 1 */
#define PKR_CHECK_COUNT (PKF_CHECK_COUNT + 1)

/* pkr_check_claims' which_out */
#define PKR_CLAIM_NONE 0 /* all three hold */
#define PKR_CLAIM_LIMBS 1
#define PKR_CLAIM_RECOMPOSE 2
#define PKR_CLAIM_M 3

typedef struct pkr_statement {
    unsigned n;      /* the column: 2^n entries */
    unsigned bits;   /* every entry is below 2^bits */
    unsigned k;      /* bits of a limb; the table I_k and m have 2^k entries */
    unsigned n_bind; /* caller elements absorbed first */
} pkr_statement;

/* The plan of a statement.  Group g < groups looks up 2^shift_of[g] limb_{limb_of[g]}; groups .. c - 1 (G = 3 only) is the spare. */
typedef struct pkr_limb_plan {
    unsigned limbs;                    /* L */
    unsigned top_bits;                 /* r */
    unsigned groups;                   /* G */
    unsigned c;                        /* the lookup's groups: 1, 2 or 4 */
    unsigned limb_of[PKR_MAX_GROUPS];  /* for g < c */
    unsigned shift_of[PKR_MAX_GROUPS]; /* k - r for the top check, 0 otherwise */
} pkr_limb_plan;

/* What an accepted proof is accepted PROVIDED of; Montgomery. */
typedef struct pkr_claims {
    uint64_t z_lo[PKR_MAX_VARS][4];         /* n coordinates, pkw_open's order: where f and every limb are opened */
    uint64_t z_t[PKR_MAX_VARS][4];          /* k coordinates: where m is opened */
    uint64_t limb_coeff[PKR_MAX_GROUPS][4]; /* [i] = coeff_i for i < L; 0 elsewhere */
    uint64_t limbs_value[4];                /* sum_i limb_coeff[i] limb_i(z_lo) must be this */
    uint64_t pow2[PKR_MAX_GROUPS][4];       /* [i] = 2^(k i) for i < L; 0 elsewhere: f(z_lo) must be sum_i pow2[i] limb_i(z_lo) */
    uint64_t m_value[4];                    /* m(z_t) must be this */
} pkr_claims;

typedef struct pkr_prover pkr_prover;

int pkr_abi_version(void);
const char *pkr_check_name(int check); /* pkf_check_name's names, and "TABLE" */
const char *pkr_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n outside 1 .. 28, bits outside 1 .. 64, k outside 1 .. 28, more than 4 groups (the reason
 * names a k that works), n + log2 c above 28, n_bind above 16. */
int pkr_plan(const pkr_statement *stmt, pkr_limb_plan *plan_out);
/* *len is always set to the full length; bytes are copied where they fit. */
int pkr_io_pattern(const pkr_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkr_proof_bytes(const pkr_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds: its own arena (I_k, 2^k elements; the scaled column, 2^n elements,
 * only when r < k; 2^k u32 counts; the cell of the first bad entry; every part rounded up to 64 bytes) and the pkt prover's
 * (pkt_prover_arena_bytes of (n, k, 1, c)). */
int pkr_prover_arena_bytes(const pkr_statement *stmt, size_t *bytes);
/* Host only: limbs of up to this many bits are counted in a workgroup's LDS histogram, wider ones with device-memory atomics. */
unsigned pkr_count_lds_max_k(void);

/* The prover owns one device arena, sized here, with I_k written here, and the pkt prover (its statement is constant).  A proof
 * allocates no device memory.  ctx is borrowed: destroy the prover first. */
int pkr_prover_create(pk_ctx *ctx, const pkr_statement *stmt, pkr_prover **out);
int pkr_prover_destroy(pkr_prover *p);
const char *pkr_last_error(const pkr_prover *p);

/* The fused device pass: from d_f (2^n elements, device) it writes the L limb columns d_limbs_out[i] (L device pointers on the host,
 * 2^n elements each) and d_m_out (2^k elements), the multiplicities of all c groups, the scaled top limb and the spare group
 * included.  Every entry is taken out of Montgomery form and ALL FOUR words of its canonical value are checked against 2^bits.  An
 * entry >= 2^bits returns PK_ERR_UNSATISFIED with *first_bad (may be NULL) = the smallest such x, also named in the reason; the outputs
 * are not meaningful then (nothing is written outside them).  PK_OK: *first_bad = UINT64_MAX.  d_f is never written.  Blocking. */
int pkr_decompose(pkr_prover *p, const uint64_t *d_f, uint64_t *const *d_limbs_out, uint64_t *d_m_out, uint64_t *first_bad);

/* d_limbs: L device pointers on the host, from pkr_decompose or anywhere else; d_m: 2^k elements; bind: n_bind elements.  f is not
 * needed.  When r < k the scaled top column is written into the prover's arena; then pkt_prove runs with the arena's I_k as the
 * table, into host staging, and only an accepted proof is copied out.  pkt_prove's refusals pass through as PK_ERR_UNSATISFIED with
 * the group translated: a limb >= 2^k is "a row is not in t" in its limb's group, a top limb >= 2^r the same in the top-check group,
 * each with its x; "m is wrong"; "a denominator is zero".  A refused proof writes nothing and leaves the prover usable.
 * *len = pkr_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG, nothing proved.  claims_out may be NULL.  Blocking. */
int pkr_prove(pkr_prover *p, const uint64_t *const *d_limbs, const uint64_t *d_m, const uint64_t *bind, uint8_t *proof_out, size_t cap, size_t *len,
              pkr_claims *claims_out);

/* Host only, no device.  io_pattern NULL: pkr_io_pattern's bytes for stmt.  It checks the framing and the outer transcript, runs
 * pkt_verify and then PKR_CHECK_TABLE, at the end of the proof's bytes.  claims_out is written when the proof is accepted.  side_out:
 * PKT_SIDE_*; layer_out: the layer of that side the verdict is about, as pkt_verify's (0 for the framing, the outer transcript and
 * this library's own check, which names side T).  result carries pkf's check numbers unchanged, and PKR_CHECK_TABLE; its offset
 * counts bytes of the proof.  Any of claims_out, side_out, layer_out may be NULL. */
int pkr_verify(const pkr_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind, const uint8_t *proof, size_t len,
               pkr_claims *claims_out, int *side_out, unsigned *layer_out, pkv_result *result);

/* Host only: the three claims.  f_eval: f(z_lo); limb_evals: L elements, limb_i(z_lo); m_eval: m(z_t); all Montgomery, below p.  PK_OK
 * with *which_out = PKR_CLAIM_NONE when all hold, else the first that does not, in the order of PKR_CLAIM_*.  PK_ERR_BAD_ARG with a
 * reason: a bad statement, a null pointer, an element not below p. */
int pkr_check_claims(const pkr_statement *stmt, const pkr_claims *claims, const uint64_t *f_eval, const uint64_t *limb_evals, const uint64_t *m_eval,
                     int *which_out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_RANGECHECK_H */
