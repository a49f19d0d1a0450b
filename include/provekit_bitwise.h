/*
 * provekit_bitwise.h -- C ABI of libprovekit_bitwise.so: AND / XOR / OR of device columns, entry by entry, by digit lookups.
 *
 * A thirteenth library above the product's C ABI: it links libprovekit_hip.so, libprovekit_sumcheck.so, libprovekit_fracsum.so
 * (transitively) and libprovekit_tuplelookup.so, calls pkt_* through their C ABI and of the product only pk_malloc, pk_free and
 * pk_ctx_sync, and adds HIP kernels of its own for gfx950 (csrc/bitwise/bitwise.hip): the fused pass that forms c = a op b, splits
 * all three columns into digit columns and counts their rows' multiplicities, and the operation's table.  It links neither
 * libprovekit_whir.so nor the verify library: committing and opening the columns is the caller's composition
 * (examples/bitwise_pcs_demo.cpp).
 *
 * WHY: after range checks, "column c is a AND b" (or XOR, or OR) on machine words is the lookup a circuit uses most: every hash
 * gadget and every integer bit operation.  A word is split into digits, and every digit triple (a_i, b_i, a_i op b_i) is looked up in
 * one table of 2^(2d) rows.  With the tuple-lookup library alone a caller splits three columns on the host, uploads 3 L digit columns
 * and L index lists, builds and uploads the table, calls pkt_multiplicities and pkt_prove and re-derives the three recomposition
 * identities by hand; nothing stops it from looking the digits up in a table that is not the operation's.  Here the composition is
 * stated once, the verifier evaluates the table's extension itself, and one fused device pass replaces the host's split, the
 * uploads, the index lists and the gathering count: a row's place in the table is (a_i << d) | b_i, nothing is gathered.
 *
 * THE STATEMENT: n, op, d, L, n_bind: columns a, b, c of 2^n field elements (Montgomery form, below p).  op is PKB_AND, PKB_XOR or
 * PKB_OR; a digit has d bits, 1 <= d <= 12; there are L digits, 1 <= L <= 4; bits = L d <= 48; 1 <= n; n_bind is 0 .. 16.  The claim,
 * for every x: a[x] and b[x], as canonical integers, are below 2^bits, and c[x] = a[x] op b[x].  (op, d = 8, L = 4) is a u32 operation
 * by byte lookups.
 *
 * THE PLAN (pkb_plan; one rule, csrc/bitwise/statement.hpp, shared by prover, verifier, kernels and claims):
 *     digit i of a word v is v_i = (v >> d i) mod 2^d, i < L.  Group i < L is the row (a_i, b_i, c_i): three digit columns.
 *     c_groups is the smallest of {1, 2, 4} with c_groups >= L.  At L = 3 the spare fourth group is group 0 again: the same device
 *     pointers, counted twice in m.  n + log2 c_groups <= 28 (pkt's bound).
 *   There is no top check: a word width that is not a multiple of d is a range check on top (provekit_rangecheck.h).
 *   The table has k = 2 d variables: row y = (u << d) | v is (u, v, u op v).
 *   m[y], y < 2^(2d): how many rows of all c_groups groups equal row y.
 *
 * THE PROTOCOL
 *   1. the outer transcript has the label "provekit-hip/bitwise/v1/<and|xor|or>/n<n>/d<d>/l<L>"; it absorbs the n_bind caller
 *      elements (the roots of the commitments to a, b, c, the digit columns and m, all committed before any challenge; none: no
 *      operation) and squeezes one seed.  The outer IO pattern: the label, then A<n_bind>bind, S1seed;
 *   2. the proof is ONE whole pkt proof (provekit_tuplelookup.h) of the statement (n, k = 2 d, w = 3, c_groups, n_bind = 1) that binds
 *      the seed, over the groups above, the operation's table and m: pkb_proof_bytes is pkt_proof_bytes of that statement;
 *   3. the table is NOT committed.  The verifier runs pkt_verify and adds one check of its own, numbered after PKF_CHECK_COUNT:
 *        PKB_CHECK_TABLE: the lookup's table claim t_value at its point z_T equals U(z_T) + beta V(z_T) + beta^2 O(z_T), with
 *        variable 0 the most significant bit as everywhere:
 *            U = sum_{j<d} 2^(d-1-j) z[j],   V = sum_{j<d} 2^(d-1-j) z[d+j],   O = sum_{j<d} 2^(d-1-j) o(z[j], z[d+j]),
 *            o(s, t) = s t for AND, s + t - 2 s t for XOR, s + t - s t for OR.
 *        All three are multilinear and agree with the table's columns on 0/1 points, so they are the columns' extensions; the
 *        verifier evaluates them itself, O(d).  Without the check a prover may look the digits up in any table.
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED five claims hold (pkb_claims, pkb_check_claims), of the evaluations at z_lo of a, b, c
 * and the 3 L digit columns digit_{j,i} (j = 0, 1, 2 for a, b, c), and of m at z_T:
 *     PKB_CLAIM_DIGITS:       sum_{j<3, i<L} coeff[j][i] digit_{j,i}(z_lo) = the lookup's f_value,  coeff[j][i] = beta^j times the sum
 *                             of eq(z_hi, g) over the groups g the plan maps to digit i.  Only committed columns are opened: the
 *                             spare group is never opened, it is group 0's columns again;
 *     PKB_CLAIM_RECOMPOSE_A:  a(z_lo) = sum_i 2^(d i) a_i(z_lo);   PKB_CLAIM_RECOMPOSE_B, _C: the same for b and c;
 *     PKB_CLAIM_M:            m(z_T) = the lookup's m_value.
 * One pkw_open (provekit_whir.h) of {a, b, c} and the digit batches at z_lo and one of m at z_T give the evaluations.
 *
 * SOUNDNESS.  (a) The lookup: pkt's terms for (n, 2 d, 3, c_groups) (provekit_tuplelookup.h): its compression term at w = 3,
 * 2 c_groups 2^n 2^(2d) / p; LogUp (c_groups 2^n + 2^(2d)) / p; the two chains, per layer e the sumcheck error 3 e / p and 1 / p for
 * each of lambda_e and rho, over n + log2 c_groups - 1 and 2 d - 1 layers.  Accepted with PKB_CLAIM_DIGITS and PKB_CLAIM_M it means:
 * every row (a_i[x], b_i[x], c_i[x]) is a row of the table the proof's t_value belongs to.  (b) The table check is exact: the
 * verifier computes the three extensions itself, so that table is the operation's: every a_i[x] and b_i[x] is an integer below 2^d
 * and c_i[x] = a_i[x] op b_i[x].  (c) The recompositions: a and sum_i 2^(d i) a_i are two multilinear polynomials in n variables; z_lo
 * is drawn after the columns are bound, so when they differ they agree at z_lo with probability at most n / p (Schwartz-Zippel); the
 * same for b and for c: 3 n / p together.  (d) No wrap-around: the digits sum to an integer below 2^(L d) <= 2^48 < p, so a[x] equals
 * that integer in the field and as a canonical value, and the operation on words is the operation on their digits, digit by digit.
 *
 * Out of scope: words above 48 bits or L > 4 (two statements on halves); widths that are not a multiple of d; constants as operands;
 * NOT, shifts and rotations; several operations in one proof; hiding / zero knowledge; device sets (on a context of a set the prover
 * runs whole on its rank); a device verifier; an LDS histogram above 2^12 bins; wiring into pk_prove.
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  a and b are never written.
 */
#ifndef PROVEKIT_BITWISE_H
#define PROVEKIT_BITWISE_H

#include "provekit_tuplelookup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKB_MAX_VARS 28
#define PKB_MAX_BIND 16
#define PKB_MAX_DIGIT_BITS 12
#define PKB_MAX_DIGITS 4
#define PKB_MAX_GRID 1024

/* pkb_statement's op */
#define PKB_AND 0
#define PKB_XOR 1
#define PKB_OR 2
#define PKB_OP_COUNT 3

/* pkf's check numbers keep their values; this library's own follows them */
#define PKB_CHECK_TABLE PKF_CHECK_COUNT /* the lookup's table claim is not U + beta V + beta^2 O at z_T: its table is not the operation's */
#define PKB_CHECK_COUNT (PKF_CHECK_COUNT + 1)

/* pkb_check_claims' which_out */
#define PKB_CLAIM_NONE 0 /* all five hold */
#define PKB_CLAIM_DIGITS 1
#define PKB_CLAIM_RECOMPOSE_A 2
#define PKB_CLAIM_RECOMPOSE_B 3
#define PKB_CLAIM_RECOMPOSE_C 4
#define PKB_CLAIM_M 5

typedef struct pkb_statement {
    unsigned n;      /* the columns: 2^n entries */
    unsigned op;     /* PKB_AND, PKB_XOR or PKB_OR */
    unsigned d;      /* bits of a digit; the table and m have 2^(2d) rows */
    unsigned L;      /* digits of a word: a, b and c are below 2^(L d) */
    unsigned n_bind; /* caller elements absorbed first */
} pkb_statement;

/* The plan of a statement.  Group g < c_groups looks up the digits digit_of[g] of a, b and c. */
typedef struct pkb_digit_plan {
    unsigned bits;                     /* L d */
    unsigned k;                        /* 2 d: the table's variables */
    unsigned c_groups;                 /* the lookup's groups: 1, 2 or 4 */
    unsigned digit_of[PKB_MAX_DIGITS]; /* for g < c_groups; the spare group of L = 3 is digit 0 again */
} pkb_digit_plan;

/* What an accepted proof is accepted PROVIDED of; Montgomery. */
typedef struct pkb_claims {
    uint64_t z_lo[PKB_MAX_VARS][4];               /* n coordinates, pkw_open's order: where a, b, c and every digit column are opened */
    uint64_t z_t[PKB_MAX_VARS][4];                /* 2 d coordinates: where m is opened */
    uint64_t digit_coeff[3][PKB_MAX_DIGITS][4];   /* [j][i] = coeff[j][i] for i < L; 0 elsewhere */
    uint64_t digits_value[4];                     /* sum_{j, i} digit_coeff[j][i] digit_{j,i}(z_lo) must be this */
    uint64_t pow2[PKB_MAX_DIGITS][4];             /* [i] = 2^(d i) for i < L; 0 elsewhere */
    uint64_t m_value[4];                          /* m(z_t) must be this */
} pkb_claims;

typedef struct pkb_prover pkb_prover;

int pkb_abi_version(void);
const char *pkb_check_name(int check); /* pkf_check_name's names, and "TABLE" */
const char *pkb_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n outside 1 .. 28, an unknown op, d outside 1 .. 12, L outside 1 .. 4, n + log2 c_groups
 * above 28, n_bind above 16. */
int pkb_plan(const pkb_statement *stmt, pkb_digit_plan *plan_out);
/* *len is always set to the full length; bytes are copied where they fit. */
int pkb_io_pattern(const pkb_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkb_proof_bytes(const pkb_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds: its own arena (the table's three columns, 2^(2d) elements each;
 * 2^(2d) u32 counts; the cell of the first bad entry; every part rounded up to 64 bytes) and the pkt prover's
 * (pkt_prover_arena_bytes of (n, 2 d, 3, c_groups)). */
int pkb_prover_arena_bytes(const pkb_statement *stmt, size_t *bytes);
/* Host only: digits of up to this many bits (2^(2d) <= 2^12 bins) are counted in a workgroup's LDS histogram, wider ones with
 * device-memory atomics. */
unsigned pkb_count_lds_max_d(void);

/* The prover owns one device arena, sized here, with the operation's table written here, and the pkt prover (its statement is
 * constant).  A proof allocates no device memory.  ctx is borrowed: destroy the prover first. */
int pkb_prover_create(pk_ctx *ctx, const pkb_statement *stmt, pkb_prover **out);
int pkb_prover_destroy(pkb_prover *p);
const char *pkb_last_error(const pkb_prover *p);

/* The fused device pass over d_a, d_b (2^n elements each, device).  c_given = 0: it WRITES d_c = a op b; c_given = 1: it reads d_c
 * and compares.  It writes the 3 L digit columns d_digits_out[j * L + i] (device pointers on the host, 2^n elements each; j = 0, 1, 2
 * for a, b, c) and d_m_out (2^(2d) elements), the multiplicities of all c_groups groups, the spare group included.  Every operand is
 * taken out of Montgomery form and ALL FOUR words of its canonical value are checked against 2^bits.  PK_ERR_UNSATISFIED with
 * *first_bad (may be NULL) = the smallest failing x, also named in the reason, which says which case it is: "a is not below 2^bits",
 * "b is not below 2^bits" (a is, at that x) or "c is not a op b" (both operands are, at that x).  The outputs are not meaningful then
 * (nothing is written outside them).  PK_OK: *first_bad = UINT64_MAX.  d_a and d_b are never written.  Blocking. */
int pkb_decompose(pkb_prover *p, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_c, int c_given, uint64_t *const *d_digits_out, uint64_t *d_m_out,
                  uint64_t *first_bad);

/* d_digits: 3 L device pointers on the host, d_digits[j * L + i], from pkb_decompose or anywhere else; d_m: 2^(2d) elements; bind:
 * n_bind elements.  a, b and c are not needed.  pkt_prove runs with the arena's table, into host staging, and only an accepted proof
 * is copied out.  pkt_prove's refusals pass through as PK_ERR_UNSATISFIED with the group translated to the digit: a digit row outside
 * the table is "a row is not in t" in digit i, with its x; "m is wrong"; "a denominator is zero".  A refused proof writes nothing and
 * leaves the prover usable.  *len = pkb_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG, nothing proved.  claims_out may be
 * NULL.  Blocking. */
int pkb_prove(pkb_prover *p, const uint64_t *const *d_digits, const uint64_t *d_m, const uint64_t *bind, uint8_t *proof_out, size_t cap, size_t *len,
              pkb_claims *claims_out);

/* Host only, no device.  io_pattern NULL: pkb_io_pattern's bytes for stmt.  It checks the framing and the outer transcript, runs
 * pkt_verify and then PKB_CHECK_TABLE, at the end of the proof's bytes.  claims_out is written when the proof is accepted.  side_out:
 * PKT_SIDE_*; layer_out: the layer of that side the verdict is about, as pkt_verify's (0 for the framing, the outer transcript and
 * this library's own check, which names side T).  result carries pkf's check numbers unchanged, and PKB_CHECK_TABLE; its offset
 * counts bytes of the proof.  Any of claims_out, side_out, layer_out may be NULL. */
int pkb_verify(const pkb_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind, const uint8_t *proof, size_t len,
               pkb_claims *claims_out, int *side_out, unsigned *layer_out, pkv_result *result);

/* Host only: the five claims.  abc_evals: 3 elements, a(z_lo), b(z_lo), c(z_lo); digit_evals: 3 L elements, [j * L + i] =
 * digit_{j,i}(z_lo); m_eval: m(z_t); all Montgomery, below p.  PK_OK with *which_out = PKB_CLAIM_NONE when all hold, else the first
 * that does not, in the order of PKB_CLAIM_*.  PK_ERR_BAD_ARG with a reason: a bad statement, a null pointer, an element not below p. */
int pkb_check_claims(const pkb_statement *stmt, const pkb_claims *claims, const uint64_t *abc_evals, const uint64_t *digit_evals, const uint64_t *m_eval,
                     int *which_out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_BITWISE_H */
