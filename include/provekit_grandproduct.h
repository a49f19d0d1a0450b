/*
 * provekit_grandproduct.h -- C ABI of libprovekit_grandproduct.so: GKR grand products and multiset equality over device tables.
 *
 * A seventh library above the product's C ABI: it links libprovekit_hip.so and libprovekit_sumcheck.so, calls only what
 * provekit_hip.h and provekit_sumcheck.h declare, and adds one HIP kernel family of its own for gfx950 (csrc/grandproduct/tree.hip).
 * It does not link libprovekit_whir.so: committing and opening the tables is the caller's composition
 * (examples/grandproduct_pcs_demo.cpp).  A proof costs NO commitment beyond the input tables.
 *
 * 1. THE GRAND PRODUCT.  The statement: n (1 .. 28), n_bind (0 .. 16) and a table v of 2^n values in device memory, Montgomery form,
 * below p.  The claim is   prod_x v[x] = P.   Zero entries are legal: the product is then 0 and nothing divides.
 *
 * The layers of the product tree: V_n = v, V_d[x] = V_{d+1}[x] * V_{d+1}[x + 2^d] for x < 2^d and d = n-1 .. 0, V_0[0] = P.  With
 * variable 0 <-> the most significant index bit (pks's and pkw_open's convention) the two children of a layer are the two contiguous
 * halves of one array: L_d[x] = V_{d+1}[x], R_d[x] = V_{d+1}[x + 2^d], and V_d(z) = sum_x eq(z, x) L_d(x) R_d(x).  The prover keeps
 * the layers in heap layout, tree[2^d + x] = V_d[x] (2^n elements, index 0 unused; the last layer's halves are the caller's v).
 *
 * The protocol (GKR for a product tree; Thaler, "Time-optimal interactive proofs for circuit evaluation", 2013):
 *   1. the outer transcript has the label "provekit-hip/grandproduct/v1/n<n>";
 *   2. it absorbs the n_bind caller elements (the roots; none: no operation);
 *   3. it absorbs the two values of V_1 ("top"); P is their product and is not sent;
 *   4. it squeezes rho_1; the running claim is c_1 = (1 - rho_1) V_1[0] + rho_1 V_1[1] at the point z_1 = (rho_1);
 *   5. for d = 1 .. n-1: it squeezes seed_d; a pks proof (provekit_sumcheck.h) is made of the statement n = d, m = 2, T = 1,
 *      masks {3}, coefficient 1, has_tau = 1, n_bind = 1 with tables {L_d, R_d}, tau = z_d, bind = {seed_d} and expected sum c_d; the
 *      outer transcript absorbs that proof's two final values (l, r) -- read from the inner proof, not repeated -- and squeezes
 *      rho_{d+1}; the claim becomes c_{d+1} = (1 - rho_{d+1}) l + rho_{d+1} r at z_{d+1} = (rho_{d+1}, r_d), r_d the inner proof's
 *      point: the new coordinate comes first, it is the most significant bit of the child layer.
 * The outer IO pattern: the label, then A<n_bind>bind, A2top, S1rho, and per d: S1seed, A2finals, S1rho.
 *
 * The proof is   top (64 bytes) | pks proof 1 | .. | pks proof n-1:   64 + 48 (n - 1)(n + 2) bytes; at n = 1 the 64 bytes alone.
 *
 * WHAT "ACCEPTED" MEANS: accepted PROVIDED one evaluation claim holds:  v(z_n) = c_n,  z_n in pkw_open's coordinate order.
 * pkg_verify writes P, z_n and c_n; pkw_open / pkw_verify (provekit_whir.h) establish the claim for a committed table.
 * Soundness: the n - 1 sumchecks' errors (3 d / p for layer d, its zero check's tau included) and one 1 / p per rho.
 *
 * 2. MULTISET EQUALITY on top of it.  The statement: n, w (1 .. 4 columns per side: pkw_commit's batch limit), n_bind; side A is w
 * device columns a_j, side B w columns b_j, 2^n values each.  The claim: the rows (a_0[x], .., a_{w-1}[x]) and (b_0[x], ..) are
 * equal as multisets.  The outer transcript: the label "provekit-hip/multiset/v1/n<n>/w<w>", absorb n_bind elements (the columns'
 * roots), squeeze gamma, squeeze beta (only when w > 1), squeeze two seeds.  Pattern: A<n_bind>bind, S1gamma, [S1beta], S2seeds.
 * The leaves: leaf_A[x] = gamma - sum_j beta^j a_j[x], likewise for B.  The proof is
 *     grand-product proof of leaf_A | grand-product proof of leaf_B,      each of the statement (n, n_bind = 1) with bind = {its seed};
 * the verifier requires P_A = P_B (PKG_CHECK_PRODUCT, side B).  Accepted PROVIDED two claims (pkg_multiset_claims):
 *     sum_j beta^j a_j(z_A) = gamma - c_A     and     sum_j beta^j b_j(z_B) = gamma - c_B:
 * the caller opens the w columns of a side at its point with one pkw_open and forms the combination.
 * Soundness: two different multisets of rows give different products at a random (gamma, beta) with probability at most
 * (2^n + w) / p; to that add the two grand products' errors.
 *
 * Out of scope: hiding / zero knowledge; device sets (on a context of a set the prover runs whole on its rank; nothing is sharded);
 * a batched device verifier; batching several products into one chain by a random coefficient; proving the small layers on the host.
 *
 * Conventions: provekit_hip.h's.  Every call returns PK_OK or a negative PK_ERR_*; "rejected" is a verdict in the pkv_result, not an
 * error.  Field elements are Montgomery 4 x u64.  A prover is single-caller.  The caller's tables are never written.
 */
#ifndef PROVEKIT_GRANDPRODUCT_H
#define PROVEKIT_GRANDPRODUCT_H

#include "provekit_sumcheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKG_MAX_VARS 28
#define PKG_MAX_BIND 16
#define PKG_MAX_COLUMNS 4
#define PKG_MAX_GRID 1024

/* The verifier core's and pks's check numbers keep their values; this library's own follows them. */
#define PKG_CHECK_PRODUCT PKS_CHECK_COUNT /* the product is not the expected one / the two sides' products differ */
#define PKG_CHECK_COUNT (PKS_CHECK_COUNT + 1)

/* pkg_multiset_verify's side_out */
#define PKG_SIDE_A 0
#define PKG_SIDE_B 1

typedef struct pkg_statement {
    unsigned n;      /* the table: 2^n values */
    unsigned n_bind; /* caller elements absorbed first */
} pkg_statement;

typedef struct pkg_multiset_statement {
    unsigned n;      /* 2^n rows per side */
    unsigned w;      /* columns per side */
    unsigned n_bind; /* caller elements absorbed first */
} pkg_multiset_statement;

/* What an accepted multiset proof is accepted PROVIDED of; Montgomery.  The required combinations are already gamma - c. */
typedef struct pkg_multiset_claims {
    uint64_t gamma[4];
    uint64_t beta[4];                   /* 1 when w = 1 (no squeeze) */
    uint64_t z_a[PKG_MAX_VARS][4];      /* n coordinates, pkw_open's order */
    uint64_t z_b[PKG_MAX_VARS][4];
    uint64_t comb_a[4];                 /* sum_j beta^j a_j(z_a) must be this */
    uint64_t comb_b[4];                 /* sum_j beta^j b_j(z_b) must be this */
} pkg_multiset_claims;

typedef struct pkg_prover pkg_prover;
typedef struct pkg_multiset_prover pkg_multiset_prover;

int pkg_abi_version(void);
const char *pkg_check_name(int check); /* pks_check_name's names, and "PRODUCT" */
const char *pkg_create_error(void);    /* why the calling thread's last call was refused before it had a prover to report to */

/* Host only.  PK_ERR_BAD_ARG with a reason: n outside 1 .. 28, n_bind above 16.  *len is always set to the full length; bytes are
 * copied where they fit. */
int pkg_io_pattern(const pkg_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkg_proof_bytes(const pkg_statement *stmt, size_t *len);
/* Host only: the device memory a prover of this statement holds: the tree (2^n elements) and its n - 1 pks provers' arenas. */
int pkg_prover_arena_bytes(const pkg_statement *stmt, size_t *bytes);
/* Host only: t.  Once a layer has at most 2^t entries, one workgroup finishes all remaining layers out of LDS in one launch. */
unsigned pkg_tail_max_n(void);

/* The prover owns one device arena, sized here, and n - 1 pks provers (their statements are constant).  A proof allocates nothing.
 * ctx is borrowed: destroy the prover first. */
int pkg_prover_create(pk_ctx *ctx, const pkg_statement *stmt, pkg_prover **out);
int pkg_prover_destroy(pkg_prover *p);
const char *pkg_last_error(const pkg_prover *p);

/* The tree kernels by themselves (tests, benchmarks): d_v 2^n elements; d_tree_out 2^n elements, written in heap layout
 * (d_tree_out[2^d + x] = V_d[x] for d < n; element 0 is not written); product_out: P, one host element.  n 1 .. 28.  Blocking. */
int pkg_tree(pk_ctx *ctx, unsigned n, const uint64_t *d_v, uint64_t *d_tree_out, uint64_t *product_out);

/* d_v: 2^n elements; bind: n_bind elements.  *len = pkg_proof_bytes, also when cap is too small: PK_ERR_BAD_ARG, nothing proved,
 * the prover stays usable.  product_out (1 element), point_out (n elements: z_n), value_out (1 element: c_n) may be NULL.  Blocking. */
int pkg_prove(pkg_prover *p, const uint64_t *d_v, const uint64_t *bind, uint8_t *proof_out, size_t cap, size_t *len, uint64_t *product_out,
              uint64_t *point_out, uint64_t *value_out);

/* Host only, no device.  io_pattern NULL: pkg_io_pattern's bytes for stmt.  expected_product NULL: any P is taken.  product_out,
 * point_out (n), value_out are written when the proof is accepted (each may be NULL).  layer_out (may be NULL): the layer d the
 * verdict is about, 0 for the outer framing and transcript.  result carries the verifier core's and pks's check numbers unchanged,
 * and PKG_CHECK_PRODUCT; its offset counts bytes of the whole proof. */
int pkg_verify(const pkg_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind,
               const uint64_t *expected_product_or_null, const uint8_t *proof, size_t len, uint64_t *product_out, uint64_t *point_out,
               uint64_t *value_out, unsigned *layer_out, pkv_result *result);

/* Host only.  PK_ERR_BAD_ARG with a reason: n outside 1 .. 28, w outside 1 .. 4, n_bind above 16. */
int pkg_multiset_io_pattern(const pkg_multiset_statement *stmt, uint8_t *buf, size_t cap, size_t *len);
int pkg_multiset_proof_bytes(const pkg_multiset_statement *stmt, size_t *len);

/* One pkg_prover and ONE leaf table serve both sides, one after the other: the arena is the leaf table, the tree and the pks arenas. */
int pkg_multiset_prover_create(pk_ctx *ctx, const pkg_multiset_statement *stmt, pkg_multiset_prover **out);
int pkg_multiset_prover_destroy(pkg_multiset_prover *p);
const char *pkg_multiset_last_error(const pkg_multiset_prover *p);

/* d_a, d_b: w device pointers each (host arrays), 2^n elements per column; bind: n_bind elements.  The two products are compared
 * before anything is written: unequal products return PK_ERR_UNSATISFIED with a reason, nothing is written and the prover stays
 * usable.  *len as for pkg_prove.  claims_out may be NULL.  Blocking. */
int pkg_multiset_prove(pkg_multiset_prover *p, const uint64_t *const *d_a, const uint64_t *const *d_b, const uint64_t *bind, uint8_t *proof_out,
                       size_t cap, size_t *len, pkg_multiset_claims *claims_out);

/* Host only, no device.  claims_out is written when the proof is accepted.  side_out: PKG_SIDE_*; layer_out as for pkg_verify (0
 * also for the outer transcript of the multiset argument and for the comparison of the two products, which names side B). */
int pkg_multiset_verify(const pkg_multiset_statement *stmt, const uint8_t *io_pattern_or_null, size_t io_pattern_len, const uint64_t *bind,
                        const uint8_t *proof, size_t len, pkg_multiset_claims *claims_out, int *side_out, unsigned *layer_out, pkv_result *result);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_GRANDPRODUCT_H */
