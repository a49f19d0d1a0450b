/* pk_probes.h -- libpk_probes.so: measurement probes and rejected prototypes, built from the product's headers and linked against
 * libprovekit_hip.so, but NOT part of the drop-in (nothing here is for a binder of include/provekit_hip.h).  Same conventions:
 * int status (0 ok, PK_ERR_*), pk_ctx from pk_ctx_create. */
#ifndef PK_PROBES_H
#define PK_PROBES_H
#include "provekit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the same ops run by a kernel on device buffers (device-vs-host codegen diff in the GPU suite) */
int pk_probe_arith_device(pk_ctx *ctx, int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t n);
/* the parts of the safegcd inverse (pk_selftest_inv30, pk_selftest.h: parts 0..6) run by a kernel, one lane per record: d_in and d_out
 * hold n records of 32 words each */
int pk_probe_inv30_device(pk_ctx *ctx, int part, const int32_t *d_in, int32_t *d_out, size_t n);
/* measurement aid (SURVEY 8d "measured_peak_modmul_per_s"): rate of register-resident 9x29-bit Montgomery squarings,
 * ilp (1|2|4) independent chains per lane, waves_per_simd (1..8) resident waves, iters squarings per chain */
int pk_probe_modmul_rate(pk_ctx *ctx, unsigned waves_per_simd, unsigned ilp, unsigned iters, double *modmul_per_s);
/* VERDICT r05 item 3, the ceiling of a hand-allocated Skyscraper square round by ABLATION: rounds per second of the product's round
 * (variant 0) and of the same round with the instructions assembly could fold away left out (1: the 8 additions of the round constant;
 * 2: also the zero-extensions of r into the 64-bit columns; 3: also the 8 doublings) -- wrong results, the product's multiply-adds and
 * dependency structure (tools/probes/probes.hip sq_round_ablated, tools/sq_round_ablation.py, profiles/r06_sq_round_ablation.json) */
int pk_probe_sq_round_rate(pk_ctx *ctx, int variant, unsigned waves_per_simd, unsigned ilp, unsigned iters, double *rounds_per_s);
/* PROTOTYPE, not on the product path (tools/probes/fe52.hpp): the reference's f64-FMA Montgomery square on 5 x 52-bit limbs
 * (skyscraper/block-multiplier/src/portable_simd.rs:17-196, utils.rs:66-147, constants.rs:100-133; round-toward-zero as
 * fp-rounding/src/lib.rs:57-78).  a: n values < 2^256 (4 x u64 each) -> out5: n x 5 limbs of x^2 * 2^-260 mod p, lazily
 * reduced (< 2^257).  Host: under fesetround(FE_TOWARDZERO); device: MODE.FP_ROUND set by the kernel; _rate_fp52: the same
 * probe as pk_probe_modmul_rate for this multiplier, so the two can be compared on one box. */
int pk_probe_fp52_sqr(const uint64_t *a, uint64_t *out5, size_t n);
/* PROTOTYPE probe, not on the product path: the wavefront-cooperative Skyscraper square round (limbs in lanes 0..8, v_readlane
 * broadcasts, DPP window shift) next to the lone lane's round (skyscraper29s.hpp sky_sq_round_s), `iters` rounds each on one
 * wavefront of an idle GPU: out[36] = coop l, coop r, lane l, lane r (9 x 29-bit limbs each); cycles[0..1] = s_memtime ticks of the
 * two loops inside one launch, cycles[2..3] = nanoseconds of each loop in a launch of its own (hipEvents).  north_star's
 * "one-wavefront-per-node Skyscraper rounds", measured. */
int pk_probe_coop_round(pk_ctx *ctx, const uint32_t l[9], const uint32_t r[9], unsigned iters, uint32_t out[36],
                           uint64_t cycles[4]);
int pk_probe_fp52_sqr_device(pk_ctx *ctx, const uint64_t *d_a, uint64_t *d_out5, size_t n);
int pk_probe_modmul_rate_fp52(pk_ctx *ctx, unsigned waves_per_simd, unsigned ilp, unsigned iters, double *modmul_per_s);
/* modular reduction as a constant-matrix product on the matrix core (v_mfma_i32_16x16x64_i8 over the
 * 8/8/8/5-bit digits a 29-bit limb already holds; tools/probes/probes.hip "Reduction on the matrix core") -- measured and
 * NOT adopted.  pk_probe_mfma_reduce: the product itself, exact (d_t_limbs: n x 18 limbs of 29 bits, d_out: n x 36 column sums
 * with sum_i out[i] 2^(29 (i/4) + 8 (i%4)) == t 2^-256 mod p, non-negative, < 2^270).  The two rate probes return squarings per
 * second: the matrix pipe fed for free, and the vector work that remains with the matrix products and lane movement free. */
/* one Fiat-Shamir round trip as pk_prove makes it (launch + stream synchronisation) against the same round trip
 * through a persistent kernel's pinned mailbox, `host_work_permutes` sponge permutations of host work in between; microseconds per
 * round over `rounds` dependent round trips (tools/roundtrip.py, profiles/r04_roundtrip.json). */
/* products by a constant per second, register-resident chains: the Montgomery product (mont261_29, shoup = 0) against the Shoup form
 * with a precomputed quotient (shoup261_29, shoup = 1: 143 multiply-adds instead of 162 + 9); csrc/fe29.hpp */
int pk_probe_constmul_rate(pk_ctx *ctx, unsigned waves_per_simd, unsigned ilp, unsigned iters, int shoup, double *modmul_per_s);
int pk_probe_roundtrip(pk_ctx *ctx, unsigned rounds, unsigned host_work_permutes, double *us_per_round_launch,
                          double *us_per_round_mailbox);
/* `launches` dependent one-wavefront kernels back to back on the context's stream, one synchronisation at the end: microseconds per
 * kernel boundary with no host in the loop */
int pk_probe_launch_chain(pk_ctx *ctx, unsigned launches, unsigned threads_per_launch, double *us_per_launch);
int pk_probe_mfma_reduce(pk_ctx *ctx, const uint32_t *d_t_limbs, int32_t *d_out, size_t n);
int pk_probe_mfma_reduce_rate(pk_ctx *ctx, unsigned waves_per_simd, unsigned iters, double *squarings_per_s);
int pk_probe_mfma_valu_rate(pk_ctx *ctx, unsigned waves_per_simd, unsigned ilp, unsigned iters, double *squarings_per_s);

/* The leaf hash of a column-major codeword the CALLER built in the hash-ready encoding PK_LEAVES_SCALED32 (csrc/internal.hpp
 * leaf_hash_x with scaled_in: the kernel the product reaches only behind its own NTT), for tests/test_gpu_scaled_codeword.py:
 * d_leaves = width x n_leaves elements, each below the encoding's consumer bound; d_digests = n_leaves canonical digests.
 * pk_probe_scaled32_bounds (host only): that bound and the largest element a commit stores, as csrc/skyscraper29s.hpp states
 * them (SCALED32_BOUND_NUM / _DEN, SCALED32_PRODUCER_SHIFT), 4 x u64 each. */
int pk_probe_leaf_hash_scaled(pk_ctx *ctx, const uint64_t *d_leaves, size_t n_leaves, size_t width, uint64_t *d_digests);
int pk_probe_scaled32_bounds(uint64_t consumer_bound[4], uint64_t producer_max[4]);

/* The entry points of csrc/mle.hip that have no C ABI of their own (csrc/internal.hpp: dot_rows, eval_univariate_multi, lincomb2,
 * fold_pairs2 and the launch-only sumcheck rounds), for tests/test_gpu_mle_edges.py: the functions' own argument order, device
 * pointers the caller owns.  dot_rows in its non-deferred form, fold_pairs2 and the sumcheck launches without a gate (gate_seq = 0)
 * only.  pk_probe_sumcheck_collect_spin takes the three sums of the context's LAST launch (its *red_seq_out) without draining the
 * stream.  pk_probe_num_cus / pk_probe_reduction_blocks: the compute-unit count the context sizes its grids by, and the grid
 * reduce.hpp's reduction_blocks gives `work_items` items in the context's current mode. */
int pk_probe_num_cus(pk_ctx *ctx, int *num_cus);
int pk_probe_reduction_blocks(pk_ctx *ctx, size_t work_items, unsigned *blocks);
int pk_probe_dot_rows(pk_ctx *ctx, const uint64_t *d_w, size_t row_stride, unsigned nrows, const uint64_t *d_f, const uint64_t *d_g, size_t n,
                      uint64_t *out);
int pk_probe_eval_univariate_multi(pk_ctx *ctx, const uint64_t *const *d_polys, unsigned np, size_t n, const uint64_t z[4], uint64_t *out);
int pk_probe_lincomb2(pk_ctx *ctx, uint64_t *d_out, const uint64_t *d_a, const uint64_t *beta, const uint64_t *d_b, size_t n);
int pk_probe_fold_pairs2(pk_ctx *ctx, const uint64_t *d_v0, uint64_t *d_out0, const uint64_t *d_v1, uint64_t *d_out1, size_t len,
                         const uint64_t *r);
int pk_probe_sumcheck_cubic_launch(pk_ctx *ctx, uint64_t *d_a, uint64_t *d_b, uint64_t *d_c, uint64_t *d_eq, size_t len,
                                   const uint64_t *fold_or_null, unsigned *red_seq_out);
int pk_probe_sumcheck_quadratic_launch(pk_ctx *ctx, const uint64_t *d_f, const uint64_t *d_w, size_t len, const uint64_t *fold_or_null,
                                       uint64_t *d_f_out, uint64_t *d_w_out, unsigned *red_seq_out);
int pk_probe_sumcheck_collect_spin(pk_ctx *ctx, unsigned red_seq, uint64_t out[12]);
/* ... and the fused steps of the commit and of WhirProver::start, for tests/test_gpu_commit_fused.py.  pk_probe_lincomb2_pair: two
 * lincomb2 with one beta in one launch.  pk_probe_axpy3: y += g3[0] r0 + g3[1] r1 + g3[2] r2, g3 = 3 HOST elements, row k at
 * d_rows + k * row_stride elements.  pk_probe_to_coeffs_generated: f = [witness, zero padded to 2^(m-1) || draw stream_mask],
 * g = draw stream_g under seed32, 2^m elements each -- the evaluation tables and their to_coeffs, four tables the caller owns. */
int pk_probe_lincomb2_pair(pk_ctx *ctx, uint64_t *d_out0, const uint64_t *d_a0, const uint64_t *d_b0, size_t n0, uint64_t *d_out1,
                           const uint64_t *d_a1, const uint64_t *d_b1, size_t n1, const uint64_t *beta);
int pk_probe_axpy3(pk_ctx *ctx, uint64_t *d_y, const uint64_t *g3, const uint64_t *d_rows, size_t row_stride, size_t n);
int pk_probe_to_coeffs_generated(pk_ctx *ctx, unsigned m, const uint64_t *d_wit, size_t n_wit, const uint8_t seed32[32], uint32_t stream_mask,
                                 uint32_t stream_g, uint64_t *d_f_evals, uint64_t *d_g_evals, uint64_t *d_f_coeffs, uint64_t *d_g_coeffs);
/* ... and the fused steps of the WHIR opening, for tests/test_gpu_opening_fused.py.  pk_probe_opening_first: round 0 of a quadratic
 * sumcheck in the launch that forms its tables (csrc/internal.hpp opening_first_launch), 2^n_vars entries, n_vars >= 1.  d_e0 != NULL: the
 * opening's first launch -- d_p = d_e0 + beta d_e1, d_w = (overwrite ? 0 : d_w) + sum_j scales[j] eq(points[j], .) + sum_k row_scales[k] row_k
 * with nrows = 1 or 3 rows of row_len leading entries at d_rows + k * row_stride, nsums = 2 (out = h(0), h(2)) or 3.  d_e0 == NULL: a
 * round's new weights -- d_p is read only, no rows (nrows = 0), nsums = 3.  points (q x n_vars), scales, beta, row_scales: HOST.  grid:
 * 0, or a cap on the workgroups.  pk_probe_dot_rows_eq: out[4 k] = <row k, eq(point, .)> over the rows' first n entries, nrows = 1 or
 * 3, without the table (dot_rows_eq). */
int pk_probe_opening_first(pk_ctx *ctx, const uint64_t *d_e0, const uint64_t *d_e1, const uint64_t *beta, uint64_t *d_p, uint64_t *d_w,
                           unsigned n_vars, const uint64_t *points, const uint64_t *scales, unsigned q, int overwrite, const uint64_t *d_rows,
                           size_t row_stride, unsigned nrows, size_t row_len, const uint64_t *row_scales, int nsums, unsigned grid,
                           uint64_t out[12]);
int pk_probe_dot_rows_eq(pk_ctx *ctx, const uint64_t *d_rows, size_t row_stride, unsigned nrows, const uint64_t *point, unsigned n_vars, size_t n,
                         uint64_t *out);

/* libprovekit_whir.so's linear-statement kernels (csrc/whir_pcs/linear.hip) where its C ABI does not reach, for
 * tests/test_gpu_whir_pcs_linear.py and tools/whir_pcs_linear_bench.py.  This library links libprovekit_whir.so for them.
 * pk_probe_whir_combine: d_w[x] = (accumulate ? d_w[x] : 0) + sum_i scales[i] * d_weights[i][x], x < len (d_weights: HOST array of
 * l device tables; scales: l HOST elements, Montgomery).  pk_probe_whir_weighted_sums: pkw_weighted_sums on a grid of `grid`
 * workgroups (0 or 1..pk_probe_whir_wsum_grid(n_vars)) with register tile 0 (what ships: 2 x 2, and 1 x 4 for batch = 1), 1 (1 x 4), 2 (2 x 1) or 3 (2 x 2 always).
 * pk_probe_wsum_tile_host: the shipped tile's accumulate / flush / result code on the HOST, f = 2 x terms and w = 2 x terms
 * elements (operand-major), out = 4 elements out[u * 2 + v] = sum_t f[u][t] * w[v][t] * 2^-256 mod p. */
int pk_probe_whir_combine(pk_ctx *ctx, uint64_t *d_w, size_t len, const uint64_t *const *d_weights, const uint64_t *scales, unsigned l,
                          int accumulate);
int pk_probe_whir_weighted_sums(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *const *d_weights,
                                unsigned l, unsigned grid, int tile, uint64_t *out);
unsigned pk_probe_whir_wsum_grid(unsigned n_vars);
int pk_probe_wsum_tile_host(const uint64_t *f, const uint64_t *w, unsigned terms, uint64_t *out);

/* The rank slices of a device set (csrc/whir_pcs/pcs.cpp), on ONE context, for tests/test_gpu_whir_pcs_sharded.py and
 * tools/whir_pcs_sharded_profile.py.  pk_probe_whir_eval_slice: one pass of the evaluation kernel (Q <= 8 HOST points) over the
 * workgroups [first_wg, first_wg + count) of pk_probe_whir_eval_grid(n_vars); partial_out = batch * 8 * count HOST elements,
 * [(b * 8 + i) * count + j].  pk_probe_whir_wsum_slice: one pass of the weighted-sums kernel (L <= 8 weights) over the same kind of
 * slice of a grid of `grid` (0: pk_probe_whir_wsum_grid); partial_out = batch * L * count elements, [(b * L + i) * count + j].
 * pk_probe_whir_finish: the library's finish kernel over HOST partials that lie in n_wg / chunk blocks of `chunk` workgroups each,
 * block_stride elements apart (`total` elements in all): out[y * count + i], y < rows, i < count <= row_stride.  ms, where not
 * null: the launch's time between two events on an otherwise idle context, in milliseconds. */
unsigned pk_probe_whir_eval_grid(unsigned n_vars);
int pk_probe_whir_eval_slice(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *points, unsigned Q,
                             unsigned first_wg, unsigned count, uint64_t *partial_out, float *ms);
int pk_probe_whir_wsum_slice(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *const *d_weights,
                             unsigned L, unsigned grid, unsigned first_wg, unsigned count, int tile, uint64_t *partial_out, float *ms);
int pk_probe_whir_finish(pk_ctx *ctx, const uint64_t *partials, size_t total, unsigned n_wg, unsigned chunk, size_t block_stride, unsigned rows,
                         unsigned count, unsigned row_stride, uint64_t *out);

/* ... and its sparse-weight code (csrc/whir_pcs/sparse.hip, sparse.hpp; whir_sparse.hip here), for tests/test_gpu_whir_pcs_sparse.py,
 * tests/test_whir_pcs_sparse_host.py and tools/whir_pcs_sparse_bench.py.  pk_probe_whir_sparse_sums: pkw_sparse_sums on a grid of
 * `grid` workgroups per weight (0 or 1..pk_probe_whir_wsum_grid(n_vars)).  pk_probe_whir_sparse_grid: the grid the library takes for
 * weights of at most nnz entries at `steps` steps per workgroup (1: the sums, 8: the evaluation).  pk_probe_sparse_tile_host: the
 * sums kernel's lanes on the HOST (two slices of two polynomials, as on the device), f = 4 x terms gathered elements, w = terms values, out = 4 elements.  pk_probe_sparse_eq_host:
 * sum_k value[k] * eq(index[k], point) by the host verifier's chunked eq tables. */
unsigned pk_probe_whir_sparse_threads(void);
unsigned pk_probe_whir_sparse_chunk_bits(void);
unsigned pk_probe_whir_sparse_grid(unsigned n_vars, size_t nnz, unsigned steps);
int pk_probe_whir_sparse_sums(pk_ctx *ctx, const uint64_t *const *d_evals, unsigned batch, unsigned n_vars, const uint64_t *offsets,
                              const uint32_t *d_index, const uint64_t *d_value, unsigned l, unsigned grid, uint64_t *out);
int pk_probe_sparse_tile_host(const uint64_t *f, const uint64_t *w, unsigned terms, uint64_t *out);
int pk_probe_sparse_eq_host(unsigned n_vars, const uint64_t *point, const uint32_t *index, const uint64_t *value, size_t nnz, uint64_t *out);

/* ... and its hiding stage (csrc/whir_pcs/hiding.hip; whir_hiding.hip here), for tests/test_gpu_whir_pcs_hiding.py and
 * tools/whir_pcs_hiding_bench.py.  pk_probe_whir_hiding_fill: the one launch of pkw_commit_hiding on a grid of `grid` workgroups
 * (0: pk_probe_whir_hiding_grid(polys, n)): d_tables = HOST array of polys + 1 device tables of 2^(n+1) elements; the upper halves
 * of the first `polys` take the masks, the last table takes g, the lower halves are not touched.  polys 1..3, n 1..29.  The grid
 * rule is one workgroup per threads * pairs_per_lane pairs of the (polys + 2) * 2^(n-1), rounded up. */
int pk_probe_whir_hiding_fill(pk_ctx *ctx, uint64_t *const *d_tables, unsigned polys, unsigned n, const uint8_t key32[32], unsigned grid);
unsigned pk_probe_whir_hiding_grid(unsigned polys, unsigned n);
unsigned pk_probe_whir_hiding_threads(void);
unsigned pk_probe_whir_hiding_pairs_per_lane(void);

/* libprovekit_lookup.so's gather by itself (csrc/lookup/kernels.hpp), for tools/lookup_bench.py: staged != 0 its LDS-staged kernel
 * (k <= pkl_gather_lds_max_k()), staged == 0 the kernel that reads through L2, whatever the library's rule would pick; grid 0: the
 * kernel's own rule.  d_g, d_dt: 2^k elements; d_idx: 2^n indices; d_hf, d_df: 2^n elements, written.  *ms: the launch's device
 * time.  Blocking. */
int pk_probe_lookup_gather(pk_ctx *ctx, const uint32_t *d_idx, const uint64_t *d_g, const uint64_t *d_dt, unsigned n, unsigned k, uint64_t *d_hf,
                           uint64_t *d_df, int staged, unsigned grid, float *ms);
/* A pkl_prover's test and benchmark knobs, which the library's C ABI does not carry (csrc/lookup/prover.hpp).  Host only.
 * pk_probe_lookup_set_grid: the workgroups of the prover's own kernels from the next call on, 1 .. 1024; 0: each kernel's rule.  No
 * bit of any result depends on it (tests/test_gpu_lookup.py).
 * pk_probe_lookup_profile: the last proof's phases in milliseconds -- ms5[0..3): count, table, gather, device time between events
 * around each phase's launches; ms5[3..5): the f side's and the t side's pks_prove, host time.  A phase that has not run reads 0. */
struct pkl_prover;
int pk_probe_lookup_set_grid(struct pkl_prover *p, unsigned grid);
int pk_probe_lookup_profile(const struct pkl_prover *p, double *ms5);

/* libprovekit_grandproduct.so's tree kernels by themselves (csrc/grandproduct/kernels.hpp) with the two knobs its C ABI does not carry:
 * layers per launch of tree_kernel / leaf_kernel (1 .. 3; 0: the library's value, pk_probe_grandproduct_default_layers) and the grid
 * (1 .. 1024; 0: one lane per low index).  No bit of any layer depends on either (tests/test_gpu_grandproduct.py).  d_v, d_tree,
 * d_leaf: 2^n elements; d_cols: w device pointers (a host array); gamma, beta: one host element each.  *ms: the launches' device
 * time.  Blocking. */
int pk_probe_grandproduct_tree(pk_ctx *ctx, unsigned n, const uint64_t *d_v, uint64_t *d_tree, unsigned layers, unsigned grid, float *ms);
int pk_probe_grandproduct_leaf_tree(pk_ctx *ctx, unsigned n, unsigned w, const uint64_t *const *d_cols, const uint64_t *gamma, const uint64_t *beta,
                                    uint64_t *d_leaf, uint64_t *d_tree, unsigned layers, unsigned grid, float *ms);
unsigned pk_probe_grandproduct_default_layers(void);
/* A pkg_prover's test and benchmark knobs (csrc/grandproduct/prover.hpp).  Host only.  pk_probe_grandproduct_set_knobs: the same two
 * knobs for the prover's proofs from the next call on.  pk_probe_grandproduct_profile: the last proof's tree phase in milliseconds of
 * device time (events around its launches) and layer_ms28[d], 1 <= d < n, layer d's pks_prove in host time; what has not run reads 0.
 * pk_probe_multiset_inner: the pkg_prover a multiset prover proves both sides through (its profile is the side proved last, B). */
struct pkg_prover;
struct pkg_multiset_prover;
int pk_probe_grandproduct_set_knobs(struct pkg_prover *p, unsigned layers, unsigned grid);
int pk_probe_grandproduct_profile(const struct pkg_prover *p, double *tree_ms, double *layer_ms28);
struct pkg_prover *pk_probe_multiset_inner(struct pkg_multiset_prover *p);

/* libprovekit_fracsum.so's kernels by themselves (csrc/fracsum/kernels.hpp) with the two knobs its C ABI does not carry: layers per
 * launch of frac_tree_kernel / lookup_leaf_kernel (1 .. 3; 0: the library's value, pk_probe_fracsum_default_layers) and the grid
 * (1 .. 1024; 0: one lane per index).  No bit of any layer depends on either (tests/test_gpu_fracsum.py).  d_p (NULL: unit
 * numerators), d_q, d_table, d_m (NULL: unit), d_leaf, d_ptree, d_qtree: 2^n elements; alpha, lambda: one host element each;
 * pk_probe_fracsum_combine: d_u[x] = d_pR[x] (NULL: 1) + lambda d_qR[x] for x < count.  *ms: the launches' device time.  Blocking. */
int pk_probe_fracsum_tree(pk_ctx *ctx, unsigned n, const uint64_t *d_p_or_null, const uint64_t *d_q, uint64_t *d_ptree, uint64_t *d_qtree,
                          unsigned layers, unsigned grid, float *ms);
int pk_probe_fracsum_lookup_leaf(pk_ctx *ctx, unsigned n, const uint64_t *d_table, const uint64_t *d_m_or_null, const uint64_t *alpha,
                                 uint64_t *d_leaf, uint64_t *d_ptree, uint64_t *d_qtree, unsigned layers, unsigned grid, float *ms);
int pk_probe_fracsum_combine(pk_ctx *ctx, size_t count, const uint64_t *d_pR_or_null, const uint64_t *d_qR, const uint64_t *lambda, uint64_t *d_u,
                             unsigned grid, float *ms);
unsigned pk_probe_fracsum_default_layers(void);
/* A pkf_prover's test and benchmark knobs (csrc/fracsum/prover.hpp).  Host only.  pk_probe_fracsum_set_knobs: the same two knobs for
 * the prover's proofs from the next call on.  pk_probe_fracsum_profile: in milliseconds, the last proof's tree phase and, for
 * 1 <= d < n, combine_ms28[d] layer d's combine pass in device time (events around their launches), and layer_ms28[d] layer d's
 * pks_prove in host time; what has not run reads 0.  pk_probe_fracsum_lookup_side: the pkf_prover of a lookup prover's side (PKF_SIDE_*). */
struct pkf_prover;
struct pkf_lookup_prover;
int pk_probe_fracsum_set_knobs(struct pkf_prover *p, unsigned layers, unsigned grid);
int pk_probe_fracsum_profile(const struct pkf_prover *p, double *tree_ms, double *combine_ms28, double *layer_ms28);
struct pkf_prover *pk_probe_fracsum_lookup_side(struct pkf_lookup_prover *p, int side);

/* libprovekit_tuplelookup.so's leaf kernel by itself (csrc/tuplelookup/kernels.hpp) with the grid its C ABI does not carry (workgroups
 * per group, 1 .. 1024; 0: the library's rule, pk_probe_tuple_leaf_items rows per lane).  No bit of the leaves depends on it
 * (tests/test_gpu_tuplelookup.py).  d_cols: c * w device pointers on the host, as pkt_leaves; *ms: the launch's device time.  Blocking.
 * A pkt_prover's test and benchmark knobs (csrc/tuplelookup/prover.hpp), host only: pk_probe_tuple_set_grid sets the grid of its leaf
 * AND count kernels from the next call on; pk_probe_tuple_profile: in milliseconds, the last proof's two leaf launches and the last
 * pkt_multiplicities' count and mont launches in device time, and side_ms2[PKT_SIDE_*] the two pkf_prove in host time. */
struct pkt_prover;
int pk_probe_tuple_leaves(pk_ctx *ctx, unsigned n, unsigned w, unsigned c, const uint64_t *const *d_cols, const uint64_t *alpha, const uint64_t *beta,
                          uint64_t *d_leaf, unsigned grid, float *ms);
int pk_probe_tuple_set_grid(struct pkt_prover *p, unsigned grid);
int pk_probe_tuple_profile(const struct pkt_prover *p, double *leaf_ms, double *count_ms, double *side_ms2);
unsigned pk_probe_tuple_leaf_items(void);

/* libprovekit_memcheck.so's two leaf kernels by themselves (csrc/memcheck/kernels.hpp) with the grid its C ABI does not carry (1 .. 1024
 * workgroups; 0: the library's rule, pk_probe_mem_leaf_items rows per lane).  No bit of the tables depends on it
 * (tests/test_gpu_memcheck.py).  Arguments as pkm_leaves; ms2: the device time of the pass over the operations, then the cells.  Blocking.
 * A pkm_prover's test and benchmark knobs (csrc/memcheck/prover.hpp), host only: pk_probe_mem_set_grid sets the grid of every kernel of
 * its traces and proofs from the next call on; pk_probe_mem_profile: in milliseconds, trace_ms4 the last pkm_trace's key, sort, resolve
 * and count phases and *leaf_ms the last proof's two leaf launches in device time, and side_ms3[PKM_SIDE_*] the three inner proofs in
 * host time.  pk_probe_mem_trace_items: the rows per lane the trace builder's grid rule aims at; pk_probe_mem_count_lds_max_n: up to
 * 2^this bins the time side's histogram is counted in LDS. */
struct pkm_prover;
struct pkm_columns;
int pk_probe_mem_leaves(pk_ctx *ctx, unsigned n, unsigned k, const struct pkm_columns *cols, const uint64_t *gamma, const uint64_t *beta, uint64_t *d_ops,
                        uint64_t *d_mem, uint64_t *d_f_or_null, unsigned grid, float *ms2);
int pk_probe_mem_set_grid(struct pkm_prover *p, unsigned grid);
int pk_probe_mem_profile(const struct pkm_prover *p, double *trace_ms4, double *leaf_ms, double *side_ms3);
unsigned pk_probe_mem_leaf_items(void);
unsigned pk_probe_mem_trace_items(void);
unsigned pk_probe_mem_count_lds_max_n(void);

/* libprovekit_spark.so's gather kernel by itself (csrc/spark/kernels.hpp) over tables the caller holds, with the grid its C ABI does not
 * carry (1 .. 1024 workgroups; 0: the library's rule, pk_probe_spark_gather_items entries per lane): d_eq_row 2^s and d_eq_col 2^t
 * elements, d_bad one u64 cell (all ones afterwards: every index was inside).  *ms: its device time.  Blocking.
 * A pkx_prover's test and benchmark knobs (csrc/spark/prover.hpp), host only: pk_probe_spark_set_grid sets the grid of every kernel of
 * its calls from the next call on -- no bit of a result depends on it (tests/test_gpu_spark.py); pk_probe_spark_profile: in
 * milliseconds, matrix_ms2 the last pkx_matrix's count and column phases and *gather_ms the last pkx_begin's gather in device time,
 * *eq_ms the last proof's two eq tables and side_ms3[PKX_SIDE_*] its three inner proofs in host time.  pk_probe_spark_matrix_items:
 * the entries per lane the preprocessing kernels' grid rule aims at. */
struct pkx_prover;
int pk_probe_spark_gather(pk_ctx *ctx, unsigned n, unsigned s, unsigned t, const uint32_t *d_row_idx, const uint32_t *d_col_idx, const uint64_t *d_eq_row,
                          const uint64_t *d_eq_col, uint64_t *d_e_row, uint64_t *d_e_col, unsigned long long *d_bad, unsigned grid, float *ms);
int pk_probe_spark_set_grid(struct pkx_prover *p, unsigned grid);
int pk_probe_spark_profile(const struct pkx_prover *p, double *matrix_ms2, double *gather_ms, double *eq_ms, double *side_ms3);
unsigned pk_probe_spark_gather_items(void);
unsigned pk_probe_spark_matrix_items(void);

/* libprovekit_rangecheck.so's decomposition pass by itself (csrc/rangecheck/kernels.hpp) over tables the caller holds, with the grid its
 * C ABI does not carry (1 .. 1024 workgroups; 0: the library's rule, pk_probe_range_decompose_items entries per lane): d_limbs L device
 * pointers on the host, d_counts 2^k u32, d_bad one u64 cell (all ones afterwards: every entry was below 2^bits), d_m 2^k elements.
 * *ms: its device time, the counts' Montgomery pass included.  Blocking.
 * A pkr_prover's test and benchmark knobs (csrc/rangecheck/prover.hpp), host only: pk_probe_range_set_grid sets the grid of every
 * kernel of its calls from the next call on -- no bit of a result depends on it (tests/test_gpu_rangecheck.py); pk_probe_range_profile:
 * in milliseconds, the last pkr_decompose's launches and the last proof's scale pass in device time, its pkt_prove in host time.
 * pk_probe_range_grids: the workgroups the library's rule gives the decompose, scale (0: none), index and m kernels of a statement. */
struct pkr_prover;
int pk_probe_range_decompose(pk_ctx *ctx, unsigned n, unsigned bits, unsigned k, const uint64_t *d_f, uint64_t *const *d_limbs, uint32_t *d_counts,
                             unsigned long long *d_bad, uint64_t *d_m, unsigned grid, float *ms);
int pk_probe_range_set_grid(struct pkr_prover *p, unsigned grid);
int pk_probe_range_profile(const struct pkr_prover *p, double *decompose_ms, double *scale_ms, double *lookup_ms);
int pk_probe_range_grids(unsigned n, unsigned bits, unsigned k, unsigned *grids4);
unsigned pk_probe_range_decompose_items(void);

/* libprovekit_bitwise.so's decomposition pass by itself (csrc/bitwise/kernels.hpp) over tables the caller holds, with the grid its C
 * ABI does not carry (1 .. 1024 workgroups; 0: the library's rule, pk_probe_bitwise_decompose_items entries per lane): d_c written
 * (c_given = 0) or read and compared, d_digits 3 L device pointers on the host ([j L + i]), d_counts 2^(2d) u32, d_bad one u64 cell
 * (all ones afterwards: no entry failed; else (x << 2) | case of the smallest failing x), d_m 2^(2d) elements.  *ms: its device time,
 * the counts' Montgomery pass included.  Blocking.
 * A pkb_prover's test and benchmark knobs (csrc/bitwise/prover.hpp), host only: pk_probe_bitwise_set_grid sets the grid of every
 * kernel of its calls from the next call on -- no bit of a result depends on it (tests/test_gpu_bitwise.py); pk_probe_bitwise_profile:
 * in milliseconds, the last pkb_decompose's launches in device time, the last proof's pkt_prove in host time.
 * pk_probe_bitwise_grids: the workgroups the library's rule gives the decompose, table and m kernels of a statement. */
struct pkb_prover;
int pk_probe_bitwise_decompose(pk_ctx *ctx, unsigned n, unsigned op, unsigned d, unsigned L, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_c, int c_given,
                               uint64_t *const *d_digits, uint32_t *d_counts, unsigned long long *d_bad, uint64_t *d_m, unsigned grid, float *ms);
int pk_probe_bitwise_set_grid(struct pkb_prover *p, unsigned grid);
int pk_probe_bitwise_profile(const struct pkb_prover *p, double *decompose_ms, double *lookup_ms);
int pk_probe_bitwise_grids(unsigned n, unsigned op, unsigned d, unsigned L, unsigned *grids3);
unsigned pk_probe_bitwise_decompose_items(void);

/* csrc/witness.hip's thresholds (csrc/witness_shape.hpp) and the shape of a levelled builder list (witness.hip here), for
 * tests/test_witness_edge_cases_host.py and tests/test_gpu_witness_edges.py.  Host only.  pk_probe_witness_phases: *n_phases = the
 * phases of postcard(Vec<WitnessBuilder>) after levelling (two per level); with cap >= *n_phases, widths[ph] = the items of phase
 * ph, op_counts[ph * pk_probe_witness_n_ops() + op] = its items of variant op, blocks_before[ph] = the Spice blocks and long sums
 * that run right before it (each of the three may be null).  A list the library refuses: PK_ERR_BAD_ARG, the reason in err. */
unsigned pk_probe_witness_narrow(void);
unsigned pk_probe_witness_sum_heavy(void);
unsigned pk_probe_witness_sum_chunk(void);
unsigned pk_probe_witness_n_ops(void);
int pk_probe_witness_phases(const uint8_t *bytes, size_t len, uint32_t *widths, uint32_t *op_counts, uint32_t *blocks_before, size_t cap,
                            size_t *n_phases, char *err, size_t err_cap);

/* csrc/r1cs.hip's thresholds (csrc/r1cs_shape.hpp: a line of more than heavy_degree entries is summed by workgroups, heavy_chunk
 * entries each), the terms per Montgomery reduction of its dot product (csrc/fe29.hpp DOT29_GROUP) and the lanes a chunk's entries
 * are strided by (csrc/reduce.hpp RED_THREADS); the two entry points only the sharded prover calls (csrc/internal.hpp: their own
 * argument order, device pointers the caller owns); and pk_probe_dot29_host: the loop of a line's dot product on the HOST,
 * out = sum_t a[t] * b[t] * 2^-256 mod p over `terms` pairs of 4 x u64 (a: the first factors, where the interned values go).  For
 * tests/test_r1cs_edge_cases_host.py and tests/test_gpu_r1cs_edges.py (r1cs.hip here). */
unsigned pk_probe_r1cs_heavy_degree(void);
unsigned pk_probe_r1cs_heavy_chunk(void);
unsigned pk_probe_dot29_group(void);
unsigned pk_probe_reduction_threads(void);
int pk_probe_r1cs_witness_bounds_strided(pk_ctx *ctx, const pk_r1cs *r, const uint64_t *d_z, unsigned m0, unsigned stride, unsigned offset,
                                         uint64_t *d_a, uint64_t *d_b, uint64_t *d_c);
int pk_probe_r1cs_external_row_range(pk_ctx *ctx, const pk_r1cs *r, const uint64_t *d_eq, size_t first, size_t last, uint64_t *d_out);
int pk_probe_dot29_host(const uint64_t *a, const uint64_t *b, unsigned terms, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
