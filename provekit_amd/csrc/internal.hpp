// internal.hpp -- the library's internal interface: every `pk::` function that one translation unit of libprovekit_hip defines and
// another calls, grouped by the file that defines it.  Every .hip includes this header -- the defining file too, so a definition that
// drifts from what its callers compile against (parameters, return type, default) is a compile error, not a surprise at load time.
// The opaque handles (pk_tree, pk_r1cs, pk_witness_program) and pk_commit_layout are declared by the public header.
#pragma once
#include "ctx.hpp"
#include "rng_core.hpp"  // RngKey, the cipher block and the accept rule

namespace pk {

// ---- ctx.hip ------------------------------------------------------------------------------------------------------------------
int ensure_scratch(pk_ctx* ctx, size_t bytes);
int ensure_pinned(pk_ctx* ctx);  // the 4 KiB result page
int ensure_ws(pk_ctx* ctx, size_t bytes);
// test hooks, settable only through pk_selftest_set_hook (tools/probes/pk_selftest.h); 0 = off: a gated kernel's spin bound, microseconds the
// host sleeps before it publishes a gate's challenge, take the RCCL branch for a repeated device
enum { PK_HOOK_GATE_SPINS = 0, PK_HOOK_GATE_STALL_US = 1, PK_HOOK_RCCL_SAME_DEVICE = 2, PK_HOOK_COUNT = 3 };
long test_hook(int which);
// Every wait of the library for a stream goes through here (pk_device_set_host_wait): the runtime's hipStreamSynchronize -- spinning or
// blocking, whichever the device's scheduling flag says -- or, in PK_WAIT_POLL, the library's own loop: hipStreamQuery with short sleeps.
hipError_t wait_stream(int device, hipStream_t stream);
hipError_t wait_ctx(pk_ctx* ctx);  // wait_stream on the context's stream; with a deadline while an RCCL collective is pending on it (comm.hip comm_wait)
int wait_ctx_rc(pk_ctx* ctx);      // the same as a status: PK_OK, PK_ERR_RCCL (the collective failed or timed out; pk_last_error says which) or PK_ERR_HIP
int sync_stream(pk_ctx* ctx);                           // wait_stream + rewind the mailbox
int mail_alloc(pk_ctx* ctx, size_t bytes, void** out);  // 64-B aligned; valid until the next sync_stream

// ---- comm.hip: rank / size of the context's communicator (0 / 1 without one) and its collectives, enqueued on ctx->stream ----------
int comm_rank(const pk_ctx* ctx);
int comm_world(const pk_ctx* ctx);
int comm_all_gather(pk_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_rank);
int comm_all_reduce_sum_u64(pk_ctx* ctx, uint64_t* d_buf, size_t count);
int comm_collect_fe(pk_ctx* ctx, int K, uint64_t* host_out);  // the cross-rank half of collect_reduction (reduce.hpp)
int red_across_begin(pk_ctx* ctx);                            // allocate d_xred if needed and set red_across
bool comm_collective_pending(const pk_ctx* ctx);
bool comm_rccl(const pk_ctx* ctx);
hipError_t comm_wait(pk_ctx* ctx);
void comm_turn_begin(pk_ctx* ctx);  // measurement aid of the in-process transport (LocalGroup::turnstile)
void comm_turn_end(pk_ctx* ctx);
unsigned long long comm_collectives_issued(const pk_ctx* ctx);  // collectives this context's communicator has enqueued so far
void comm_abort(pk_ctx* ctx);  // this rank will not reach a collective its peers wait in: LOCAL wakes them; RCCL aborts its OWN communicator (the peers time out, comm_wait)
void comm_release(pk_ctx* ctx);

// ---- hash.hip -----------------------------------------------------------------------------------------------------------------
// leaf hash of a column-major codeword in the commit's internal (hash-ready) encoding, or in Montgomery form
int leaf_hash_x(pk_ctx* ctx, const uint64_t* d_leaves, size_t n_leaves, size_t width, uint64_t* d_digests, bool scaled_in);
int merkle_top_x(pk_ctx* ctx, uint64_t* d_nodes, size_t top_leaves);  // the levels above heap slots [top_leaves, 2 top_leaves)
int read_root(pk_ctx* ctx, const uint64_t* d_nodes, size_t n_leaves, uint64_t root[4]);  // after pk_merkle_*

// ---- ntt.hip ------------------------------------------------------------------------------------------------------------------
void ntt_retain_ctx(pk_ctx* ctx);   // one more context on this device shares its twiddle tables
void ntt_release_ctx(pk_ctx* ctx);  // the context lets go of the device's twiddle tables (freed with the last context)
bool ntt_scaled_available(unsigned log_n);  // can a transform of this size deliver the hash-ready encoding?
// the two encodes with a choice of output encoding (scaled = hash-ready)
int rs_encode_x(pk_ctx* ctx, const uint64_t* const* d_coeffs, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold,
                uint64_t* d_leaves, uint64_t* d_scratch, bool scaled);
int rs_encode_shard_x(pk_ctx* ctx, const uint64_t* const* d_coeffs, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold,
                      unsigned shard, unsigned n_shards, uint64_t* d_leaves_local, uint64_t* d_scratch, bool scaled);

// ---- pow.hip ------------------------------------------------------------------------------------------------------------------
// striped: every rank of the context's device set is inside this call with the same challenge and searches its stripe of each window
int pow_solve_x(pk_ctx* ctx, const uint8_t challenge[32], double bits, uint64_t* nonce, bool striped);

// ---- tree.hip -----------------------------------------------------------------------------------------------------------------
unsigned shard_factor(const pk_ctx* ctx, size_t rows);  // 1 = a commit of `rows` leaves is computed whole on every rank, G = sharded over the G ranks
size_t commit_scratch_fes(const pk_ctx* ctx, size_t rows, size_t width);  // device scratch (in FEs) commit_into needs
// RS-encode + Merkle commit into caller-owned device buffers (no allocation)
int commit_into(pk_ctx* ctx, const uint64_t* const* d_coeffs, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold,
                uint64_t* d_leaves, uint64_t* d_nodes, uint64_t* d_scratch, pk_commit_layout* layout_out);
// open k leaves of a tree described by raw buffers (same outputs as pk_tree_open)
int open_raw(pk_ctx* ctx, const uint64_t* d_leaves, const uint64_t* d_nodes, size_t n_leaves, size_t width, const pk_commit_layout& lay,
             const uint64_t* indices, size_t k, int canonical_leaves, uint64_t* leaves_out, uint64_t* sibling_digests, uint64_t* auth_paths);

// ---- mle.hip ------------------------------------------------------------------------------------------------------------------
// np (1 or 2) polynomials of n coefficients each at the same z, one launch: out[4 * q] = poly_q(z)
int eval_univariate_multi(pk_ctx* ctx, const uint64_t* const* d_polys, unsigned np, size_t n, const uint64_t z[4], uint64_t* out);
// nrows (= 3) weight rows against f and (d_g != null: nv = 2) g in one pass: out[4 * (nv * k + v)]
// defer: launch only -- the caller synchronises `ctx`'s stream later and takes the 3 * nv results from its pinned page (latency mode: the
// statement's sums run on a side stream underneath the blinding WHIR proof)
int dot_rows(pk_ctx* ctx, const uint64_t* d_w, size_t row_stride, unsigned nrows, const uint64_t* d_f, const uint64_t* d_g, size_t n, uint64_t* out,
             bool defer = false);
// the same against the equality table of `point` (n_vars host elements, eval_eq's order) over the rows' first n entries, nrows = 1 or 3:
// out[4 * k] = <row k, eq(point, .)>.  The table is never written: the lane forms each entry from the point's two half tables.
int dot_rows_eq(pk_ctx* ctx, const uint64_t* d_w, size_t row_stride, unsigned nrows, const uint64_t* point, unsigned n_vars, size_t n, uint64_t* out);
// Round 0 of a quadratic sumcheck (no fold) in the launch that forms its tables p and w, n entries each (a power of two >= 2):
//   the opening's first launch: p = e0 + beta e1;  w = (overwrite ? 0 : w) + sum_j scales[j] eq(points[j], .) + sum_k row_scales[k] row_k, row k at
//     d_rows + k * row_stride, nrows = 1 or 3 rows of row_len <= n leading entries;  nsums = 2 or 3
//   a round's new weights:      d_e0 = null, nrows = 0: p stands;  w as above without rows;  nsums = 3
// points (q x log2 n), scales, beta, row_scales: host.  p, w and the sums carry the bits pk_eq_accumulate, pk_fe_axpy / axpy3, lincomb2 and
// sumcheck_quadratic_launch (no fold) leave.  grid: 0, or a cap on the workgroups (tests).  Launch only, as sumcheck_quadratic_launch.
struct opening_first {
    const uint64_t *d_e0, *d_e1, *beta;
    uint64_t *d_p, *d_w;
    size_t n;
    const uint64_t *points, *scales;
    unsigned q;
    int overwrite;
    const uint64_t* d_rows;
    size_t row_stride;
    unsigned nrows;
    size_t row_len;
    const uint64_t* row_scales;
    int nsums;
};
int opening_first_launch(pk_ctx* ctx, const opening_first& a, unsigned grid, unsigned* red_seq_out);
int lincomb2(pk_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* beta, const uint64_t* d_b, size_t n);  // out = a + beta * b
// out0 = a0 + beta * b0 over n0 entries and out1 = a1 + beta * b1 over n1 in one launch (a batch of two: coefficient and evaluation tables)
int lincomb2_pair(pk_ctx* ctx, uint64_t* d_out0, const uint64_t* d_a0, const uint64_t* d_b0, size_t n0, uint64_t* d_out1, const uint64_t* d_a1,
                  const uint64_t* d_b1, size_t n1, const uint64_t* beta);
// y += g3[0] r0 + g3[1] r1 + g3[2] r2 over n entries, row k at d_rows + k * row_stride elements: one pass over y (the bits three pk_fe_axpy calls leave)
int axpy3(pk_ctx* ctx, uint64_t* d_y, const uint64_t* g3, const uint64_t* d_rows, size_t row_stride, size_t n);
// f = [witness (zero padded to 2^(m-1)) || draw stream_mask], g = draw stream_g, both of 2^m elements: the evaluation tables AND their
// to_coeffs, the tables assembled inside the first sweep instead of by a memset, a copy and two random_fe launches before it
int to_coeffs_generated(pk_ctx* ctx, unsigned m, const uint64_t* d_wit, size_t n_wit, const RngKey& key, uint32_t stream_mask, uint32_t stream_g,
                        uint64_t* d_f_evals, uint64_t* d_g_evals, uint64_t* d_f_coeffs, uint64_t* d_g_coeffs);
// two arrays of the same length folded by the same challenge in one launch (the sumcheck's p and w)
// r = NULL with gate_seq != 0: the challenge arrives through the gate (latency mode)
int fold_pairs2(pk_ctx* ctx, const uint64_t* d_v0, uint64_t* d_out0, const uint64_t* d_v1, uint64_t* d_out1, size_t len, const uint64_t* r,
                unsigned gate_seq = 0);
// count (1 .. 4) runs of n[k] elements at d_src[k], back to back into host_out: one launch that writes the context's mailbox, one
// synchronisation (the host tail's transfer of a sumcheck's short tables; at most 4 * 2^PK_HOST_TAIL_MAX_LOG2 elements in all)
int tables_to_host(pk_ctx* ctx, const uint64_t* const* d_src, const size_t* n, unsigned count, uint64_t* host_out);
// launch only: round results go to the pinned page under sequence number *red_seq_out.  gate_seq != 0 (latency mode, folding rounds
// only): the folding challenge is not known yet -- the kernel waits for sumcheck_gate_publish(ctx, gate_seq, challenge).
// The weight of the cubic round's pairs is d_weight, one of two kinds:
//   EqArray: the eq table, folded in place with a, b, c; the sums are the round's f(0), f(-1), f_inf;
//   Level:   the level E_i of the round the kernel evaluates (eq_suffix_tables below; npairs entries, read only); the sums are Q(0), Q(-1), Q_inf.
enum class CubicWeight { EqArray, Level };
int sumcheck_cubic_launch(pk_ctx* ctx, uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, CubicWeight kind, uint64_t* d_weight, size_t len,
                          const uint64_t* fold_or_null, unsigned gate_seq, unsigned* red_seq_out);
// nsums = 3: the sums are h(0), h(1), h(2); nsums = 2: h(0), h(2) -- the caller holds the round's claim h(0) + h(1) (sumcheck_quadratic_from_claim)
int sumcheck_quadratic_launch(pk_ctx* ctx, const uint64_t* d_f, const uint64_t* d_w, size_t len, const uint64_t* fold_or_null, unsigned gate_seq,
                              uint64_t* d_f_out, uint64_t* d_w_out, int nsums, unsigned* red_seq_out);
void sumcheck_quadratic_from_claim(const uint64_t claim[4], uint64_t out[12]);  // out = h(0), h(2)  ->  h(0), claim - h(0), h(2)
// The cubic round without the eq array.  eq_suffix_tables: the levels E_i = eq(r[i+1 .. n), .), i = 0 .. n-1, back to back in 2^n elements
// (E_i at 2^n - 2^(n-i)).  sumcheck_cubic_launch(CubicWeight::Level) takes the level of the round it evaluates and returns Q(0), Q(-1), Q_inf;
// sumcheck_spliteq_correct turns them into the round's f(0), f(-1), f_inf with P = prod_{k<i} eq(r_k, alpha_k), which sumcheck_spliteq_advance
// carries from round to round.
int eq_suffix_tables(pk_ctx* ctx, const uint64_t* r, unsigned n, uint64_t* d_out);
void sumcheck_spliteq_correct(const uint64_t P[4], const uint64_t r_i[4], uint64_t out[12]);
void sumcheck_spliteq_advance(uint64_t P[4], const uint64_t r_i[4], const uint64_t alpha_i[4]);
// the host's side of a gated launch and the wait for a launch's results without draining the stream (latency mode); without a gate: after a stream sync
int sumcheck_collect_spin(pk_ctx* ctx, int nsums, unsigned red_seq, uint64_t out[12]);
int sumcheck_collect(pk_ctx* ctx, int nsums, uint64_t out[12]);
unsigned sumcheck_gate_next(pk_ctx* ctx);
void sumcheck_gate_publish(pk_ctx* ctx, unsigned gate_seq, const uint64_t challenge[4]);
int sumcheck_gate_check(pk_ctx* ctx);   // PK_OK, or PK_ERR_HIP with the message set: a gated kernel of this context gave up on its challenge since the last call
void sumcheck_gate_clear(pk_ctx* ctx);  // forget a give-up word without touching the error message

// ---- r1cs.hip -----------------------------------------------------------------------------------------------------------------
// rank `offset` of `stride` ranks: a, b, c for the rows i = j * stride + offset, j < 2^m0 / stride (sharded sumcheck)
int witness_bounds_strided(pk_ctx* ctx, const pk_r1cs* r, const uint64_t* d_z, unsigned m0, unsigned stride, unsigned offset, uint64_t* d_a,
                           uint64_t* d_b, uint64_t* d_c);
// columns [first, last) of the three external rows, written at their absolute positions of d_out (3 x num_witnesses)
int external_row_range(pk_ctx* ctx, const pk_r1cs* r, const uint64_t* d_eq_alpha, size_t first, size_t last, uint64_t* d_out);

// ---- rng.hip: the proof RNG ---------------------------------------------------------------------------------------------------
enum { RNG_MASK = 1, RNG_G = 2, RNG_BLIND = 3, RNG_MASK_B = 4, RNG_G_B = 5, RNG_FILL = 6 };  // draws of one proof (the `stream` word of the nonce)
int proof_key(pk_ctx* ctx, const uint8_t* rng_seed32, RngKey& key);  // fresh from the OS unless injected; the same on every rank of a device set
int random_fe(pk_ctx* ctx, uint64_t* d_out, size_t n, const RngKey& key, uint32_t stream);  // launch only

// ---- witness.hip --------------------------------------------------------------------------------------------------------------
void witness_program_shape(const pk_witness_program* p, size_t* n_witnesses, size_t* n_challenges, size_t* n_acir);
// host only, for the lab: decode and level a postcard list; items per phase, items per phase and variant (wb::N_OPS per phase,
// witness_shape.hpp), the Spice blocks and long sums that run right before each phase
int witness_phase_shape(const uint8_t* bytes, size_t len, std::vector<uint32_t>& widths, std::vector<uint32_t>& op_counts, std::vector<uint32_t>& blocks_before,
                        std::string& error);

// ---- whir_config.hip: the scheme's shape (host only) --------------------------------------------------------------------------
const char* whir_config_error(const pk_whir_config* c);  // nullptr if this prover runs `c`, else why not
unsigned blinding_log_len(unsigned m_0);                 // the blinding polynomial's variables less one
size_t scheme_arena_bytes(unsigned m, unsigned m_0, size_t num_witnesses, const pk_whir_config& w);
std::string whir_r1cs_io_pattern(unsigned m_0, const pk_whir_config& w, const pk_whir_config& h);
std::string witness_io_pattern(size_t n_public, size_t n_challenges);
// "" if the caller's IO-pattern bytes declare the operations pk_prove performs for (m_0, w, h), else the first difference
std::string io_pattern_mismatch(const std::string& theirs, unsigned m_0, const pk_whir_config& w, const pk_whir_config& h);
void copy_out(const std::string& s, void* buf, size_t cap, size_t* len);  // *len = size; copied where it fits

}  // namespace pk
