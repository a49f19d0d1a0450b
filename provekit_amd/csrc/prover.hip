// prover.hip -- host driver: WhirR1CSProver::prove (provekit/prover/src/whir_r1cs.rs:42-100) over the device kernels.
//
// This is the compiled host side of the drop-in (the reference's is Rust): transcript, challenge bookkeeping and the
// O(m_0^2) blinding algebra run here on the CPU; every data-parallel step is a call into this library's kernels on
// buffers that never leave HBM -- but for the sumchecks' short tails: tables of at most 2^host_tail_log2 entries come to the host once and
// finish there (host_tail.hpp; sumcheck_round_loop below), and for the blinding polynomial, whose tables are that short and depend on the
// proof's key alone: they are drawn on the device, come over once, and its commitment and its whole WHIR proof run on the host thread (host_whir.hpp; Proof::commit_witness below).  One
// proof allocates no device memory: it all comes from a per-scheme arena.
//
//   pk_prove -> prove, one stage per step of the reference (struct Proof)
//    +- commit_witness (whir_r1cs.rs:57-69, 182-209): mask / random polynomial on device, to_coeffs x2, commit_batch; underneath it the
//    |    blinding commitment on the host thread
//    +- zk_sumcheck (whir_r1cs.rs:228-369): witness bounds, eq table, blinding commitment (its transcript half; on the device route all of it), m_0 cubic rounds
//    +- prove_blinding: small WHIR proof of the blinding polynomial (host thread; device route beyond the host tail's threshold)
//    +- witness_statement: external rows, weighted sums, claimed_evaluations hint (whir_r1cs.rs:81-91)
//    +- prove_witness: whir_prove (whir::Prover::prove; structure pinned by recursive-verifier/app/circuit/whir.go:51-220)
//
// In this file: the sharding helpers of one proof over a device set, the blinding algebra, the WHIR prover, the stages of pk_prove,
// and the entry points that share pk_scheme (create / destroy, pk_prove, pk_noir_prove, the scheme's IO pattern).  Elsewhere, reached
// through internal.hpp: the proof RNG and the random draws (rng.hip); the scheme's shape -- config validation and derivation, the
// arena size, the IO patterns -- which needs no device (whir_config.hip).
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "host_tail.hpp"
#include "host_whir.hpp"
#include "internal.hpp"
#include "shard_map.hpp"
#include "prover_transcript.hpp"

using namespace pk;

struct pk_scheme {
    const pk_r1cs* r1cs = nullptr;
    size_t num_constraints = 0, num_witnesses = 0;
    unsigned m = 0, m_0 = 0;
    unsigned nb = 0;  // the blinding polynomial's table: 2^nb = next_power_of_two(4 m_0) coefficients
    pk_whir_config whir_witness{}, whir_hiding{};
    char* arena = nullptr;
    size_t arena_bytes = 0;
    std::string domain_separator;
    char* noir_witness = nullptr;  // pk_noir_prove: num_witnesses elements + num_witnesses is-set bytes, allocated on first use
    pk_ctx* side = nullptr;        // latency mode: a second context (stream, workspace) of the same device for the blinding commitment
};

namespace {

// latency mode: a gated kernel is in the queue waiting for a challenge; whatever path leaves the scope, it must be released
// (with a zero challenge on an error path: the proof is abandoned anyway) so that the stream can drain
struct PendingGate {
    pk_ctx* c;
    unsigned seq = 0;
    explicit PendingGate(pk_ctx* ctx) : c(ctx) {}
    void arm(unsigned s) { seq = s; }
    void publish(const fe& challenge) {
        if (!seq) return;
        const long stall_us = test_hook(PK_HOOK_GATE_STALL_US);  // the test-suite's stand-in for a host thread that was stopped
        if (stall_us > 0) usleep((useconds_t)stall_us);
        uint64_t w[4];
        h_store(w, challenge);
        sumcheck_gate_publish(c, seq, w);
        seq = 0;
    }
    ~PendingGate() {
        if (seq) publish(fe_zero());
    }
};

struct Arena {
    char* base;
    size_t cap, off = 0;
    fe* alloc(size_t n_fe) {
        size_t bytes = ((n_fe * 32 + 255) / 256) * 256;
        if (off + bytes > cap) return nullptr;
        fe* p = (fe*)(base + off);
        off += bytes;
        return p;
    }
};

#define CK(expr)              \
    do {                      \
        int _rc = (expr);     \
        if (_rc) return _rc;  \
    } while (0)
#define ALLOC(var, n)                                                                   \
    fe* var = A.alloc(n);                                                               \
    if (!var) return set_err(ctx, PK_ERR_OOM, "prover arena exhausted (%s)", #var)

inline uint64_t* U(fe* p) { return (uint64_t*)p; }
inline const uint64_t* U(const fe* p) { return (const uint64_t*)p; }

// the context's host-tail threshold in entries (pk_selftest_set_host_tail); 0 = never: switched off, or the context is a rank of a device set
inline size_t host_tail_len(const pk_ctx* ctx) { return !ctx->comm && ctx->host_tail_log2 ? (size_t)1 << ctx->host_tail_log2 : 0; }
// "these tables go to the host tail": `len` entries, whole (not a rank's block), within the threshold.  Every place that asks, asks here.
inline bool host_tail_takes(const pk_ctx* ctx, bool sharded, size_t len) {
    const size_t tail = host_tail_len(ctx);
    return tail && !sharded && len <= tail;
}

// ------------------------------------------------------------------ one proof over a device set
// Besides the commits (tree.hip), the linear-size arrays of a sharded proof are split over the G ranks:
//   * the Spartan sumcheck's a, b, c, eq by the LOW index bits (rank g holds i = g mod G at local index i / G): the leading
//     variable is folded first and pairs i with i + len/2 (sumcheck.rs:28-33), both on one rank, so the existing kernels run
//     unchanged on the local arrays;
//   * the WHIR sumcheck's polynomial and weight tables, the equality weights, the statement weights (external rows) and the
//     OOD evaluations by contiguous BLOCKS (the high index bits): WHIR folds the lowest variable first (pairs 2i, 2i+1).
// Per round every rank reduces its share and the 96 bytes are summed over the ranks (ctx->red_across: reduce.hpp,
// comm_collect_fe); once the local length falls to SHARD_MIN_LOCAL the arrays are all-gathered and the tail of the sumcheck
// runs replicated.  Every sum is an exact field sum, so the transcript is byte-identical to the lone prover's.
constexpr size_t SHARD_MIN_LOCAL = (size_t)1 << 12;

struct Across {  // scope in which this context's reductions are partial sums to be added over the ranks
    pk_ctx* c;
    bool on;
    int rc = PK_OK;
    Across(pk_ctx* ctx, bool enable, const fe* scales = nullptr) : c(ctx), on(enable) {
        if (on) {
            rc = red_across_begin(c);
            c->red_scales = scales;
        }
    }
    ~Across() {
        if (on) {
            c->red_across = false;
            c->red_scales = nullptr;
        }
    }
};
// eq((x_0 .. x_{lg-1}), bits of g), x_0 <-> the most significant of the lg bits (eval_eq's order, sumcheck.rs:146-171)
fe eq_bits(const fe* x, unsigned lg, unsigned g) {
    fe acc = fe_one();
    for (unsigned t = 0; t < lg; t++) acc = h_mul(acc, ((g >> (lg - 1 - t)) & 1u) ? x[t] : h_sub(fe_one(), x[t]));
    return acc;
}
// all-gather of the ranks' local arrays: gathered[r * len + j]; STRIDED additionally re-interleaves to full[j * G + r]
__global__ __launch_bounds__(256) void interleave_fe_kernel(const fe* __restrict__ gathered, fe* __restrict__ full, size_t total, unsigned G) {
    PK_LATENCY_PRIO();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) fe_store(full + i, fe_load(gathered + shard_gathered_slot(i, total, G)));
}
int gather_blocks(pk_ctx* ctx, const fe* local, size_t len, fe* full) { return comm_all_gather(ctx, local, full, 32 * len); }
int gather_strided(pk_ctx* ctx, const fe* local, size_t len, fe* tmp, fe* full) {
    const unsigned G = (unsigned)comm_world(ctx);
    int rc = comm_all_gather(ctx, local, tmp, 32 * len);
    if (rc) return rc;
    const size_t total = len * G;
    interleave_fe_kernel<<<(unsigned)((total + 255) / 256), 256, 0, ctx->stream>>>(tmp, full, total, G);
    PK_LAUNCH_CHECK(ctx);
    return PK_OK;
}
// sum_i c[i] z^i, split into the ranks' blocks when the polynomial is long: rank r evaluates its block in z and the ranks'
// values are combined as sum_r z^(r*B) * partial_r
int eval_univariate_multi_x(pk_ctx* ctx, const fe* const* d_polys, unsigned np, size_t n, const fe& z, fe* out) {
    const unsigned G = (unsigned)comm_world(ctx);
    uint64_t zz[4], o[8];
    h_store(zz, z);
    const uint64_t* ptrs[2] = {nullptr, nullptr};
    if (G > 1 && n / G >= 4 * SHARD_MIN_LOCAL) {
        const size_t B = n / G;
        fe scales[PK_MAX_RANKS];
        const fe zB = h_pow(z, B);
        scales[0] = fe_one();
        for (unsigned r = 1; r < G; r++) scales[r] = h_mul(scales[r - 1], zB);
        for (unsigned q = 0; q < np; q++) ptrs[q] = U(d_polys[q] + (size_t)comm_rank(ctx) * B);
        Across ac(ctx, true, scales);
        CK(ac.rc);
        CK(eval_univariate_multi(ctx, ptrs, np, B, zz, o));
    } else {
        for (unsigned q = 0; q < np; q++) ptrs[q] = U(d_polys[q]);
        CK(eval_univariate_multi(ctx, ptrs, np, n, zz, o));
    }
    for (unsigned q = 0; q < np; q++) out[q] = h_load(o + 4 * q);
    return PK_OK;
}

// ------------------------------------------------------------------ S6: blinding algebra (host, O(m_0^2))
// compute_blinding_coefficients_for_round (provekit/prover/src/whir_r1cs.rs:103-170)
void blinding_coefficients_for_round(const std::vector<fe>& g /*4 per variable*/, size_t compute_for, const fe* alphas, fe out[4]) {
    const size_t n = g.size() / 4;
    bool all_fixed = false;
    if (compute_for == n) {
        all_fixed = true;
        compute_for = n - 1;
    }
    fe prefix_sum = fe_zero();
    for (size_t i = 0; i < compute_for; i++) prefix_sum = h_add(prefix_sum, eval_cubic(&g[4 * i], alphas[i]));
    fe suffix_sum = fe_zero();
    const fe zero = fe_zero(), one = fe_one();
    for (size_t i = compute_for + 1; i < n; i++)
        suffix_sum = h_add(suffix_sum, h_add(eval_cubic(&g[4 * i], zero), eval_cubic(&g[4 * i], one)));
    fe prefix_multiplier = fe_one();
    for (size_t i = 0; i < n - 1 - compute_for; i++) prefix_multiplier = h_add(prefix_multiplier, prefix_multiplier);
    fe suffix_multiplier = h_mul(prefix_multiplier, h_half());
    fe constant = h_add(h_mul(prefix_multiplier, prefix_sum), h_mul(suffix_multiplier, suffix_sum));
    const fe* cur = &g[4 * compute_for];
    fe c[4] = {h_add(h_mul(prefix_multiplier, cur[0]), constant), h_mul(prefix_multiplier, cur[1]), h_mul(prefix_multiplier, cur[2]),
               h_mul(prefix_multiplier, cur[3])};
    if (all_fixed) {
        out[0] = eval_cubic(c, alphas[compute_for]);
        out[1] = out[2] = out[3] = fe_zero();
        return;
    }
    for (int i = 0; i < 4; i++) out[i] = c[i];
}

// ------------------------------------------------------------------ STIR query indices, proof of work (the rules: protocol.hpp)
std::vector<uint64_t> stir_queries(Transcript& T, size_t domain_size, unsigned fold, unsigned num_queries) {
    std::vector<uint8_t> raw(stir_query_bytes(domain_size, fold) * num_queries);
    T.challenge_bytes(raw.data(), raw.size());
    return stir_indexes(raw.data(), domain_size, fold, num_queries);
}

int pow_round(pk_ctx* ctx, Transcript& T, double bits) {
    if (bits <= 0.0) return PK_OK;
    uint8_t challenge[POW_CHALLENGE_BYTES], be[POW_NONCE_BYTES];
    T.challenge_bytes(challenge, sizeof challenge);
    uint64_t nonce = 0;
    int rc = PK_OK;
    // a few bits: ~2^bits host compressions against a launch and a synchronisation (the same nonce: the smallest valid one)
    if (host_tail_len(ctx) && bits <= (double)ctx->host_pow_max_bits) nonce = host_whir::pow_grind(challenge, bits);
    else rc = pow_solve_x(ctx, challenge, bits, &nonce, comm_world(ctx) > 1);  // nonce ranges striped over the ranks of a device set
    nonce_to_bytes(nonce, be);
    T.add_bytes(be, sizeof be);
    return rc;
}

// ------------------------------------------------------------------ WHIR
struct Commitment {  // whir::committer::Witness
    unsigned n_vars = 0, batch = 0;
    fe* polys[4] = {};  // coefficient form
    fe* evals[4] = {};  // the same polynomials as evaluation tables, when the committer still holds them (else null)
    fe* leaves = nullptr;
    fe* nodes = nullptr;
    size_t rows = 0, width = 0;
    // Where polys, evals, leaves and nodes live: in the arena, or -- a commitment of polynomials in host memory (whir_commit_compute, host_whir.hpp) -- in host memory:
    // leaves and nodes in `mem` (shared by the copies of this struct), polys and evals with the caller.  Whoever reads them asks here.
    bool host = false;
    std::shared_ptr<std::vector<fe>> mem;
    pk_commit_layout layout{};    // how commit_into laid the codeword out (shards, leaf encoding): recorded, not recomputed
    std::vector<fe> ood_points;   // Montgomery
    std::vector<fe> ood_answers;  // [poly][point], Montgomery
    fe beta;                      // batching randomness
};
// What the prover asks of a commitment -- its root, its polynomials at a point, its rows opened: the bodies below hold the only tests of
// where it lives.  A device root is read on the context that built the tree.
int commitment_root(pk_ctx* ctx, const Commitment& C, fe& root) {
    if (!C.host) return read_root(ctx, U(C.nodes), C.rows, (uint64_t*)root.v);
    root = C.nodes[1];
    return PK_OK;
}
// polynomials b .. b + np - 1 (np <= 2) at one point: one launch (and one host round trip) on the device, Horner on the host
int commitment_evaluate(pk_ctx* ctx, const Commitment& C, unsigned b, unsigned np, const fe& z, fe* out) {
    const size_t n = (size_t)1 << C.n_vars;
    if (!C.host) return eval_univariate_multi_x(ctx, C.polys + b, np, n, z, out);
    for (unsigned q = 0; q < np; q++) out[q] = host_whir::horner(C.polys[b + q], n, z);
    return PK_OK;
}
// the k rows idx[] (canonical), each row's sibling digest and authentication path
int commitment_open(pk_ctx* ctx, const Commitment& C, const uint64_t* idx, size_t k, uint64_t* leaves, uint64_t* sib, uint64_t* paths) {
    if (!C.host) return open_raw(ctx, U(C.leaves), U(C.nodes), C.rows, C.width, C.layout, idx, k, /*canonical=*/1, leaves, sib, paths);
    host_whir::open(C.leaves, C.nodes, C.rows, C.width, idx, k, (fe*)leaves, (fe*)sib, (fe*)paths);
    return PK_OK;
}

// hints: stir_answers = Vec<Vec<F>> and merkle_proof = ark MultiPath of the commitment's tree at the queried rows (common.go:36-61)
int emit_opening_hints(pk_ctx* ctx, Transcript& T, const Commitment& C, const std::vector<uint64_t>& idx) {
    const size_t k = idx.size(), width = C.width;
    const unsigned logn = ilog2(C.rows);
    const size_t plen = logn ? logn - 1 : 0;
    std::vector<uint64_t> leaves(4 * k * width), sib(4 * (k ? k : 1)), paths(4 * (k * plen ? k * plen : 1));
    CK(commitment_open(ctx, C, idx.data(), k, leaves.data(), sib.data(), paths.data()));
    const auto ser0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> buf;
    put_u64(buf, k);
    for (size_t q = 0; q < k; q++) put_vec(buf, (const fe*)(leaves.data() + 4 * q * width), width, /*montgomery=*/false);
    T.hint(buf.data(), buf.size());
    size_t len = 0;
    pk_multipath_serialize(idx.data(), k, plen, sib.data(), paths.data(), nullptr, 0, &len);
    std::vector<uint8_t> mp(len ? len : 1);
    CK(pk_multipath_serialize(idx.data(), k, plen, sib.data(), paths.data(), mp.data(), len, &len));
    T.hint(mp.data(), len);
    T.hint_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - ser0).count();
    return PK_OK;
}

// CommitmentWriter::commit_batch (call site provekit/prover/src/whir_r1cs.rs:200-206; transcript order mtUtilities.go:51-76)
// the commitment's device work (RS-encode, leaf hashes, tree) on `ctx`'s stream, nothing read back: the half that needs no transcript
// -- in latency mode the blinding commitment's runs on a second stream while the witness commitment fills the chip.  Also the
// re-commit of every WHIR round (batch 1).  host: the polynomials stand in host memory and so will the commitment, computed on the host
// thread (host_whir.hpp): nothing of the arena, no launch.
int whir_commit_compute(pk_ctx* ctx, Arena& A, bool host, unsigned n_vars, unsigned log_inv_rate, unsigned fold, fe* const* polys, unsigned batch,
                        Commitment& C) {
    C.n_vars = n_vars;
    C.batch = batch;
    C.rows = (size_t)1 << (n_vars + log_inv_rate - fold);
    C.width = (size_t)batch << fold;
    for (unsigned b = 0; b < batch; b++) C.polys[b] = polys[b];
    if (host) {
        C.host = true;
        C.mem = std::make_shared<std::vector<fe>>(C.rows * C.width + 2 * C.rows);
        C.leaves = C.mem->data();
        C.nodes = C.leaves + C.rows * C.width;
        C.layout = pk_commit_layout{1, 0, PK_LEAVES_MONTGOMERY};
        host_whir::commit(ctx->hash_version, polys, batch, n_vars, log_inv_rate, fold, C.leaves, C.nodes);
        return PK_OK;
    }
    ALLOC(leaves, C.rows * C.width / shard_factor(ctx, C.rows));  // a rank of a device set keeps only its rows (tree.hip)
    ALLOC(nodes, 2 * C.rows);
    C.leaves = leaves;
    C.nodes = nodes;
    CK(ensure_ws(ctx, commit_scratch_fes(ctx, C.rows, C.width) * 32));
    const uint64_t* ptrs[4];
    for (unsigned b = 0; b < batch; b++) ptrs[b] = U(polys[b]);
    return commit_into(ctx, ptrs, batch, n_vars, log_inv_rate, fold, U(leaves), U(nodes), (uint64_t*)ctx->d_ws, &C.layout);
}
// ... and the half that talks: root, OOD points and answers, batching randomness (mtUtilities.go:51-76)
int whir_commit_transcript(pk_ctx* ctx, const pk_whir_config& cfg, const fe& root, Transcript& T, Commitment& C) {
    const unsigned batch = C.batch;
    T.add_canon(root);
    C.ood_points.resize(cfg.commitment_ood_samples);
    T.challenge_scalars(C.ood_points.data(), C.ood_points.size());
    C.ood_answers.resize((size_t)batch * C.ood_points.size());
    for (size_t j = 0; j < C.ood_points.size(); j++) {
        // the polynomials of a batch are evaluated at the same point: two per launch (and per host round trip)
        for (unsigned b = 0; b < batch; b += 2) {
            const unsigned np = batch - b >= 2 ? 2 : 1;
            fe ans[2];
            CK(commitment_evaluate(ctx, C, b, np, C.ood_points[j], ans));
            for (unsigned q = 0; q < np; q++) C.ood_answers[(b + q) * C.ood_points.size() + j] = ans[q];
        }
    }
    for (unsigned b = 0; b < batch; b++) T.add_scalars(&C.ood_answers[b * C.ood_points.size()], C.ood_points.size());
    C.beta = batch > 1 ? T.challenge_scalar() : fe_one();  // whir draws the batching randomness only for a real batch
    return PK_OK;
}

// whir::Prover::prove opens a batch of two at the linear weights of a statement (struct Weights).
// On a device set (and a polynomial long enough) the sumcheck tables, the weights and the OOD evaluations are split into the
// ranks' blocks.
bool whir_sharded(const pk_ctx* ctx, unsigned n_vars) {
    const size_t G = (size_t)comm_world(ctx);
    return G > 1 && (((size_t)1 << n_vars) / G) >= 2 * SHARD_MIN_LOCAL;
}
// how many of a weight's `stored` leading entries lie inside the block [off, off + len)
size_t in_block(size_t stored, size_t off, size_t len) {
    const size_t hi = stored < off + len ? stored : off + len;
    return hi > off ? hi - off : 0;
}
// The linear weights of a statement, stated once: `n` evaluation tables over the hypercube of which only the first len[i] entries are
// stored -- the rest is zero by construction (create_combined_statement_over_two_polynomials zero-extends each row,
// whir_r1cs.rs:382-412), so nothing is spent on the zero half.  The rows stand on the device -- of a sharded opening only the entries
// inside this rank's block need to be present -- or, the one row of a statement over a host commitment, in host memory.
struct Weights {
    bool host;
    unsigned n;
    const fe* row[3];
    size_t len[3];
    const fe* sums;  // sums[i * 2 + b] = <weight i, polynomial b>, as the transcript holds them (may be null: the first round then forms three sums)
    // three device rows at equal stride and of one length: one pass serves all three (the statement weights into w0, the deferred hint)
    const bool equal_stride3 = n == 3 && len[0] == len[1] && len[1] == len[2] && row[1] > row[0] && row[1] - row[0] == row[2] - row[1];
    size_t stride() const { return equal_stride3 ? (size_t)(row[1] - row[0]) : 0; }
};

// ------------------------------------------------------------------ the round loop of the prover's sumchecks
// `rounds` rounds, each: the round's sums, the message, absorb, squeeze the folding challenge, record it.  The Spartan cubic rounds
// (ZkRounds) and the WHIR quadratic rounds (WhirProver) bring, as `s`, only what differs between them:
//   launch(t, fold, gate_seq, &red_seq), nsums(t)  enqueue round t's kernel, which first folds by `fold` or by the gate's challenge (round 0: neither); its sums
//   closing_fold(), fold(r, gate_seq)              whether the last challenge is applied by a fold of its own, and that fold
//   meanwhile(t)                                   host work of round t that needs the earlier challenges only
//   before_sync_launch(), sharded                  synchronous rounds: what precedes the launch; whether the sums are sums over the ranks
//   message(t, out, msg), record(t, msg, r)        the kernel's sums -> the message msg[0 .. return value); round t's challenge r is known
// Latency mode (pipelined): what consumes round t's challenge -- round t+1, or after the last round the closing fold -- is enqueued
// BEFORE round t's result is read, gated on the challenge the host publishes once it has squeezed it, and meanwhile() runs under that
// kernel; the round trip then costs the link, not a launch + sync.  A gated kernel waits on the host: PendingGate releases it on
// whatever path leaves the round.  Otherwise every round is a synchronous call that first folds by the previous challenge.
// The host tail (pk_selftest_set_host_tail, host_tail.hpp): once what comes next -- a round, or the closing fold -- would read tables of s.len
// entries or fewer than the context's threshold, s.to_host(t) brings them over as they stand (one launch, one synchronisation) and from
// there on the loop is the host's: host_round(t, fold) applies the pending fold by the previous challenge ON THE HOST, after the copy,
// then sums; host_fold closes.  In latency mode the round at the boundary is not enqueued behind a gate.  Only a sumcheck whose
// host_capable() holds: not sharded.
template <class S>
int sumcheck_round_loop(pk_ctx* ctx, Transcript& T, unsigned rounds, bool pipelined, S& s) {
    unsigned red_cur = 0, red_next = 0;
    uint64_t f[4];  // the previous round's challenge
    auto host_next = [&] { return s.on_host() || (s.host_capable() && host_tail_takes(ctx, s.sharded, s.len)); };
    bool queued = false;  // latency mode: this round's kernel is in the queue already ...
    bool closed = false;  // ... and so is the closing fold
    if (pipelined && !host_next()) {
        CK(s.launch(0, nullptr, 0, &red_cur));
        queued = true;
    }
    for (unsigned t = 0; t < rounds; t++) {
        PendingGate gate(ctx);
        const bool more = t + 1 < rounds;
        bool queued_next = false;
        uint64_t out[12];
        if (!queued && host_next()) {  // the tables only shrink: once true, true for the rest of the loop
            CK(s.to_host(t));
            s.meanwhile(t);
            s.host_round(t, t ? f : nullptr, out);
        } else if (pipelined) {
            if ((more || s.closing_fold()) && !host_next()) {
                gate.arm(sumcheck_gate_next(ctx));
                CK(more ? s.launch(t + 1, nullptr, gate.seq, &red_next) : s.fold(nullptr, gate.seq));
                (more ? queued_next : closed) = true;
            }
            s.meanwhile(t);
            CK(sumcheck_collect_spin(ctx, s.nsums(t), red_cur, out));
            red_cur = red_next;
        } else {
            s.meanwhile(t);
            CK(s.before_sync_launch());
            Across ac(ctx, s.sharded);
            CK(ac.rc);
            unsigned seq = 0;
            CK(s.launch(t, t ? f : nullptr, 0, &seq));
            CK(sumcheck_collect(ctx, s.nsums(t), out));
        }
        fe msg[4];
        const unsigned n = s.message(t, out, msg);
        T.add_scalars(msg, n);
        const fe r = T.challenge_scalar();
        gate.publish(r);
        h_store(f, r);
        s.record(t, msg, r);
        queued = queued_next;
    }
    if (rounds && !closed && s.closing_fold()) {
        if (host_next()) {
            CK(s.to_host(rounds));
            s.host_fold(f);
        } else {
            CK(s.fold(f, 0));
        }
    }
    return PK_OK;
}

// The working polynomial of an opening, c = sum_b beta^b poly_b (mtUtilities.go:98-114), in coefficient form and whole on every rank: what
// each round folds, re-commits and evaluates.  It lives where the commitment opened lives: in the arena, or -- a host commitment -- in host
// memory, where its folds, re-commitments and evaluations are host_whir.hpp's and nothing of the arena is taken.  The bodies below hold
// the only tests of which.
struct WorkingPoly {
    pk_ctx* ctx;
    Arena& A;
    const bool host;
    unsigned nv;
    fe* d = nullptr;     // device
    std::vector<fe> h;   // host

    // fold the coefficient form by the k challenges rs
    int fold(const std::vector<fe>& rs, unsigned k) {
        const unsigned nv2 = nv - k;
        if (host) {
            std::vector<fe> h2((size_t)1 << nv2);
            host_whir::fold_coeffs(h.data(), nv, rs.data(), k, h2.data());
            h.swap(h2);
        } else {
            ALLOC(d2, (size_t)1 << nv2);
            CK(pk_fold_coeffs(ctx, U(d), nv, (const uint64_t*)rs.data(), k, U(d2)));
            d = d2;
        }
        nv = nv2;
        return PK_OK;
    }
    // commit to it alone (N1+N2+M1+M2): the tree of the next round
    int commit(unsigned log_inv_rate, unsigned fold, Commitment& next) {
        fe* poly = host ? h.data() : d;
        return whir_commit_compute(ctx, A, host, nv, log_inv_rate, fold, &poly, 1, next);
    }
    int evaluate(const fe& z, fe& out) {
        if (!host) return eval_univariate_multi_x(ctx, &d, 1, (size_t)1 << nv, z, &out);
        out = host_whir::horner(h.data(), (size_t)1 << nv, z);
        return PK_OK;
    }
    // the coefficients in the clear, for the transcript: the last use of the polynomial
    int to_host(std::vector<fe>& out) {
        if (host) {
            out = std::move(h);
            return PK_OK;
        }
        out.resize((size_t)1 << nv);
        return pk_memcpy_d2h(ctx, out.data(), d, 32 * out.size());
    }
};

struct WhirProver {
    pk_ctx* ctx;
    Arena& A;
    const pk_whir_config& cfg;
    const Commitment& C;
    Transcript& T;
    const unsigned n, k, G, lgG, rank;
    bool sharded;          // the sumcheck tables are this rank's block [off0, off0 + B0) of the hypercube
    const size_t B0, off0;
    WorkingPoly c;
    fe* bp[2] = {};        // sumcheck operands: p = evaluations of c over the hypercube, w = combined weights; ping-pong halves
    fe* bw[2] = {};
    fe* gathered[4] = {};  // sharded: where p, w go once the blocks are short (p0, p1, w0, w1)
    // the host tail: once p and w are short they live here (p, then w, in one buffer), folded in place, for the rest of the opening -- the
    // rounds, the closing folds and the equality weights of the later rounds.  The opening of a host commitment starts here.
    bool host = false;
    std::vector<fe> htab;
    fe *hp = nullptr, *hw = nullptr;
    int cur = 0;
    size_t len;             // local length of p and w
    std::vector<fe> rs;     // the challenges of the last sumcheck_rounds call
    fe claim;               // <p, w>, the sum the next sumcheck round's h(0) + h(1) must equal -- while have_claim
    bool have_claim = false;
    std::vector<fe> all_r;  // every folding challenge, in squeeze order

    WhirProver(pk_ctx* c, Arena& a, const pk_whir_config& cf, const Commitment& com, Transcript& t)
        : ctx(c), A(a), cfg(cf), C(com), T(t), n(cf.n_vars), k(cf.folding_factor), G((unsigned)comm_world(c)), lgG(ilog2(G)),
          rank((unsigned)comm_rank(c)), sharded(whir_sharded(c, n)), B0(sharded ? ((size_t)1 << n) / G : (size_t)1 << n),
          off0(sharded ? (size_t)rank * B0 : 0), c{ctx, A, com.host, cf.n_vars}, len(B0) {}

    // equality weights of the univariate points zs (expand_from_univariate; variable 0 <-> the top index bit), scaled by 1, gamma,
    // gamma^2, ... and accumulated into the weight table w.  The whole table, or -- sharded -- this rank's block, whose top lgG index bits
    // are the rank: that factor of eq goes into the scale and the table is built over the rest.  defer: the accumulation is left to
    // round 0's own launch (launch(0), mle.hip opening_first_launch), which needs w's pairs anyway
    int eq_weights(unsigned nv, const std::vector<fe>& zs, const fe& gamma, int overwrite, bool defer) {
        const size_t q = zs.size();
        const unsigned lg = sharded ? lgG : 0, nl = nv - lg;
        std::vector<fe> x(nv ? nv : 1);
        std::vector<fe>& pts = first.pts;  // they outlive this call when the launch is deferred
        std::vector<fe>& scales = first.scales;
        pts.assign(q * (nl ? nl : 1), fe_zero());
        scales.assign(q ? q : 1, fe_zero());
        fe g = fe_one();
        for (size_t j = 0; j < q; j++) {
            expand_from_univariate(zs[j], nv, x.data());
            scales[j] = lg ? h_mul(g, eq_bits(x.data(), lg, rank)) : g;
            std::copy(x.begin() + lg, x.begin() + nv, pts.begin() + j * nl);
            g = h_mul(g, gamma);
        }
        if (host) {  // never a rank's block: lg = 0
            host_tail::eq_accumulate(hw, nv, pts.data(), scales.data(), q, overwrite != 0);
            return PK_OK;
        }
        if (!defer) return pk_eq_accumulate(ctx, U(bw[cur]), nl, (const uint64_t*)pts.data(), (const uint64_t*)scales.data(), (unsigned)q, overwrite);
        first.a = opening_first{};
        first.a.d_w = U(bw[cur]);
        first.a.n = (size_t)1 << nl;
        first.a.points = (const uint64_t*)pts.data();
        first.a.scales = (const uint64_t*)scales.data();
        first.a.q = (unsigned)q;
        first.a.overwrite = overwrite;
        first.pending = true;
        return PK_OK;
    }
    // Round 0's tables while they are still to be formed: the equality weights (eq_weights, deferred) and, in the opening's first launch,
    // the batch combination and the statement rows (start).  launch(0) forms them in the round's own kernel.
    struct First {
        bool pending = false;
        opening_first a{};
        std::vector<fe> pts, scales;
        uint64_t beta[4], row_scales[12];
    } first;

    void flip() {
        cur = 1 - cur;
        len /= 2;
    }

    // `rounds` quadratic sumcheck rounds on p, w (sumcheck_round_loop), each: the round's h(0), h(1), h(2), absorb, squeeze the folding
    // challenge, record it; afterwards p, w describe the folded polynomial.  A round whose claim h(0) + h(1) the prover holds -- every
    // round but the first after new weights went into w: the claim is the previous round's h(r), and before the first call the
    // statement's own sum (start) -- asks its kernel for h(0) and h(2) only and takes h(1) = claim - h(0).  Latency mode: one GPU.
    // Sharded, the sums of a round are sums over the ranks' blocks.
    int sumcheck_rounds(unsigned rounds) {
        rs.clear();
        ns0 = have_claim ? 2 : 3;
        const bool pipelined = ctx->latency_mode && G == 1 && rounds && len >= ((size_t)1 << rounds);
        return sumcheck_round_loop(ctx, T, rounds, pipelined, *this);
    }
    // what sumcheck_round_loop asks of its sumcheck
    int ns0 = 3;  // sums of round 0; the later rounds always have their claim
    int nsums(unsigned t) const { return t ? 2 : ns0; }
    int launch(unsigned t, const uint64_t* fold, unsigned gate_seq, unsigned* red_seq) {  // round 0 folds nothing; it writes what is pending
        if (first.pending) {  // only ever ahead of a round 0
            first.pending = false;
            first.a.d_p = U(bp[cur]);
            first.a.nsums = nsums(t);
            return opening_first_launch(ctx, first.a, 0, red_seq);
        }
        CK(sumcheck_quadratic_launch(ctx, U(bp[cur]), U(bw[cur]), len, fold, gate_seq, U(bp[1 - cur]), U(bw[1 - cur]), nsums(t), red_seq));
        if (fold || gate_seq) flip();
        return PK_OK;
    }
    bool closing_fold() const { return len >= 2; }  // applies the last challenge: p, w then describe the folded polynomial
    int fold(const uint64_t* r, unsigned gate_seq) {
        CK(fold_pairs2(ctx, U(bp[cur]), U(bp[1 - cur]), U(bw[cur]), U(bw[1 - cur]), len, r, gate_seq));
        flip();
        return PK_OK;
    }
    // the host tail: p and w as they stand -- a pending fold is applied on the host, by host_round -- and from then on for good
    bool on_host() const { return host; }
    bool host_capable() const { return !sharded; }
    int to_host(unsigned) {
        if (host) return PK_OK;
        if (first.pending) return set_err(ctx, PK_ERR_HIP, "host tail: a round's weights are still to be formed on the device");
        host_tables(len);
        const uint64_t* src[2] = {U(bp[cur]), U(bw[cur])};
        const size_t cnt[2] = {len, len};
        return tables_to_host(ctx, src, cnt, 2, U(htab.data()));  // the two runs back to back: p, then w
    }
    void host_tables(size_t entries) {
        htab.resize(2 * entries);
        hp = htab.data();
        hw = hp + entries;
        host = true;
    }
    void host_round(unsigned t, const uint64_t* fold, uint64_t out[12]) {
        const fe r = fold ? h_load(fold) : fe_zero();
        len = host_tail::quadratic_round(hp, hw, len, fold ? &r : nullptr, nsums(t), out);
    }
    void host_fold(const uint64_t* r) {
        const fe rr = h_load(r);
        host_tail::fold_pairs(hp, len, rr);
        host_tail::fold_pairs(hw, len, rr);
        len /= 2;
    }
    int before_sync_launch() { return PK_OK; }
    void meanwhile(unsigned) {}
    unsigned message(unsigned t, uint64_t out[12], fe msg[4]) {
        if (nsums(t) == 2) {
            uint64_t cl[4];
            h_store(cl, claim);
            sumcheck_quadratic_from_claim(cl, out);
        }
        for (int q = 0; q < 3; q++) msg[q] = h_load(out + 4 * q);
        return 3;
    }
    void record(unsigned, const fe* msg, const fe& r) {
        rs.push_back(r);
        all_r.push_back(r);
        claim = eval_quadratic_012(msg, r);  // the next round's h(0) + h(1)
        have_claim = true;
    }

    // all-gather of the ranks' blocks of p and w into (p0, w0) -- block r of the gather IS index range r -- after which the rest of
    // the sumcheck runs replicated
    int gather(fe* p0, fe* p1, fe* w0, fe* w1) {
        CK(gather_blocks(ctx, bp[cur], len, p0));
        CK(gather_blocks(ctx, bw[cur], len, w0));
        bp[0] = p0; bp[1] = p1; bw[0] = w0; bw[1] = w1;
        cur = 0;
        len *= G;
        sharded = false;
        return PK_OK;
    }
    // once a rank's block is short; a sumcheck_rounds call shrinks the block 2^k-fold, so blocks never run out inside one
    int maybe_gather() { return sharded && len <= SHARD_MIN_LOCAL ? gather(gathered[0], gathered[1], gathered[2], gathered[3]) : PK_OK; }

    // How the opening starts: where c, p0 and w0 are formed.  Chosen once, by start().
    enum class Route {
        Host,         // a host commitment: c, p0, w0 on the host; nothing of the arena
        FirstLaunch,  // mle.hip opening_first_launch: p0, w0 and round 0's sums from one pass over the two evaluation tables and the statement rows
        Plain         // everything else on the device: a rank's block, tables the host tail takes at once, rows the first launch does not take
    };

    // the working polynomial, the sumcheck tables, the initial weights and the first k sumcheck rounds
    int start(const Weights& W) {
        // pk_prove opens what commit_batch made, and a host commitment at a host weight: general batches are libprovekit_whir's (whir_pcs/pcs.cpp)
        PK_REQUIRE(ctx, C.batch == 2 && C.evals[0] && C.evals[1] && W.host == C.host && !(C.host && (sharded || W.n != 1 || W.len[0] > ((size_t)1 << n))),
                   "an opening of pk_prove: a batch of two with both evaluation tables, its weights where the commitment is");
        // (tables that round 0 takes to the host at once are formed by the plain sequence: the first launch would leave them pending)
        const bool first_launch = !host_tail_takes(ctx, sharded, B0) && !sharded && B0 >= 2 && k >= 1 && (W.equal_stride3 || W.n == 1) && W.len[0] <= B0;
        const Route route = C.host ? Route::Host : first_launch ? Route::FirstLaunch : Route::Plain;
        // initial combination randomness; weights = sum gamma^i w_i over [OOD constraints..., statement weights...]
        const fe gamma = T.challenge_scalar();
        // <p, w> of the tables about to be built, from values the transcript holds: an OOD constraint's sum is its answer, a statement weight's its claimed sum
        auto batched = [&](const fe* v, size_t step) { return h_add(v[0], h_mul(C.beta, v[step])); };  // sum_b beta^b v[b * step]
        const size_t q = C.ood_points.size();
        claim = fe_zero();
        fe g = fe_one();
        for (size_t j = 0; j < q; j++, g = h_mul(g, gamma)) claim = h_add(claim, h_mul(g, batched(&C.ood_answers[j], q)));
        fe scale[3];  // of the statement rows: the powers of gamma that follow the OOD constraints'
        for (unsigned i = 0; i < W.n; i++, g = h_mul(g, gamma)) {
            scale[i] = g;
            if (W.sums) claim = h_add(claim, h_mul(g, batched(W.sums + 2 * (size_t)i, 1)));
        }
        have_claim = W.sums || !W.n;
        switch (route) {
            case Route::Host: CK(start_host(W, gamma, scale)); break;
            case Route::FirstLaunch: CK(start_first_launch(W, gamma, scale)); break;
            case Route::Plain: CK(start_plain(W, gamma, scale)); break;
        }
        if (sharded) {
            const size_t cap = G * SHARD_MIN_LOCAL;
            const size_t sizes[4] = {cap, cap / 2, cap, cap / 2};
            for (int q = 0; q < 4; q++) {
                ALLOC(buf, sizes[q]);
                gathered[q] = buf;
            }
        }
        CK(sumcheck_rounds(k));
        return maybe_gather();
    }
    int start_host(const Weights& W, const fe& gamma, const fe* scale) {
        const size_t N = (size_t)1 << n;
        host_tables(N);
        host_tail::lincomb2(hp, C.evals[0], C.beta, C.evals[1], N);
        c.h.resize(N);
        host_tail::lincomb2(c.h.data(), C.polys[0], C.beta, C.polys[1], N);
        CK(eq_weights(n, C.ood_points, gamma, /*overwrite=*/1, /*defer=*/false));
        host_tail::axpy(hw, scale[0], W.row[0], W.len[0]);
        return PK_OK;
    }
    int device_tables() {  // of both device routes: c, and the ping-pong halves of p and w
        ALLOC(dc, (size_t)1 << n);
        ALLOC(p0, B0);
        ALLOC(p1, B0 / 2 ? B0 / 2 : 1);
        ALLOC(w0, B0);
        ALLOC(w1, B0 / 2 ? B0 / 2 : 1);
        c.d = dc;
        bp[0] = p0; bp[1] = p1; bw[0] = w0; bw[1] = w1;
        return PK_OK;
    }
    int start_first_launch(const Weights& W, const fe& gamma, const fe* scale) {
        CK(device_tables());
        h_store(first.beta, C.beta);
        CK(lincomb2(ctx, U(c.d), U(C.polys[0]), first.beta, U(C.polys[1]), (size_t)1 << n));  // the working polynomial alone: p0 comes from the first launch
        CK(eq_weights(n, C.ood_points, gamma, /*overwrite=*/1, /*defer=*/true));
        for (unsigned i = 0; i < W.n; i++) h_store(first.row_scales + 4 * i, scale[i]);  // the rows join w0 where round 0 first reads it
        first.a.d_e0 = U(C.evals[0]);
        first.a.d_e1 = U(C.evals[1]);
        first.a.beta = first.beta;
        first.a.d_rows = U(W.row[0]);
        first.a.row_stride = W.stride();
        first.a.nrows = W.n;
        first.a.row_len = W.len[0];
        first.a.row_scales = first.row_scales;
        return PK_OK;
    }
    int start_plain(const Weights& W, const fe& gamma, const fe* scale) {
        CK(device_tables());
        uint64_t beta[4], s[12];
        h_store(beta, C.beta);  // the coefficient and the evaluation combination of a batch of two in one launch
        CK(lincomb2_pair(ctx, U(c.d), U(C.polys[0]), U(C.polys[1]), (size_t)1 << n, U(bp[0]), U(C.evals[0] + off0), U(C.evals[1] + off0), B0, beta));
        CK(eq_weights(n, C.ood_points, gamma, /*overwrite=*/1, /*defer=*/false));
        for (unsigned i = 0; i < W.n; i++) h_store(s + 4 * i, scale[i]);
        if (W.equal_stride3) return axpy3(ctx, U(bw[0]), s, U(W.row[0] + off0), W.stride(), in_block(W.len[0], off0, B0));  // one read and one write of w0 instead of three
        for (unsigned i = 0; i < W.n; i++) {
            const size_t cnt = in_block(W.len[i], off0, B0);
            if (cnt) CK(pk_fe_axpy(ctx, U(bw[0]), s + 4 * i, U(W.row[i] + off0), cnt));
        }
        return PK_OK;
    }

    // W2: a round's new weights -- the equality weights of its OOD and STIR points, scaled by powers of the combination randomness -- join w.
    // Tables short enough for the host tail go there first, and the weights join w on the host.  Else, unless this is a rank's block, the
    // round's first sumcheck launch adds them.  At every number of points: the fused kernel runs at three waves per SIMD where
    // eq_accumulate_kernel has four, and the round of 110 points still came out ahead (EXPERIMENTS.md round 29)
    int round_weights(const std::vector<fe>& zs, const fe& gamma) {
        if (host_tail_takes(ctx, sharded, len)) CK(to_host(0));
        CK(eq_weights(c.nv, zs, gamma, /*overwrite=*/0, /*defer=*/!host && !sharded && len >= 2 && k >= 1));
        have_claim = false;  // the new weights' sums include the folded polynomial at the STIR points, which the prover never evaluates
        return PK_OK;
    }

    // the folding rounds: fold, re-commit, OOD, PoW, STIR openings of the previous tree, new weights, k sumcheck rounds (whir.go:51-220)
    int rounds() {
        const Commitment* prev = &C;  // the tree this round's STIR queries open
        Commitment com;
        unsigned log_inv_rate = cfg.starting_log_inv_rate;
        size_t domain_size = (size_t)1 << (n + log_inv_rate);
        fe exp_gen = folded_domain_generator(n + log_inv_rate, k);
        for (unsigned r = 0; r < cfg.n_rounds; r++) {
            // W1: fold the coefficient form by this round's randomness
            CK(c.fold(rs, k));
            log_inv_rate += k - 1;  // the domain halves while the polynomial shrinks 2^k-fold
            // N1+N2+M1+M2: re-commit
            Commitment next;
            fe root;
            CK(c.commit(log_inv_rate, k, next));
            CK(commitment_root(ctx, next, root));
            T.add_canon(root);
            // E1: OOD
            std::vector<fe> zs(cfg.ood_samples[r]);
            T.challenge_scalars(zs.data(), zs.size());
            std::vector<fe> ood_ans(zs.size());
            for (size_t j = 0; j < zs.size(); j++) CK(c.evaluate(zs[j], ood_ans[j]));
            T.add_scalars(ood_ans.data(), ood_ans.size());
            // P1
            CK(pow_round(ctx, T, cfg.pow_bits[r]));
            // Q1: STIR queries into the previous tree
            const std::vector<uint64_t> idx = stir_queries(T, domain_size, k, cfg.num_queries[r]);
            CK(emit_opening_hints(ctx, T, *prev, idx));
            // W2: equality weights of the OOD and STIR points
            const fe gamma = T.challenge_scalar();
            for (uint64_t i : idx) zs.push_back(h_pow(exp_gen, i));
            CK(round_weights(zs, gamma));
            // W3
            CK(sumcheck_rounds(k));
            CK(maybe_gather());
            com = std::move(next);
            prev = &com;
            domain_size /= 2;
            exp_gen = h_mul(exp_gen, exp_gen);
        }
        return final_round(*prev, domain_size);
    }

    // final round: the folded polynomial in the clear, PoW, final STIR openings, final sumcheck
    int final_round(const Commitment& prev, size_t domain_size) {
        if (sharded) {  // a schedule that ends before the blocks got short: finish replicated
            const size_t cap = len * G;
            ALLOC(fp0, cap);
            ALLOC(fp1, cap / 2 ? cap / 2 : 1);
            ALLOC(fw0, cap);
            ALLOC(fw1, cap / 2 ? cap / 2 : 1);
            CK(gather(fp0, fp1, fw0, fw1));
        }
        CK(c.fold(rs, k));
        std::vector<fe> fin;
        CK(c.to_host(fin));
        T.add_scalars(fin.data(), fin.size());
        CK(pow_round(ctx, T, cfg.final_pow_bits));
        const std::vector<uint64_t> idx = stir_queries(T, domain_size, k, cfg.final_queries);
        CK(emit_opening_hints(ctx, T, prev, idx));
        CK(sumcheck_rounds(c.nv));
        return pow_round(ctx, T, cfg.final_folding_pow_bits);  // whir.go:196-201
    }

    // deferred_weight_evaluations hint (common.go:63-73): each linear weight's MLE at the full folding point.
    // Round t folds index bit t (LSB first), so the point in eval_eq's MSB-first order is reverse(all_r).
    int deferred_hint(const Weights& W) {
        if (!W.n) return PK_OK;
        std::vector<fe> point(all_r.rbegin(), all_r.rend());
        const bool sh = whir_sharded(ctx, n);  // the eq table and the dot products by blocks, like the weights themselves
        std::vector<fe> evals(W.n);
        if (W.host) {
            uint64_t o[4] = {};
            host_tail::dot_rows_eq(W.row[0], 0, 1, point.data(), n, W.len[0], o);
            evals[0] = h_load(o);
        } else if (!sh && (W.equal_stride3 || W.n == 1)) {  // without the table: each lane forms its entries from the point's half tables
            uint64_t o[12] = {};
            CK(dot_rows_eq(ctx, U(W.row[0]), W.stride(), W.n, (const uint64_t*)point.data(), n, W.len[0], o));
            for (unsigned i = 0; i < W.n; i++) evals[i] = h_load(o + 4 * i);
        } else {
            ALLOC(d_eq, B0);
            if (sh) {
                const fe sc = eq_bits(point.data(), lgG, rank);
                CK(pk_eq_accumulate(ctx, U(d_eq), n - lgG, (const uint64_t*)(point.data() + lgG), (const uint64_t*)&sc, 1, 1));
            } else {
                CK(pk_eq_table(ctx, (const uint64_t*)point.data(), n, U(d_eq)));
            }
            Across ac(ctx, sh);
            CK(ac.rc);
            if (W.equal_stride3) {  // the three external rows against the eq table in one pass
                uint64_t o[12] = {};
                CK(dot_rows(ctx, U(W.row[0] + off0), W.stride(), 3, U(d_eq), nullptr, in_block(W.len[0], off0, B0), o));
                for (int i = 0; i < 3; i++) evals[i] = h_load(o + 4 * i);
            } else {
                for (unsigned i = 0; i < W.n; i++) {
                    uint64_t o[4] = {};
                    if (sh || W.len[i]) CK(pk_dot(ctx, U(W.row[i] + off0), U(d_eq), in_block(W.len[i], off0, B0), o));
                    evals[i] = h_load(o);
                }
            }
        }
        std::vector<uint8_t> buf;
        put_vec(buf, evals.data(), W.n);
        T.hint(buf.data(), buf.size());
        return PK_OK;
    }
};
int whir_prove(pk_ctx* ctx, Arena& A, const pk_whir_config& cfg, const Commitment& C, const Weights& W, Transcript& T) {
    WhirProver P(ctx, A, cfg, C, T);
    CK(P.start(W));
    CK(P.rounds());
    return P.deferred_hint(W);
}

// batch_commit_to_polynomial (provekit/prover/src/whir_r1cs.rs:182-209)
struct BatchCommit {
    Commitment com;
    fe* f_evals = nullptr;  // masked polynomial, evaluation form (2^m)
    fe* g_evals = nullptr;  // random polynomial, evaluation form (2^m)
    std::vector<fe> h_tables;  // a host commitment (com.host): f, g, then their coefficient forms, 2^m entries each, as they came over; f_evals .. point here
};
// masks, coefficient forms and the commitment's device work on `ctx`'s stream; nothing is read back and the transcript is not touched
int batch_commit_compute(pk_ctx* ctx, Arena& A, unsigned m, const pk_whir_config& cfg, const fe* d_evals, size_t n_evals, const RngKey& key,
                         u32 stream_mask, u32 stream_g, BatchCommit& out) {
    const size_t half = (size_t)1 << (m - 1), N = 2 * half;
    ALLOC(f, N);
    ALLOC(g, N);
    ALLOC(fe_, N);
    ALLOC(ge_, N);
    // f = [witness (zero padded) || mask]   (zk_utils.rs:3-22)
    // f, g hold the evaluation forms (kept for the weighted sums); the coefficient forms go to fe_, ge_
    if (comm_world(ctx) <= 1) {  // the tables are assembled inside the first to_coeffs sweep (mle.hip to_coeffs_generated)
        CK(to_coeffs_generated(ctx, m, U(d_evals), n_evals, key, stream_mask, stream_g, U(f), U(g), U(fe_), U(ge_)));
    } else {
        CK(pk_memset_zero(ctx, f, 32 * half));
        CK(pk_memcpy_d2d(ctx, f, d_evals, 32 * n_evals));
        {
            ProfScope prof(ctx, "random_fe");
            CK(random_fe(ctx, U(f + half), half, key, stream_mask));
            CK(random_fe(ctx, U(g), N, key, stream_g));
        }
        CK(pk_to_coeffs_into(ctx, U(f), U(fe_), m));
        CK(pk_to_coeffs_into(ctx, U(g), U(ge_), m));
    }
    out.f_evals = f;
    out.g_evals = g;
    fe* polys[2] = {fe_, ge_};
    int rc = whir_commit_compute(ctx, A, /*host=*/false, cfg.n_vars, cfg.starting_log_inv_rate, cfg.folding_factor, polys, 2, out.com);
    out.com.evals[0] = f;
    out.com.evals[1] = g;
    return rc;
}

// public inputs of the witness transcript: the ACIR witness values at the circuit's public indices
__global__ void gather_fe_kernel(const fe* __restrict__ src, const uint32_t* __restrict__ idx, size_t n, fe* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fe_store(dst + i, fe_load(src + idx[i]));
}

// One proof over a device set: a rank that leaves early (arena exhausted, a HIP error, an unsatisfied witness on this rank only)
// never reaches the collectives its peers are -- or will be -- waiting in.  Whatever the exit path, a failing rank aborts the
// group (in-process transport: the waiting ranks wake with PK_ERR_RCCL; host transport: this rank's communicator is marked
// failed; RCCL: this rank's OWN communicator is aborted -- its peers are rescued by their collective deadline, comm.hip comm_wait).
// One exception, RCCL only, where an abort is irreversible: a refusal that every rank of the set makes identically (a bad argument,
// an unsatisfied witness, an IO-pattern mismatch) BEFORE this call has enqueued any collective leaves the ranks in step, so the
// communicator stays usable for the next call.
struct AbortOnFailure {
    pk_ctx* c;
    unsigned long long issued0;
    int rc = PK_ERR_HIP;  // until done(): a path that leaves without reporting its status fails, and not the same on every rank
    explicit AbortOnFailure(pk_ctx* ctx) : c(ctx), issued0(comm_collectives_issued(ctx)) {}
    int done(int status) { return rc = status; }
    ~AbortOnFailure() {
        if (rc == PK_OK) return;
        struct Drain {  // whatever happens to the communicator, an abandoned proof leaves nothing behind on the stream: a gated kernel
            pk_ctx* c;  // released with a zero challenge must have finished -- and its give-up word be cleared -- before the next proof starts
            ~Drain() {
                (void)wait_ctx(c);
                sumcheck_gate_clear(c);
            }
        } drain{c};
        if (comm_world(c) <= 1) return;
        const bool same_everywhere = rc == PK_ERR_BAD_ARG || rc == PK_ERR_UNSATISFIED || rc == PK_ERR_IO_PATTERN;
        if (comm_rccl(c) && same_everywhere && comm_collectives_issued(c) == issued0) return;
        comm_abort(c);
    }
};

// latency mode, one GPU: the scheme's second context (a stream and workspace of its own on the same device, created on first use)
// runs the work that can overlap -- the blinding commitment underneath the witness commitment, the external rows underneath the
// blinding WHIR proof.  Whatever path leaves pk_prove, its stream must not still be working in this proof's arena: drained on every
// exit, its mailbox rewound.
struct SideContext {
    pk_ctx* c = nullptr;
    int open(pk_ctx* ctx, pk_scheme* s) {
        if (!s->side) {
            int dev = 0;
            PK_HIP(ctx, hipGetDevice(&dev));
            CK(pk_ctx_create(dev, &s->side));
        }
        c = s->side;
        c->hash_version = ctx->hash_version;
        return PK_OK;
    }
    ~SideContext() {
        if (!c) return;
        (void)wait_stream(c->device, c->stream);
        c->mail_off = 0;
    }
};

// one pk_prove call: the state its stages share
struct Proof {
    pk_ctx* ctx;
    pk_scheme* s;
    const fe* d_witness;
    size_t n_witness;
    const RngKey& key;
    Arena A;
    Transcript T;
    const unsigned G, lgG, rank;
    // sharded witness WHIR: a rank needs (and computes) only the columns of the external rows inside its block of the hypercube
    const bool st_sharded;
    const size_t blk, blk_lo;
    SideContext side;
    pk_ctx* aux;             // where the work that can overlap runs: the side context in latency mode on one GPU, else ctx
    BatchCommit W, B;        // the witness commitment, the blinding commitment
    std::vector<fe> g_univ;  // blinding univariates: 4 coefficients per variable
    fe* h_univ = nullptr;    // ... as the side stream copied them into its mailbox
    std::vector<fe> alpha;   // the zk sumcheck's challenges
    fe* rows = nullptr;      // the three external rows, n_witness each
    fe row_sums[6];          // their sums against f and g: [row][f, g]
    const bool timing = getenv("PK_PROVE_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t_lap = std::chrono::steady_clock::now();

    Proof(pk_ctx* c, pk_scheme* sc, const fe* w, size_t nw, const RngKey& k)
        : ctx(c), s(sc), d_witness(w), n_witness(nw), key(k), A{sc->arena, sc->arena_bytes}, T(sc->domain_separator), G((unsigned)comm_world(c)),
          lgG(ilog2(G)), rank((unsigned)comm_rank(c)), st_sharded(whir_sharded(c, sc->m)), blk(((size_t)1 << sc->m) / (st_sharded ? G : 1)),
          blk_lo(st_sharded ? (size_t)rank * blk : 0), aux(c), g_univ(4 * (size_t)sc->m_0) {}

    // where the blinding commitment runs, decided once by init(): what each means is told above commit_witness
    enum class BlindingAt { HostThread, SideStream, Inline } blinding_at = BlindingAt::Inline;

    int init() {
        if (ctx->latency_mode && G == 1) {
            CK(side.open(ctx, s));
            aux = side.c;
        }
        blinding_at = host_tail_takes(ctx, false, (size_t)2 << s->nb) ? BlindingAt::HostThread : aux != ctx ? BlindingAt::SideStream : BlindingAt::Inline;
        return PK_OK;
    }
    // the external rows go to the side context too, unless there are none
    pk_ctx* rows_ctx() const { return n_witness ? aux : ctx; }
    // a failure on the side context is reported where the caller looks
    int relay(pk_ctx* c, int rc, const char* what) {
        if (!rc || c == ctx) return rc;
        return set_err(ctx, rc, "%s on the side stream: %s", what, pk_last_error(c));
    }
    void lap(const char* what) {  // PK_PROVE_TIMING: one stderr line per stage
        if (!timing) return;
        (void)wait_ctx(ctx);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[pk_prove] %-28s %8.3f ms (sponge: %u permutes, %.3f ms; hint serialisation so far %.3f ms)\n", what,
                1e3 * std::chrono::duration<double>(t - t_lap).count(), T.permutes(), 1e3 * T.permute_seconds, 1e3 * T.hint_seconds);
        t_lap = t;
    }

    int commit_witness();
    int blinding_transcript();
    int zk_sumcheck();
    int zk_rounds(fe* z[4], size_t len, bool sharded, const fe* r);
    int prove_blinding();
    int witness_statement();
    int prove_witness();
};

// blinding univariates: 4 random coefficients per variable [RNG], committed with the small WHIR (whir_r1cs.rs:212-226): the device
// work, on `ctx`'s stream.  On the side context the coefficients come back through its mailbox, else at once.
// First the draw, shared with the host route: 4 m_0 coefficients at the head of a zeroed table of 2^nb
int blinding_draw(pk_ctx* ctx, Proof& P, fe*& d_blind) {
    Arena& A = P.A;
    const size_t NB = (size_t)1 << P.s->nb;
    ALLOC(tab, NB);
    d_blind = tab;
    CK(pk_memset_zero(ctx, d_blind, 32 * NB));
    return random_fe(ctx, U(d_blind), P.g_univ.size(), P.key, RNG_BLIND);  // 4 m_0 <= 108: one workgroup
}
int blinding_compute(pk_ctx* ctx, Proof& P) {
    Arena& A = P.A;
    const size_t NB = (size_t)1 << P.s->nb, n = P.g_univ.size();
    fe* d_blind = nullptr;
    CK(blinding_draw(ctx, P, d_blind));
    if (P.blinding_at == Proof::BlindingAt::Inline) {
        CK(pk_memcpy_d2h(ctx, P.g_univ.data(), d_blind, 32 * n));
    } else {
        CK(mail_alloc(ctx, 32 * n, (void**)&P.h_univ));
        PK_HIP(ctx, hipMemcpyAsync(P.h_univ, d_blind, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    }
    return batch_commit_compute(ctx, A, P.s->nb + 1, P.s->whir_hiding, d_blind, NB, P.key, RNG_MASK_B, RNG_G_B, P.B);
}

// The host route (BlindingAt::HostThread), first half: the blinding coefficients, the two tables and their coefficient forms are drawn
// and formed on the device as blinding_compute does -- three small launches -- and come over in ONE transfer, f | g | their coefficient
// forms, 2^(nb+1) entries each (tables_to_host: one launch, one synchronisation).  Nothing of the blinding polynomial is on the device
// afterwards.  Called before the witness commitment is enqueued, so that its wait is for these launches alone.
int blinding_tables_to_host(pk_ctx* ctx, Proof& P) {
    Arena& A = P.A;
    const unsigned mb = P.s->nb + 1;
    const size_t NB = (size_t)1 << P.s->nb, N = 2 * NB, n = P.g_univ.size();
    fe* d_blind = nullptr;
    CK(blinding_draw(ctx, P, d_blind));
    ALLOC(f, N);
    ALLOC(g, N);
    ALLOC(fc, N);
    ALLOC(gc, N);
    CK(to_coeffs_generated(ctx, mb, U(d_blind), NB, P.key, RNG_MASK_B, RNG_G_B, U(f), U(g), U(fc), U(gc)));
    P.B.h_tables.resize(4 * N);
    const uint64_t* src[4] = {U(f), U(g), U(fc), U(gc)};
    const size_t cnt[4] = {N, N, N, N};
    CK(tables_to_host(ctx, src, cnt, 4, U(P.B.h_tables.data())));
    std::copy(P.B.h_tables.begin(), P.B.h_tables.begin() + n, P.g_univ.begin());  // f's head is the blinding polynomial
    return PK_OK;
}
// ... second half: the commitment of the tables that came over, on the host thread (host_whir.hpp)
int blinding_commit_host(pk_ctx* ctx, Proof& P) {
    BatchCommit& out = P.B;
    const pk_whir_config& cfg = P.s->whir_hiding;
    const size_t N = (size_t)2 << P.s->nb;
    fe *f = out.h_tables.data(), *g = f + N;
    out.f_evals = f;
    out.g_evals = g;
    fe* polys[2] = {g + N, g + 2 * N};
    out.com.evals[0] = f;
    out.com.evals[1] = g;
    return whir_commit_compute(ctx, P.A, /*host=*/true, cfg.n_vars, cfg.starting_log_inv_rate, cfg.folding_factor, polys, 2, out.com);
}

// external rows (whir_r1cs.rs:81-91, 382-412): eq(alpha) and the three rows [S4] on `ctx`'s stream.  On the side context the six
// weighted sums follow at once, deferred: their results are read after its next synchronisation.
int external_rows(pk_ctx* ctx, Proof& P) {
    Arena& A = P.A;
    const size_t nw = P.n_witness;
    ALLOC(d_eq_alpha, (size_t)1 << P.s->m_0);
    ALLOC(rows, 3 * (nw ? nw : 1));
    P.rows = rows;
    CK(pk_eq_table(ctx, (const uint64_t*)P.alpha.data(), P.s->m_0, U(d_eq_alpha)));
    if (P.st_sharded) CK(external_row_range(ctx, P.s->r1cs, U(d_eq_alpha), P.blk_lo, std::min(nw, P.blk_lo + P.blk), U(rows)));  // this rank's columns
    else CK(pk_r1cs_external_row(ctx, P.s->r1cs, U(d_eq_alpha), U(rows)));
    if (ctx == P.ctx) return PK_OK;
    return dot_rows(ctx, U(rows), nw, 3, U(P.W.f_evals), U(P.W.g_evals), nw, nullptr, /*defer=*/true);
}

// --- commit to the masked witness polynomial (whir_r1cs.rs:57-69), and -- underneath it -- to the blinding polynomial, which depends on
// nothing but the proof's key.  The witness commitment's launches fill the chip for 2.6 ms (several times that under load), and this
// thread would only wait for its root.  What runs where (Proof::blinding_at):
//   HostThread: the blinding tables (2^(nb+1) entries) go to the host tail -- every size pk_prove is used at.  They are drawn on the
//     device FIRST and come over in one transfer (blinding_tables_to_host); then, between the witness commitment's launches and read_root,
//     the 32-leaf codeword, its leaf hashes (chains of 31 compressions, ~0.7 ms of host time) and the tree are computed HERE, on this
//     thread, in either mode, and so is the whole blinding WHIR later (host_whir.hpp);
//   otherwise (threshold 0, a device set, a larger blinding polynomial) it is device work, 0.6 ms of launches that keep 32 lanes busy:
//     SideStream, in latency mode, right after the witness commitment's launches, underneath them; Inline, in plain mode, on the
//     prover's own stream, from zk_sumcheck.
// Only the blinding commitment's transcript half (root, OOD, batching) waits for its turn (blinding_transcript).
int Proof::commit_witness() {
    if (blinding_at == BlindingAt::HostThread) CK(blinding_tables_to_host(ctx, *this));
    CK(batch_commit_compute(ctx, A, s->m, s->whir_witness, d_witness, n_witness, key, RNG_MASK, RNG_G, W));
    if (blinding_at == BlindingAt::HostThread) CK(blinding_commit_host(ctx, *this));
    if (blinding_at == BlindingAt::SideStream) CK(relay(aux, blinding_compute(aux, *this), "blinding commitment"));  // Inline: zk_sumcheck enqueues it
    fe root;
    CK(commitment_root(ctx, W.com, root));
    return whir_commit_transcript(ctx, s->whir_witness, root, T, W.com);
}

// the blinding commitment's transcript half.  Its root is read on the context that built the tree (on the side context that waits
// for its stream and rewinds its mailbox), then the coefficients are taken out of the mailbox before anything is allocated there.
int Proof::blinding_transcript() {
    fe root;
    CK(relay(aux, commitment_root(aux, B.com, root), "blinding commitment"));
    if (blinding_at == BlindingAt::SideStream) memcpy(g_univ.data(), h_univ, 32 * g_univ.size());
    return whir_commit_transcript(ctx, s->whir_hiding, root, T, B.com);
}

// zk sumcheck message (whir_r1cs.rs:280-345): the round polynomial c[0..3] of the blinded sum from the sumcheck's h(0), h(-1), h(inf)
// (`out`), the blinding polynomial's round coefficients gp, rho and the running claim `saved`
void zk_round_message(const uint64_t out[12], const fe gp[4], const fe& rho, const fe& saved, fe c[4]) {
    const fe half = h_half();
    c[0] = h_add(h_load(out), h_mul(rho, gp[0]));
    const fe g_m1 = h_sub(h_add(h_sub(gp[0], gp[1]), gp[2]), gp[3]);
    const fe at_m1 = h_add(h_load(out + 4), h_mul(rho, g_m1));
    c[2] = h_mul(half, h_sub(h_sub(h_sub(h_add(saved, at_m1), c[0]), c[0]), c[0]));
    c[3] = h_add(h_load(out + 8), h_mul(rho, gp[3]));
    c[1] = h_sub(h_sub(h_sub(h_sub(saved, c[0]), c[0]), c[3]), c[2]);
}

// --- run_zk_sumcheck_prover (whir_r1cs.rs:228-369): witness bounds, eq table, blinding commitment, m_0 cubic rounds
int Proof::zk_sumcheck() {
    const unsigned m_0 = s->m_0;
    std::vector<fe> r(m_0);
    T.challenge_scalars(r.data(), m_0);
    const size_t M0 = (size_t)1 << m_0;
    // On a device set the four sumcheck arrays are split by the LOW index bits: rank g holds the entries i = g (mod G) at local
    // index i / G (see "one proof over a device set" above).  eq(r, i) factors into eq over the high variables (the local
    // table) times eq(last lgG variables, bits of g), a scalar that goes in as the table's scale.
    const bool sharded = G > 1 && M0 / G >= 2 * SHARD_MIN_LOCAL;
    const size_t length = sharded ? M0 / G : M0;
    ALLOC(d_a, length);
    ALLOC(d_b, length);
    ALLOC(d_cc, length);
    ALLOC(d_eq, length);
    if (sharded) {
        CK(witness_bounds_strided(ctx, s->r1cs, U(d_witness), m_0, G, rank, U(d_a), U(d_b), U(d_cc)));  // S1, this rank's rows
        const fe sc = eq_bits(&r[m_0 - lgG], lgG, rank);
        CK(pk_eq_accumulate(ctx, U(d_eq), m_0 - lgG, (const uint64_t*)r.data(), (const uint64_t*)&sc, 1, 1));  // S2
    } else {
        CK(pk_r1cs_witness_bounds(ctx, s->r1cs, U(d_witness), m_0, U(d_a), U(d_b), U(d_cc)));  // S1
        CK(eq_suffix_tables(ctx, (const uint64_t*)r.data(), m_0, U(d_eq)));                  // S2: the levels E_i instead of the table (mle.hip)
    }
    if (blinding_at == BlindingAt::Inline) CK(blinding_compute(ctx, *this));  // else the side stream, or the host, finished it long ago
    CK(blinding_transcript());
    lap("bounds+eq+blinding commit");
    fe* z[4] = {d_a, d_b, d_cc, d_eq};
    return zk_rounds(z, length, sharded, sharded ? nullptr : r.data());
}

// The m_0 cubic rounds (the hot loop, whir_r1cs.rs:280-345), as sumcheck_round_loop runs them: no closing fold, three sums per round.
// Latency mode (one GPU): a round's blinding coefficients, which depend only on the earlier challenges, are computed while its
// kernel runs.  Sharded, a round's evaluations are sums over the ranks' shares; short shares are gathered and finish replicated.
// r != null (every proof that is not sharded): z[3] holds the suffix equality tables of r instead of the eq array, the kernels fold a, b,
// c only and return Q(0), Q(-1), Q_inf; the round's scalars P_t (1 - r_t), P_t (2 - 3 r_t), P_t (2 r_t - 1) are applied here.  A sharded
// proof (r == null) keeps the four-array kernels: its arrays are split by the LOW index bits, which a level E_t does not factor over.
struct ZkRounds {
    Proof& pf;
    pk_ctx* ctx;
    fe** z;
    size_t len;
    bool sharded;
    const fe* r;
    const size_t M;  // the tables' length at round 0: level E_t of z[3] starts at M - (M >> t)
    fe rho, saved;   // the blinding's weight; the running claim
    fe* zfull[4];    // sharded: where the gathered arrays go, and the gather's scratch
    fe* ztmp;
    fe gp[4];        // the blinding polynomial's coefficients of the round
    uint64_t P[4];   // P_t = prod_{k<t} eq(r_k, alpha_k)
    // the host tail, from round t0 on: a, b, c as they stood before round t0's fold, and the levels E_t0 .. of z[3], back to back
    bool host = false;
    unsigned t0 = 0;
    std::vector<fe> h;  // a | b | c (n0 entries each) | levels
    size_t n0 = 0;

    bool on_host() const { return host; }
    bool host_capable() const { return !sharded && r; }  // the Level form only
    int to_host(unsigned t) {
        if (host) return PK_OK;
        t0 = t;
        n0 = len;
        const size_t nlev = M >> t;  // levels t .. (M >> t) - 1 entries, and the buffer's last element
        const uint64_t* src[4] = {U(z[0]), U(z[1]), U(z[2]), U(z[3] + (M - nlev))};
        const size_t cnt[4] = {len, len, len, nlev};
        h.resize(3 * len + nlev);
        CK(tables_to_host(ctx, src, cnt, 4, U(h.data())));
        host = true;
        return PK_OK;
    }
    void host_round(unsigned t, const uint64_t* fold, uint64_t out[12]) {
        const fe f = fold ? h_load(fold) : fe_zero();
        const fe* E = h.data() + 3 * n0 + ((M >> t0) - (M >> t));  // level E_t
        len = host_tail::cubic_round(h.data(), h.data() + n0, h.data() + 2 * n0, E, len, fold ? &f : nullptr, out);
    }
    void host_fold(const uint64_t*) {}  // no closing fold

    int nsums(unsigned) const { return 3; }
    int launch(unsigned t, const uint64_t* fold, unsigned gate_seq, unsigned* red_seq) {  // in place; the level E_t or the eq array
        CK(sumcheck_cubic_launch(ctx, U(z[0]), U(z[1]), U(z[2]), r ? CubicWeight::Level : CubicWeight::EqArray, U(z[3] + (r ? M - (M >> t) : 0)), len, fold,
                                 gate_seq, red_seq));
        if (fold || gate_seq) len /= 2;
        return PK_OK;
    }
    bool closing_fold() const { return false; }
    int fold(const uint64_t*, unsigned) { return PK_OK; }
    void meanwhile(unsigned t) { blinding_coefficients_for_round(pf.g_univ, t, pf.alpha.data(), gp); }
    int before_sync_launch() {
        if (!sharded || len > SHARD_MIN_LOCAL) return PK_OK;
        for (int q = 0; q < 4; q++) {  // short shares: gather, re-interleave, finish replicated
            CK(gather_strided(ctx, z[q], len, ztmp, zfull[q]));
            z[q] = zfull[q];
        }
        len *= pf.G;
        sharded = false;
        return PK_OK;
    }
    unsigned message(unsigned t, uint64_t out[12], fe msg[4]) {
        if (r) sumcheck_spliteq_correct(P, U(r + t), out);
        zk_round_message(out, gp, rho, saved, msg);
        return 4;
    }
    void record(unsigned t, const fe* msg, const fe& a) {
        pf.alpha.push_back(a);
        if (r) {
            uint64_t aw[4];
            h_store(aw, a);
            sumcheck_spliteq_advance(P, U(r + t), aw);
        }
        saved = eval_cubic(msg, a);
    }
};
int Proof::zk_rounds(fe* z[4], size_t len, bool sharded, const fe* r) {
    const unsigned m_0 = s->m_0;
    // sum_over_hypercube (whir_r1cs.rs:172-180)
    fe gp[4];
    blinding_coefficients_for_round(g_univ, 0, nullptr, gp);
    const fe sum_g = h_add(eval_cubic(gp, fe_zero()), eval_cubic(gp, fe_one()));
    T.add_scalar(sum_g);
    const fe rho = T.challenge_scalar();
    ZkRounds R{*this, ctx, z, len, sharded, r, len, rho, h_mul(rho, sum_g), {}, nullptr, {}, {}};
    h_store(R.P, fe_one());
    if (sharded) {
        const size_t cap = G * SHARD_MIN_LOCAL;
        for (int q = 0; q < 4; q++) {
            ALLOC(zf, cap);
            R.zfull[q] = zf;
        }
        ALLOC(zt, cap);
        R.ztmp = zt;
    }
    alpha.reserve(m_0);
    return sumcheck_round_loop(ctx, T, m_0, ctx->latency_mode && G == 1 && m_0 >= 2, R);
}

// --- statement over the blinding commitment: weight = expand_powers(alpha) zero-extended (whir_r1cs.rs:347-366,371-380), and its
// WHIR proof.  Latency mode: the witness statement's external rows and its six weighted sums depend on alpha and nothing else, and
// the transcript wants them only AFTER this proof -- 0.4 ms of kernels that go to the side stream first and run underneath it.
int Proof::prove_blinding() {
    if (rows_ctx() != ctx) CK(relay(aux, external_rows(aux, *this), "external rows"));
    const size_t nbw = 4 * (size_t)s->m_0;  // the weight is zero beyond the 4 m_0 blinding coefficients
    std::vector<fe> wv(nbw);
    for (size_t i = 0; i < s->m_0; i++) {
        wv[4 * i] = fe_one();
        wv[4 * i + 1] = alpha[i];
        wv[4 * i + 2] = h_mul(alpha[i], alpha[i]);
        wv[4 * i + 3] = h_mul(wv[4 * i + 2], alpha[i]);
    }
    uint64_t fg[8];
    const fe* weight = wv.data();
    if (B.com.host) {  // the tables never left the host: the statement's two sums, the opening's tables and its deferred hint are formed from them and from wv there
        host_tail::dot2(wv.data(), B.f_evals, B.g_evals, nbw, fg);
    } else {
        ALLOC(d_bw, nbw);
        CK(pk_memcpy_h2d(ctx, d_bw, wv.data(), 32 * nbw));
        CK(pk_dot2(ctx, U(d_bw), U(B.f_evals), U(B.g_evals), nbw, fg));
        weight = d_bw;
    }
    const fe sums[2] = {h_load(fg), h_load(fg + 4)};
    T.add_scalars(sums, 2);
    const Weights wts{B.com.host, 1, {weight}, {nbw}, sums};
    return whir_prove(ctx, A, s->whir_hiding, B.com, wts, T);
}

// --- the statement over the witness commitment (whir_r1cs.rs:81-91): external rows, their six sums, the claimed_evaluations hint
int Proof::witness_statement() {
    pk_ctx* rc = rows_ctx();
    if (rc == ctx) CK(external_rows(ctx, *this));
    Across ac(ctx, st_sharded);
    CK(ac.rc);
    // the statement weights are the rows zero-extended to 2^m (whir_r1cs.rs:391-400): only their support is stored and summed;
    // the three rows share f and g, so all six sums come from one pass (S5)
    uint64_t o[24] = {};
    if (rc != ctx) {  // launched before the blinding WHIR proof: finished long ago
        CK(relay(rc, sync_stream(rc), "external rows"));
        memcpy(o, rc->h_pinned, 32 * 6);
    } else if (st_sharded || n_witness) {
        CK(dot_rows(ctx, U(rows + blk_lo), n_witness, 3, U(W.f_evals + blk_lo), U(W.g_evals + blk_lo), in_block(n_witness, blk_lo, blk), o));
    }
    // hint::<(Vec<F>, Vec<F>)>: the three sums against f, then the three against g
    fe fsum[3], gsum[3];
    for (int k = 0; k < 3; k++) {
        fsum[k] = row_sums[2 * k] = h_load(o + 8 * k);
        gsum[k] = row_sums[2 * k + 1] = h_load(o + 8 * k + 4);
    }
    std::vector<uint8_t> claimed;
    put_vec(claimed, fsum, 3);
    put_vec(claimed, gsum, 3);
    T.hint(claimed.data(), claimed.size());
    return PK_OK;
}

// --- WHIR weighted batch opening (whir_r1cs.rs:94-95)
int Proof::prove_witness() {
    const Weights wts{false, 3, {rows, rows + n_witness, rows + 2 * n_witness}, {n_witness, n_witness, n_witness}, row_sums};
    CK(whir_prove(ctx, A, s->whir_witness, W.com, wts, T));
    return pk_ctx_sync(ctx);
}

// WhirR1CSProver::prove (provekit/prover/src/whir_r1cs.rs:42-100): the proof string into `narg`
int prove(pk_ctx* ctx, pk_scheme* s, const uint64_t* d_witness, size_t n_witness, const uint8_t* rng_seed32, const size_t* len,
          std::vector<uint8_t>& narg) {
    PK_REQUIRE(ctx, s && d_witness && len, "null pointer");
    PK_REQUIRE(ctx, n_witness == s->num_witnesses, "Unexpected witness length for R1CS instance");  // whir_r1cs.rs:43-46
    RngKey key;
    CK(proof_key(ctx, rng_seed32, key));
    struct Turn {  // see comm.hip: a no-op outside the test-suite's one-GPU timing mode
        pk_ctx* c;
        explicit Turn(pk_ctx* ctx) : c(ctx) { comm_turn_begin(c); }
        ~Turn() { comm_turn_end(c); }
    } turn(ctx);
    Proof P(ctx, s, (const fe*)d_witness, n_witness, key);
    CK(P.init());
    (void)sumcheck_gate_check(ctx);  // a word left by an earlier, abandoned proof is not this proof's
    CK(P.commit_witness());
    P.lap("witness commit");
    CK(P.zk_sumcheck());
    P.lap("zk sumcheck rounds");
    CK(P.prove_blinding());
    P.lap("blinding WHIR proof");
    CK(P.witness_statement());
    P.lap("external rows + sums");
    CK(P.prove_witness());
    P.lap("witness WHIR proof");
    // latency mode: every gated kernel of this proof has completed by now; one that gave up on its challenge computed with zero
    CK(sumcheck_gate_check(ctx));
    // the proof performed exactly the operations its IO pattern declares (what spongefish enforces on the reference's side)
    if (!P.T.finished())
        return set_err(ctx, PK_ERR_IO_PATTERN, "%s", P.T.violation().empty() ? "the proof ended before its IO pattern did" : P.T.violation().c_str());
    narg = std::move(P.T.narg);
    return PK_OK;
}

}  // namespace

extern "C" {

int pk_scheme_destroy(pk_ctx* ctx, pk_scheme* s) {
    PK_ENTER(ctx);
    if (!s) return PK_OK;
    (void)wait_ctx(ctx);
    (void)hipFree(s->arena);
    (void)hipFree(s->noir_witness);
    if (s->side) (void)pk_ctx_destroy(s->side);
    delete s;
    return PK_OK;
}

int pk_scheme_create(pk_ctx* ctx, const pk_r1cs* r1cs, size_t num_constraints, size_t num_witnesses, unsigned m, unsigned m_0,
                     const pk_whir_config* whir_witness, const pk_whir_config* whir_for_hiding_spartan, pk_scheme** out) {
    if (!ctx || !out) return PK_ERR_BAD_ARG;
    PK_ENTER(ctx);
    *out = nullptr;
    PK_REQUIRE(ctx, r1cs && whir_witness && whir_for_hiding_spartan, "null pointer");
    PK_REQUIRE(ctx, m >= 1 && m <= 27 && m_0 >= 1 && m_0 <= 27, "scheme size out of range (1 <= m, m_0 <= 27)");
    // ensure!(...) of provekit/prover/src/whir_r1cs.rs:43-54
    PK_REQUIRE(ctx, num_witnesses <= ((size_t)1 << (m - 1)), "R1CS witness length exceeds scheme capacity");
    PK_REQUIRE(ctx, num_constraints <= ((size_t)1 << m_0), "R1CS constraints exceed scheme capacity");
    PK_REQUIRE(ctx, whir_witness->n_vars == m && whir_witness->batch_size == 2, "whir_witness config does not match m / batch 2");
    // pk_prove commits the blinding polynomial next to its mask exactly as the witness (whir_r1cs.rs:212-226): batch 2, nothing else
    PK_REQUIRE(ctx, whir_for_hiding_spartan->batch_size == 2, "whir_for_hiding_spartan must have batch_size 2");
    for (const pk_whir_config* c : {whir_witness, whir_for_hiding_spartan}) {
        const char* why = whir_config_error(c);
        PK_REQUIRE(ctx, !why, why);
    }
    const unsigned nb = blinding_log_len(m_0);
    PK_REQUIRE(ctx, whir_for_hiding_spartan->n_vars == nb + 1, "whir_for_hiding_spartan must have next_power_of_two(4*m_0)+1 variables");
    pk_scheme* s = new (std::nothrow) pk_scheme();
    if (!s) return PK_ERR_OOM;
    s->r1cs = r1cs;
    s->num_constraints = num_constraints;
    s->num_witnesses = num_witnesses;
    s->m = m;
    s->m_0 = m_0;
    s->nb = nb;
    s->whir_witness = *whir_witness;
    s->whir_hiding = *whir_for_hiding_spartan;
    s->domain_separator = whir_r1cs_io_pattern(s->m_0, s->whir_witness, s->whir_hiding);
    s->arena_bytes = scheme_arena_bytes(m, m_0, num_witnesses, s->whir_witness);
    if (hipMalloc((void**)&s->arena, s->arena_bytes) != hipSuccess) {
        const size_t mib = s->arena_bytes >> 20;
        delete s;
        (void)hipGetLastError();  // the refusal is reported here: it must not stay behind as this thread's "last error" and fail its next launch check
        return set_err(ctx, PK_ERR_OOM, "hipMalloc of the %zu MiB prover arena failed", mib);
    }
    *out = s;
    return PK_OK;
}

int pk_prove(pk_ctx* ctx, pk_scheme* s, const uint64_t* d_witness, size_t n_witness, const uint8_t* rng_seed32, uint8_t* transcript_out,
             size_t cap, size_t* len) {
    PK_ENTER(ctx);
    AbortOnFailure guard(ctx);  // before the argument checks: a rank refused here never joins its peers' collectives either
    std::vector<uint8_t> narg;
    if (int rc = guard.done(prove(ctx, s, d_witness, n_witness, rng_seed32, len, narg))) return rc;
    *len = narg.size();
    if (!transcript_out) return PK_OK;  // size query
    PK_REQUIRE(ctx, cap >= narg.size(), "transcript buffer too small");
    memcpy(transcript_out, narg.data(), narg.size());
    return PK_OK;
}

/* ---- NoirProofSchemeProver::prove after ACVM execution (provekit/prover/src/noir_proof_scheme.rs:63-92) ---- */

// the witness transcript (host only): IOPattern + seed_witness_merlin (noir_proof_scheme.rs:111-133), then one
// fill_challenge_scalars per WitnessBuilder::Challenge (witness_builder.rs:94-98)
int pk_witness_challenges(size_t num_constraints, size_t num_witnesses, const uint64_t* public_inputs, size_t n_public, uint64_t* challenges,
                          size_t n_challenges) {
    if ((n_public && !public_inputs) || (n_challenges && !challenges)) return PK_ERR_BAD_ARG;
    Transcript T(witness_io_pattern(n_public, n_challenges));
    T.add_scalar(h_from_u64(num_constraints));
    T.add_scalar(h_from_u64(num_witnesses));
    for (size_t i = 0; i < n_public; i++) T.add_scalar(h_load(public_inputs + 4 * i));
    for (size_t i = 0; i < n_challenges; i++) h_store(challenges + 4 * i, T.challenge_scalar());
    return PK_OK;
}

int pk_noir_prove(pk_ctx* ctx, pk_scheme* s, pk_witness_program* builders, const uint64_t* d_acir, size_t n_acir, const uint32_t* public_acir_idx,
                  size_t n_public, const uint8_t* rng_seed32, uint8_t* transcript_out, size_t cap, size_t* len) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, s && builders && len && (d_acir || n_acir == 0) && (public_acir_idx || n_public == 0), "null pointer");
    size_t touched = 0, n_chal = 0, acir_read = 0;
    witness_program_shape(builders, &touched, &n_chal, &acir_read);
    PK_REQUIRE(ctx, touched <= s->num_witnesses, "the witness builders write past the R1CS's witness vector");
    for (size_t i = 0; i < n_public; i++) PK_REQUIRE(ctx, public_acir_idx[i] < n_acir, "public input index outside the ACIR witness vector");
    const size_t nw = s->num_witnesses;
    if (!s->noir_witness) PK_HIP(ctx, hipMalloc((void**)&s->noir_witness, 33 * nw));
    uint64_t* d_w = (uint64_t*)s->noir_witness;
    uint8_t* d_set = (uint8_t*)s->noir_witness + 32 * nw;
    // public values -> host
    std::vector<uint64_t> pub(4 * n_public), chal(4 * n_chal);
    if (n_public) {
        uint32_t* m_idx = nullptr;
        int rc = mail_alloc(ctx, 4 * n_public, (void**)&m_idx);
        if (rc) return rc;
        memcpy(m_idx, public_acir_idx, 4 * n_public);
        gather_fe_kernel<<<(unsigned)((n_public + 255) / 256), 256, 0, ctx->stream>>>((const fe*)d_acir, m_idx, n_public, (fe*)d_w);
        PK_LAUNCH_CHECK(ctx);
        PK_HIP(ctx, hipMemcpyAsync(pub.data(), d_w, 32 * n_public, hipMemcpyDeviceToHost, ctx->stream));
        rc = sync_stream(ctx);
        if (rc) return rc;
    }
    AbortOnFailure guard(ctx);  // a witness that fails to solve on this rank only must not leave the others inside pk_prove's collectives
    RngKey key;                 // one key for the fill and the proof's masks (distinct streams)
    auto witness = [&]() -> int {
        int rc = pk_witness_challenges(s->num_constraints, nw, pub.data(), n_public, chal.data(), n_chal);
        if (rc) return set_err(ctx, rc, "witness transcript");
        CK(pk_witness_solve(ctx, builders, d_acir, n_acir, chal.data(), n_chal, d_w, nw, d_set));
        CK(proof_key(ctx, rng_seed32, key));
        return pk_witness_fill(ctx, d_w, d_set, nw, (const uint8_t*)key.k, nullptr);
    };
    if (int rc = guard.done(witness())) return rc;
    return pk_prove(ctx, s, d_w, nw, (const uint8_t*)key.k, transcript_out, cap, len);  // pk_prove carries its own guard
}

int pk_scheme_domain_separator(const pk_scheme* s, char* buf, size_t cap, size_t* len) {
    if (!s || !len) return PK_ERR_BAD_ARG;
    copy_out(s->domain_separator, buf, cap, len);
    return PK_OK;
}

int pk_scheme_set_io_pattern(pk_ctx* ctx, pk_scheme* s, const uint8_t* pattern, size_t n) {
    PK_ENTER(ctx);
    PK_REQUIRE(ctx, s, "null pointer");
    if (!pattern || !n) {  // back to the library's restatement
        s->domain_separator = whir_r1cs_io_pattern(s->m_0, s->whir_witness, s->whir_hiding);
        return PK_OK;
    }
    const std::string theirs((const char*)pattern, n);
    const std::string bad = io_pattern_mismatch(theirs, s->m_0, s->whir_witness, s->whir_hiding);
    if (!bad.empty()) return set_err(ctx, PK_ERR_IO_PATTERN, "%s", bad.c_str());
    s->domain_separator = theirs;
    return PK_OK;
}

/* ---- the host restatement of a commitment and of the grinder (host_whir.hpp), for the suite: host memory in, host memory out ---- */

// commit_into on the host thread: `batch` coefficient vectors of 2^n_vars Montgomery elements each, back to back -> the column-major leaf
// matrix (rows * width elements, Montgomery) and the heap of 2 * rows canonical digests, as pk_commit_into leaves them on the device
int pk_selftest_host_commit(int hash_version, const uint64_t* coeffs, unsigned batch, unsigned n_vars, unsigned log_inv_rate, unsigned fold,
                            uint64_t* leaves_out, uint64_t* nodes_out) {
    if (!coeffs || !leaves_out || !nodes_out || (hash_version != 1 && hash_version != 2) || batch < 1 || batch > 4 || fold > n_vars ||
        n_vars + log_inv_rate - fold > PK_HOST_TAIL_MAX_LOG2)
        return PK_ERR_BAD_ARG;
    const fe* polys[4];
    for (unsigned b = 0; b < batch; b++) polys[b] = (const fe*)coeffs + ((size_t)b << n_vars);
    host_whir::commit(hash_version, polys, batch, n_vars, log_inv_rate, fold, (fe*)leaves_out, (fe*)nodes_out);
    return PK_OK;
}
// pk_pow_solve on the host thread: the smallest valid nonce, by a search in ascending order
int pk_selftest_host_pow(const uint8_t challenge[32], double bits, uint64_t* nonce) {
    if (!challenge || !nonce || !(bits >= 0.0 && bits <= (double)PK_HOST_POW_CEILING)) return PK_ERR_BAD_ARG;
    *nonce = host_whir::pow_grind(challenge, bits);
    return PK_OK;
}

}  // extern "C"
