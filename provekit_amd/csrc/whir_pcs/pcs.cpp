// pcs.cpp -- the device half of libprovekit_whir.so's C ABI: the scheme and its arena, pkw_commit, pkw_open.
//
// pkw_open is whir::Prover::prove restated over the product library's PUBLIC entry points (provekit_hip.h) -- the same steps in the
// same order as prover.hip's WhirProver, which drives them through the library's internals -- with the prover side of the sponge
// (prover_transcript.hpp) enforcing pkw_io_pattern operation by operation.  The evaluation constraints are the weights
// eq(point_i, .): pk_eq_accumulate adds them to the OOD weights with their powers of the combination randomness, so no weight table
// is ever materialised, and their deferred evaluations eq(point_i, folding point) are O(n) products on the host.  The linear
// constraints of pkw_open_linear are dense tables on the device: linear.hip's kernels give their sums and add them to the same
// weight table in one pass, and evaluate.hip's kernel reads them once more at the folding point for their deferred evaluations.
// pkw_open_sparse states the same constraints as index/value lists: the same three steps, each by its twin in sparse.hip.
// pkw_commit_hiding / pkw_open_hiding (provekit_whir_hiding.h) are pkw_commit and pkw_open over the extended batch: hiding.hip draws
// the masks and g, and the opening is the plain one at the points (0, z_i) under the hiding label.
//
// DEVICE SETS.  A scheme on a context of a device set (G ranks, one host thread each, every rank making the same calls with the same
// inputs) shards what pk_commit_into / pk_commit_open shard, under the layouts they report, and the two ALU-bound reductions of the
// statement: rank g runs the workgroups [g n_wg / G, (g + 1) n_wg / G) of the evaluation and weighted-sums kernels, one
// pk_comm_all_gather per pass exchanges the slices' partials, and the finish kernel adds the gathered blocks on every rank -- the
// partials are fully reduced and field addition is exact, so the bits are the lone grid's.  Everything else stays replicated.
// The library can only call what provekit_hip.h declares, so a rank must never skip a collective its peers will enter: refusals
// every rank makes identically come before any collective, and after every rank-local step that can fail the ranks exchange their
// status (exchange() below; the slice passes carry it inside the gather they make anyway) and leave together.
#include <hip/hip_runtime.h>
#include <sys/random.h>

#include <cerrno>
#include <map>

#include "../prover_transcript.hpp"
#include "evaluate.hpp"
#include "hiding.hpp"
#include "linear.hpp"
#include "pcs.hpp"
#include "sparse.hpp"

using pk::fe;

struct pkw_scheme {
    pk_ctx* ctx = nullptr;
    pk_whir_config cfg{};
    std::map<unsigned, std::string> pattern_cache;  // io_pattern(cfg, q, l) by q * (PKW_MAX_WEIGHTS + 1) + l; l = 0: pkw_open's; a hiding opening's (l = 0) by HIDING_KEYS + q, above every plain key
    std::string err;
    hipStream_t stream = nullptr;  // the evaluation kernel's
    uint64_t* arena = nullptr;
    size_t arena_fes = 0;
    pkw::Plan plan;  // the arena's, under the context's device set
    // a device set: this rank, the ranks, and the buffer their exchanges go through: a send block of xchg_send_fes elements, then
    // room for every rank's
    unsigned rank = 0, world = 1;
    uint64_t* xchg = nullptr;
    size_t xchg_send_fes = 0;
};

struct pkw_commitment {
    const pkw_scheme* scheme = nullptr;
    pk_ctx* ctx = nullptr;
    uint64_t* block = nullptr;  // one allocation: evaluations, coefficients, codeword, tree
    const uint64_t* evals[4] = {};
    const uint64_t* coeffs[4] = {};
    uint64_t *leaves = nullptr, *nodes = nullptr;
    size_t rows = 0, width = 0;
    pk_commit_layout layout{};
    uint8_t root[32] = {};
};

// a commitment to (f^_0 .. f^_{B-1}, g): the plain commitment of the extended batch, and whether its one opening was handed out
struct pkw_hiding_commitment {
    pkw_commitment* inner = nullptr;
    bool opened = false;
};

namespace pkw {
namespace {

#define CK(expr)                     \
    do {                             \
        const int rc_ = (expr);      \
        if (rc_ != PK_OK) return rc_; \
    } while (0)

inline uint64_t* U(fe* p) { return reinterpret_cast<uint64_t*>(p); }
inline const uint64_t* U(const fe* p) { return reinterpret_cast<const uint64_t*>(p); }

int fail(pkw_scheme* s, int rc, const std::string& why) {
    s->err = why;
    return rc;
}

// ---- device sets: what the ranks tell each other outside the product's own sharded calls ------------------------------------------
// One small all-gather: every rank contributes 32 bytes and the status of its rank-local work so far, and gets every rank's 32 bytes
// (all: world * 32 bytes, may be null) and the FIRST non-zero status of the set in rank order, so that all ranks leave together before
// the next sharded product call.  Outside a set: the status itself, nothing is enqueued.  A failure of the exchange itself is the
// communicator's (PK_ERR_RCCL): the product has poisoned it for every rank by then
int exchange(pkw_scheme* s, int status, const uint8_t mine[32], uint8_t* all) {
    if (s->world == 1) {
        if (all && mine) memcpy(all, mine, 32);
        return status;
    }
    uint64_t block[8] = {};
    if (mine) memcpy(block, mine, 32);
    block[4] = (uint64_t)(int64_t)status;
    std::vector<uint64_t> got(8 * (size_t)s->world);
    uint64_t *send = s->xchg, *recv = s->xchg + 4 * s->xchg_send_fes;
    int rc = pk_memcpy_h2d(s->ctx, send, block, sizeof block);
    if (!rc) rc = pk_comm_all_gather(s->ctx, send, recv, sizeof block);
    if (!rc) rc = pk_memcpy_d2h(s->ctx, got.data(), recv, sizeof block * s->world);
    if (rc) return fail(s, rc, std::string("exchange between the ranks: ") + pk_last_error(s->ctx));
    for (unsigned g = 0; g < s->world; g++)
        if (all) memcpy(all + 32 * (size_t)g, &got[8 * (size_t)g], 32);
    for (unsigned g = 0; g < s->world; g++)
        if (const int theirs = (int)(int64_t)got[8 * (size_t)g + 4]) {
            if (g != s->rank || s->err.empty()) s->err = "rank " + std::to_string(g) + " of the device set failed with status " + std::to_string(theirs);
            return theirs;
        }
    return PK_OK;
}

// the arena, handed out front to back; an opening starts from the front again
struct Bump {
    uint64_t* base;
    size_t cap, used = 0;
    uint64_t* take(size_t fes) {
        fes = round8(fes ? fes : 1);
        if (used + fes > cap) return nullptr;
        uint64_t* p = base + 4 * used;
        used += fes;
        return p;
    }
};
constexpr int RANKS_DISAGREE = -1000;  // Opening::run to open_checked, which names it: never a status of the ABI
#define TAKE(var, fes)                         \
    uint64_t* var = A.take(fes);               \
    if (!var) return PK_ERR_OOM /* plan() and the opening disagree: a bug of this file */

struct Tree {  // a committed codeword: what a round's STIR queries open
    const uint64_t *leaves, *nodes;
    size_t rows, width;
    pk_commit_layout layout;
};

struct Opening {
    pkw_scheme& S;
    const pkw_commitment& C;
    pk::Transcript& T;
    Bump A;
    pk_ctx* ctx;
    const pk_whir_config& cfg;
    const unsigned n, k;
    uint64_t *p[2] = {}, *w[2] = {};
    int cur = 0;
    size_t len;
    std::vector<fe> rs, all_r;

    Opening(pkw_scheme& s, const pkw_commitment& c, pk::Transcript& t)
        : S(s), C(c), T(t), A{s.arena, s.arena_fes}, ctx(s.ctx), cfg(s.cfg), n(s.cfg.n_vars), k(s.cfg.folding_factor), len((size_t)1 << s.cfg.n_vars) {}

    // dst = sum_b beta^b x_b (mtUtilities.go:98-114)
    int batch_combine(uint64_t* dst, const uint64_t* const* x, const fe& beta) {
        const size_t N = (size_t)1 << n;
        CK(pk_memcpy_d2d(ctx, dst, x[0], 32 * N));
        fe bp = beta;
        for (unsigned b = 1; b < cfg.batch_size; b++) {
            CK(pk_fe_axpy(ctx, dst, U(&bp), x[b], N));
            bp = pk::h_mul(bp, beta);
        }
        return PK_OK;
    }
    // w (+)= sum_j scale0 * gamma^j * eq(pts_j, .) over nv variables; *next = the following power
    int eq_weights(uint64_t* dst, unsigned nv, const std::vector<fe>& pts, size_t count, const fe& gamma, fe g, int overwrite, fe* next) {
        std::vector<fe> scales(count ? count : 1);
        for (size_t j = 0; j < count; j++) {
            scales[j] = g;
            g = pk::h_mul(g, gamma);
        }
        *next = g;
        if (!count) return pk_eq_accumulate(ctx, dst, nv, nullptr, nullptr, 0, overwrite);
        for (size_t j0 = 0; j0 < count; j0 += 32) {  // the points travel through the context's pinned mailbox: modest pieces
            const size_t c = std::min<size_t>(32, count - j0);
            CK(pk_eq_accumulate(ctx, dst, nv, U(pts.data() + j0 * nv), U(scales.data() + j0), (unsigned)c, overwrite && j0 == 0));
        }
        return PK_OK;
    }
    void flip() {
        cur = 1 - cur;
        len /= 2;
    }
    // the same steps in the same order as WhirProver::sumcheck_rounds (prover.hip), synchronous form
    int sumcheck_rounds(unsigned rounds) {
        rs.clear();
        for (unsigned t = 0; t < rounds; t++) {
            uint64_t out[12];
            CK(pk_sumcheck_quadratic_round(ctx, p[cur], w[cur], len, t ? U(&rs.back()) : nullptr, p[1 - cur], w[1 - cur], out));
            if (t) flip();
            const fe msg[3] = {pk::h_load(out), pk::h_load(out + 4), pk::h_load(out + 8)};
            T.add_scalars(msg, 3);
            const fe r = T.challenge_scalar();
            rs.push_back(r);
            all_r.push_back(r);
        }
        if (rounds && len >= 2) {  // apply the last challenge: p, w now describe the folded polynomial
            CK(pk_fold_pairs(ctx, p[cur], len, U(&rs.back()), p[1 - cur]));
            CK(pk_fold_pairs(ctx, w[cur], len, U(&rs.back()), w[1 - cur]));
            flip();
        }
        return PK_OK;
    }
    std::vector<uint64_t> stir_queries(size_t domain, unsigned queries) {
        std::vector<uint8_t> raw(pk::stir_query_bytes(domain, k) * queries);
        T.challenge_bytes(raw.data(), raw.size());
        return pk::stir_indexes(raw.data(), domain, k, queries);
    }
    int pow_round(double bits) {
        if (bits <= 0.0) return PK_OK;
        uint8_t challenge[pk::POW_CHALLENGE_BYTES], be[pk::POW_NONCE_BYTES];
        T.challenge_bytes(challenge, sizeof challenge);
        uint64_t nonce = 0;
        CK(pk_pow_solve(ctx, challenge, bits, &nonce));
        pk::nonce_to_bytes(nonce, be);
        T.add_bytes(be, sizeof be);
        return PK_OK;
    }
    // hints: stir_answers = Vec<Vec<F>> and merkle_proof = ark MultiPath (common.go:36-61)
    int opening_hints(const Tree& t, const std::vector<uint64_t>& idx) {
        const size_t q = idx.size();
        unsigned logn = 0;
        while (((size_t)1 << logn) < t.rows) logn++;
        const size_t plen = logn ? logn - 1 : 0;
        std::vector<uint64_t> leaves(4 * q * t.width + 4), sib(4 * q + 4), paths(4 * q * plen + 4);
        CK(pk_commit_open(ctx, t.leaves, t.nodes, t.rows, t.width, &t.layout, idx.data(), q, /*canonical=*/1, leaves.data(), sib.data(), paths.data()));
        std::vector<uint8_t> buf;
        pk::put_u64(buf, q);
        for (size_t j = 0; j < q; j++) pk::put_vec(buf, (const fe*)(leaves.data() + 4 * j * t.width), t.width, /*montgomery=*/false);
        T.hint(buf.data(), buf.size());
        size_t mlen = 0;
        pk_multipath_serialize(idx.data(), q, plen, sib.data(), paths.data(), nullptr, 0, &mlen);
        std::vector<uint8_t> mp(mlen ? mlen : 1);
        CK(pk_multipath_serialize(idx.data(), q, plen, sib.data(), paths.data(), mp.data(), mlen, &mlen));
        T.hint(mp.data(), mlen);
        return PK_OK;
    }

    // ---- rank slices of the two reductions (a device set).  slice(n_wg) = the workgroups per rank, 0 = the pass runs replicated:
    // outside a set, with fewer workgroups than ranks, or when the ranks do not divide them
    unsigned slice(unsigned n_wg) const { return S.world > 1 && n_wg >= S.world && n_wg % S.world == 0 ? n_wg / S.world : 0; }
    uint64_t* slice_partials() const { return S.xchg; }
    // After this rank's slice of a pass was enqueued on the scheme's stream with `status`: its P partials and the status travel in one
    // all-gather, every rank returns the first non-zero status of the set, and the finish kernel adds the G gathered blocks of
    // `chunk` workgroups each: d_out[y * out_stride + i] for y < rows, i < count
    int gather_finish(int status, size_t P, unsigned chunk, unsigned rows, unsigned count, unsigned row_stride, uint64_t* d_out, unsigned out_stride) {
        if (hipStreamSynchronize(S.stream) != hipSuccess && !status) status = PK_ERR_HIP;
        uint64_t *send = S.xchg, *recv = S.xchg + 4 * S.xchg_send_fes;
        uint64_t st[4] = {(uint64_t)(int64_t)status, 0, 0, 0};
        CK(pk_memcpy_h2d(ctx, send + 4 * P, st, sizeof st));
        CK(pk_comm_all_gather(ctx, send, recv, 32 * (P + 1)));
        CK(pk_ctx_sync(ctx));
        for (unsigned g = 0; g < S.world; g++) {
            CK(pk_memcpy_d2h(ctx, st, recv + 4 * (g * (P + 1) + P), 8));
            if (const int theirs = (int)(int64_t)st[0]) {
                S.err = "rank " + std::to_string(g) + " of the device set failed in its slice of a reduction with status " + std::to_string(theirs);
                return theirs;
            }
        }
        finish_launch(S.stream, recv, chunk * S.world, rows, count, row_stride, d_out, out_stride, chunk, P + 1);
        return hipGetLastError() == hipSuccess ? PK_OK : PK_ERR_HIP;
    }
    // eval_launch, every pass sliced over the ranks where slice() allows
    int evaluations(const uint64_t* const* d_evals, unsigned batch, const uint64_t* d_points, unsigned q, uint64_t* d_part, uint64_t* d_out) {
        const unsigned per = slice(eval_grid(n));
        if (!per) return eval_launch(S.stream, d_evals, batch, n, d_points, q, d_part, d_out);
        if ((size_t)batch * EVAL_PASS * per + 1 > S.xchg_send_fes) return PK_ERR_OOM;  // every rank alike, before any launch or collective
        for (unsigned q0 = 0; q0 < q; q0 += EVAL_PASS) {
            const unsigned Q = std::min(EVAL_PASS, q - q0);
            const int rc = eval_slice_launch(S.stream, d_evals, batch, n, d_points + 4 * (size_t)q0 * n, Q, S.rank * per, per, slice_partials());
            CK(gather_finish(rc, (size_t)batch * EVAL_PASS * per, per, batch, Q, EVAL_PASS, d_out + 4 * (size_t)q0, q));
        }
        return PK_OK;
    }
    // wsum_launch, likewise
    int dense_sums(const Statement& W, uint64_t* d_part, uint64_t* d_out) {
        const unsigned batch = cfg.batch_size, per = slice(wsum_grid(n));
        if (!per) return wsum_launch(S.stream, C.evals, batch, n, W.dense, W.l, d_part, d_out);
        if ((size_t)batch * WSUM_PASS * per + 1 > S.xchg_send_fes) return PK_ERR_OOM;  // every rank alike, before any launch or collective
        for (unsigned i0 = 0; i0 < W.l; i0 += WSUM_PASS) {
            const unsigned L = std::min(WSUM_PASS, W.l - i0);
            const int rc = wsum_slice_launch(S.stream, C.evals, batch, n, W.dense + i0, L, S.rank * per, per, slice_partials());
            CK(gather_finish(rc, (size_t)batch * L * per, per, batch, L, L, d_out + 4 * (size_t)i0, W.l));
        }
        return PK_OK;
    }

    // the three steps that read the statement's weights: dense device tables, or validated index/value lists.
    // d_out[b * l + i] = <w_i, poly_b>
    int weight_sums(const Statement& W, uint64_t* d_part, uint64_t* d_out) {
        if (W.sparse) return sparse_sums_launch(S.stream, C.evals, cfg.batch_size, n, *W.sparse, d_part, d_out);
        return dense_sums(W, d_part, d_out);
    }
    // d_w += sum_i scales[i] w_i
    int weight_combine(const Statement& W, uint64_t* d_w, const fe* scales) {
        if (W.sparse) return sparse_accumulate_launch(S.stream, d_w, *W.sparse, U(scales));
        return combine_launch(S.stream, d_w, (size_t)1 << n, W.dense, U(scales), W.l, /*accumulate=*/1);
    }
    // d_out[i] = the extension of w_i at d_point.  The dense tables are read EVAL_MAX_BATCH at a time by the evaluation kernel (its
    // partials for EVAL_MAX_BATCH tables go into the commit scratch, idle by now); the lists' partials go where the sums' went
    int weight_deferred(const Statement& W, const uint64_t* d_point, uint64_t* d_part, uint64_t* scratch, uint64_t* d_out) {
        if (W.sparse) return sparse_evaluate_launch(S.stream, n, *W.sparse, d_point, d_part, d_out);
        if (eval_partial_fes(EVAL_MAX_BATCH, n) > S.plan.scratch) return PK_ERR_OOM;
        for (unsigned i0 = 0; i0 < W.l; i0 += EVAL_MAX_BATCH)
            CK(evaluations(W.dense + i0, std::min(EVAL_MAX_BATCH, W.l - i0), d_point, 1, scratch, d_out + 4 * (size_t)i0));
        return PK_OK;
    }

    // q evaluation constraints, then l linear ones (l = 0: pkw_open)
    int run(const Statement& W, fe* evals /* batch * q */, fe* sums /* batch * l */) {
        const size_t N = (size_t)1 << n;
        const unsigned batch = cfg.batch_size, q = W.q, l = W.l;
        const fe *points = reinterpret_cast<const fe*>(W.points), *tags = reinterpret_cast<const fe*>(W.tags);
        TAKE(scratch, S.plan.scratch);
        // 1-3: the commitment's transcript (mtUtilities.go:51-76)
        T.add_canon(pk::load_raw(C.root));
        std::vector<fe> ood(cfg.commitment_ood_samples), ood_ans((size_t)batch * ood.size());
        T.challenge_scalars(ood.data(), ood.size());
        for (unsigned b = 0; b < batch; b++)
            for (size_t j = 0; j < ood.size(); j++) CK(pk_eval_univariate(ctx, C.coeffs[b], N, U(&ood[j]), U(&ood_ans[b * ood.size() + j])));
        for (unsigned b = 0; b < batch; b++) T.add_scalars(&ood_ans[b * ood.size()], ood.size());
        const fe beta = batch > 1 ? T.challenge_scalar() : pk::fe_one();
        // 4, 5: the statement.  The partials of the sums go where the evaluation's went (the two uses are sequential; a pass of
        // WSUM_PASS weights needs what a pass of EVAL_PASS points does, on a grid that is never larger)
        T.add_scalars(points, (size_t)q * n);
        T.add_scalars(tags, l);
        TAKE(d_pts, (size_t)PKW_MAX_POINTS * n);
        TAKE(d_part, eval_partial_fes(batch, n));
        TAKE(d_out, (size_t)PKW_MAX_POINTS * batch);
        if ((W.sparse ? sparse_partial_fes(batch, n) : wsum_partial_fes(batch, n)) > eval_partial_fes(batch, n)) return PK_ERR_OOM;
        CK(pk_ctx_sync(ctx));
        if (q) {
            CK(pk_memcpy_h2d(ctx, d_pts, points, 32 * (size_t)q * n));
            CK(pk_ctx_sync(ctx));
            CK(evaluations(C.evals, batch, d_pts, q, d_part, d_out));
            if (hipStreamSynchronize(S.stream) != hipSuccess) return PK_ERR_HIP;
            CK(pk_memcpy_d2h(ctx, evals, d_out, 32 * (size_t)batch * q));
        }
        T.add_scalars(evals, (size_t)batch * q);
        if (l) {
            CK(weight_sums(W, d_part, d_out));
            if (hipStreamSynchronize(S.stream) != hipSuccess) return PK_ERR_HIP;
            CK(pk_memcpy_d2h(ctx, sums, d_out, 32 * (size_t)batch * l));
        }
        T.add_scalars(sums, (size_t)batch * l);
        if (S.world > 1) {  // the statement is absorbed: the ranks hold the same sponge, or leave together before the first STIR opening
            const fe mine = T.peek_challenge();
            std::vector<uint8_t> all(32 * (size_t)S.world);
            CK(exchange(&S, PK_OK, (const uint8_t*)mine.v, all.data()));
            for (unsigned g = 1; g < S.world; g++)
                if (memcmp(all.data(), all.data() + 32 * (size_t)g, 32)) return RANKS_DISAGREE;
        }
        // 6: whir::Prover::prove over the beta-combined polynomial
        TAKE(d_c0, N);
        uint64_t* d_c = d_c0;
        CK(batch_combine(d_c, C.coeffs, beta));
        TAKE(p0, N);
        TAKE(p1, N / 2);
        TAKE(w0, N);
        TAKE(w1, N / 2);
        p[0] = p0, p[1] = p1, w[0] = w0, w[1] = w1;
        CK(batch_combine(p0, C.evals, beta));
        fe gamma = T.challenge_scalar(), g;
        {  // weights = sum gamma^i w_i over [OOD constraints..., eq(point_i, .)..., the l weights...]
            std::vector<fe> pts((ood.size() + q) * n + 1);
            for (size_t j = 0; j < ood.size(); j++) pk::expand_from_univariate(ood[j], n, &pts[j * n]);
            std::copy(points, points + (size_t)q * n, pts.begin() + ood.size() * n);
            CK(eq_weights(w0, n, pts, ood.size() + q, gamma, pk::fe_one(), /*overwrite=*/1, &g));
            if (l) {
                std::vector<fe> scales(l);
                for (unsigned i = 0; i < l; i++) {
                    scales[i] = g;
                    g = pk::h_mul(g, gamma);
                }
                CK(pk_ctx_sync(ctx));  // the eq weights are the context's work: in the table before the kernel adds to it
                CK(weight_combine(W, w0, scales.data()));
                if (hipStreamSynchronize(S.stream) != hipSuccess) return PK_ERR_HIP;
            }
        }
        CK(sumcheck_rounds(k));
        Tree prev{C.leaves, C.nodes, C.rows, C.width, C.layout};
        unsigned nv = n, rate = cfg.starting_log_inv_rate;
        size_t domain = (size_t)1 << (n + rate);
        fe exp_gen = pk::folded_domain_generator(n + rate, k);
        for (unsigned r = 0; r < cfg.n_rounds; r++) {  // whir.go:51-220
            const unsigned nv2 = nv - k;
            TAKE(d_c2, (size_t)1 << nv2);
            CK(pk_fold_coeffs(ctx, d_c, nv, U(rs.data()), k, d_c2));
            d_c = d_c2;
            nv = nv2;
            rate += k - 1;
            Tree next{};
            next.rows = (size_t)1 << (nv + rate - k);
            next.width = (size_t)1 << k;
            size_t leaves_fes = 0, nodes_fes = 0;  // a rank of a device set keeps its rows of a sharded codeword: what the arena was planned with
            CK(pk_commit_sizes(ctx, 1, nv, rate, k, &leaves_fes, &nodes_fes, nullptr));
            TAKE(leaves, leaves_fes);
            TAKE(nodes, nodes_fes);
            next.leaves = leaves, next.nodes = nodes;
            fe root;
            const uint64_t* cp[1] = {d_c};
            CK(pk_commit_into(ctx, cp, 1, nv, rate, k, leaves, nodes, scratch, (uint8_t*)root.v, &next.layout));
            T.add_canon(root);
            std::vector<fe> zs(cfg.ood_samples[r]), ans(cfg.ood_samples[r]);
            T.challenge_scalars(zs.data(), zs.size());
            for (size_t j = 0; j < zs.size(); j++) CK(pk_eval_univariate(ctx, d_c, (size_t)1 << nv, U(&zs[j]), U(&ans[j])));
            T.add_scalars(ans.data(), ans.size());
            CK(pow_round(cfg.pow_bits[r]));
            const std::vector<uint64_t> idx = stir_queries(domain, cfg.num_queries[r]);
            CK(opening_hints(prev, idx));
            gamma = T.challenge_scalar();
            for (uint64_t i : idx) zs.push_back(pk::h_pow(exp_gen, i));
            std::vector<fe> pts(zs.size() * (nv ? nv : 1));
            for (size_t j = 0; j < zs.size(); j++) pk::expand_from_univariate(zs[j], nv, &pts[j * nv]);
            CK(eq_weights(w[cur], nv, pts, zs.size(), gamma, pk::fe_one(), 0, &g));
            CK(sumcheck_rounds(k));
            prev = next;
            domain /= 2;
            exp_gen = pk::h_mul(exp_gen, exp_gen);
        }
        // the final round: the folded polynomial in the clear, PoW, final STIR openings, final sumcheck
        const unsigned final_vars = nv - k;
        TAKE(d_final, (size_t)1 << final_vars);
        CK(pk_fold_coeffs(ctx, d_c, nv, U(rs.data()), k, d_final));
        std::vector<fe> fin((size_t)1 << final_vars);
        CK(pk_memcpy_d2h(ctx, fin.data(), d_final, 32 * fin.size()));
        T.add_scalars(fin.data(), fin.size());
        CK(pow_round(cfg.final_pow_bits));
        CK(opening_hints(prev, stir_queries(domain, cfg.final_queries)));
        CK(sumcheck_rounds(final_vars));
        CK(pow_round(cfg.final_folding_pow_bits));
        // deferred_weight_evaluations: each weight's MLE at the folding point, reverse(all_r) in eval_eq's MSB-first order; for
        // eq(point_i, .) that is eq(point_i, folding point); the l weights are read once more (weight_deferred)
        const std::vector<fe> point(all_r.rbegin(), all_r.rend());
        std::vector<fe> deferred(q + l);
        for (unsigned i = 0; i < q; i++) deferred[i] = pkv::eq_poly(points + (size_t)i * n, point.data(), n);
        if (l) {
            CK(pk_memcpy_h2d(ctx, d_pts, point.data(), 32 * (size_t)n));
            CK(pk_ctx_sync(ctx));
            CK(weight_deferred(W, d_pts, d_part, scratch, d_out));
            if (hipStreamSynchronize(S.stream) != hipSuccess) return PK_ERR_HIP;
            CK(pk_memcpy_d2h(ctx, deferred.data() + q, d_out, 32 * (size_t)l));
        }
        std::vector<uint8_t> buf;
        pk::put_vec(buf, deferred.data(), q + l);
        T.hint(buf.data(), buf.size());
        return PK_OK;
    }
};

}  // namespace
}  // namespace pkw

extern "C" {

const char* pkw_last_error(const pkw_scheme* s) { return s ? s->err.c_str() : "null scheme"; }

int pkw_scheme_create(pk_ctx* ctx, const pk_whir_config* cfg, pkw_scheme** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return pkw::refuse("null pointer");
    std::string why;
    if (!pkw::config_ok(cfg, why)) return pkw::refuse(why);
    int rank = 0, world = 1, kind = 0;
    if (pk_comm_info(ctx, &rank, &world, &kind) != PK_OK || world < 1 || rank < 0 || rank >= world) return pkw::refuse("the context's communicator");
    // The arena under the context's device set: pk_commit_sizes for every commit of an opening.  A rank keeps 1 / G of a sharded
    // codeword, never more than the whole; the sharded commit's scratch (the encode's staging plus local and gathered digests) may
    // exceed the lone one's by up to 1.5 digests per row (G = 2, and narrow codewords at G = 4), which is what the bound below allows
    // on top of the host-only figure of pkw_scheme_arena_bytes.  Checked here, not assumed
    pkw::Plan planned;
    const pkw::Plan lone = pkw::plan(*cfg);
    bool leaves_grew = false;
    const unsigned fold = cfg->folding_factor;
    const int prc = pkw::plan_with(*cfg, [&](unsigned batch, unsigned nv, unsigned rate, size_t* leaves, size_t* nodes, size_t* scratch) {
        const int rc = pk_commit_sizes(ctx, batch, nv, rate, fold, leaves, nodes, scratch);
        const size_t rows = (size_t)1 << (nv + rate - fold), width = (size_t)batch << fold;
        if (!rc && (*leaves > rows * width || *nodes > 2 * rows)) leaves_grew = true;
        return rc;
    }, planned);
    if (prc) return pkw::refuse("pk_commit_sizes refuses this config");
    const size_t rows0 = (size_t)1 << (cfg->n_vars + cfg->starting_log_inv_rate - fold);
    if (leaves_grew || planned.total > lone.total + 2 * rows0)
        return pkw::refuse("the arena under this device set exceeds pkw_scheme_arena_bytes by more than 64 bytes per row of the codeword");
    try {
        pkw_scheme* s = new pkw_scheme();
        s->ctx = ctx;
        s->cfg = *cfg;
        s->rank = (unsigned)rank, s->world = (unsigned)world;
        s->plan = planned;
        s->arena_fes = planned.total;
        int rc = pk_ctx_sync(ctx);  // selects the context's device on this thread
        if (!rc) rc = pk_malloc(ctx, 32 * s->arena_fes, (void**)&s->arena);
        if (!rc && world > 1) {  // a slice's partials and its status; then every rank's
            const unsigned n = cfg->n_vars;
            const size_t pass = std::max(pkw::eval_partial_fes(pkw::EVAL_MAX_BATCH, n), pkw::wsum_partial_fes(pkw::WSUM_MAX_BATCH, n));
            s->xchg_send_fes = pkw::round8(pass / 2 + 2);  // at least two ranks share a pass; never less than an Exchange block
            rc = pk_malloc(ctx, 32 * (s->xchg_send_fes + pkw::round8(pass + 2 * (size_t)world)), (void**)&s->xchg);
        }
        if (!rc && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) rc = PK_ERR_HIP;
        if (rc) {
            pkw::g_error = std::string("arena: ") + pk_last_error(ctx);
            pkw_scheme_destroy(s);
            return rc;
        }
        *out = s;
        pkw::g_error.clear();
        return PK_OK;
    } catch (...) {
        pkw::g_error = "out of memory";
        return PK_ERR_OOM;
    }
}

int pkw_scheme_destroy(pkw_scheme* s) {
    if (!s) return PK_OK;
    pk_ctx_sync(s->ctx);  // also selects the device
    if (s->stream) (void)hipStreamDestroy(s->stream);
    if (s->arena) pk_free(s->ctx, s->arena);
    if (s->xchg) pk_free(s->ctx, s->xchg);
    delete s;
    return PK_OK;
}

}  // extern "C"

namespace pkw {
namespace {

// pkw_commit after its refusals.  `rc`: the status of the caller's own rank-local work (pkw_commit_hiding's block and masks); what
// fails here before the commit is rank-local too (the allocation, the copies, the coefficient forms), so in a device set the ranks
// exchange their status once, and all of them leave with the first failure before pk_commit_into enters its collectives
int commit_checked(pkw_scheme* s, const uint64_t* const* d_evals, int rc, pkw_commitment** out) {
    const pk_whir_config& c = s->cfg;
    pkw_commitment* com = nullptr;
    if (!rc) {
        s->err.clear();
        try {
            com = new pkw_commitment();
        } catch (...) {
            rc = fail(s, PK_ERR_OOM, "out of memory");
        }
    }
    if (rc) return exchange(s, rc, nullptr, nullptr);
    com->scheme = s;
    com->ctx = s->ctx;
    const size_t N = (size_t)1 << c.n_vars;
    size_t leaves_fes = 0, nodes_fes = 0, scratch_fes = 0;
    rc = pk_commit_sizes(s->ctx, c.batch_size, c.n_vars, c.starting_log_inv_rate, c.folding_factor, &leaves_fes, &nodes_fes, &scratch_fes);
    if (!rc && scratch_fes > s->arena_fes) rc = PK_ERR_OOM;
    if (!rc) rc = pk_malloc(s->ctx, 32 * (2 * c.batch_size * N + leaves_fes + nodes_fes), (void**)&com->block);
    if (!rc) {
        uint64_t* at = com->block;
        for (unsigned b = 0; b < c.batch_size && !rc; b++) {
            uint64_t *ev = at, *co = at + 4 * N;
            at += 8 * N;
            com->evals[b] = ev;
            com->coeffs[b] = co;
            rc = pk_memcpy_d2d(s->ctx, ev, d_evals[b], 32 * N);
            if (!rc) rc = pk_to_coeffs_into(s->ctx, ev, co, c.n_vars);
        }
        com->leaves = at;
        com->nodes = at + 4 * leaves_fes;
        com->rows = (size_t)1 << (c.n_vars + c.starting_log_inv_rate - c.folding_factor);
        com->width = (size_t)c.batch_size << c.folding_factor;
    }
    if (rc) s->err = std::string("commit: ") + pk_last_error(s->ctx);
    if ((rc = exchange(s, rc, nullptr, nullptr))) {
        pkw_commitment_destroy(com);
        return rc;
    }
    rc = pk_commit_into(s->ctx, com->coeffs, c.batch_size, c.n_vars, c.starting_log_inv_rate, c.folding_factor, com->leaves, com->nodes, s->arena, com->root,
                        &com->layout);
    if (rc) {
        s->err = std::string("commit: ") + pk_last_error(s->ctx);
        pkw_commitment_destroy(com);
        return rc;
    }
    *out = com;
    return PK_OK;
}

}  // namespace
}  // namespace pkw

extern "C" {

int pkw_commit(pkw_scheme* s, const uint64_t* const* d_evals, pkw_commitment** out) {
    if (out) *out = nullptr;
    if (!s) return PK_ERR_BAD_ARG;
    if (!d_evals || !out) return pkw::fail(s, PK_ERR_BAD_ARG, "null pointer");
    for (unsigned b = 0; b < s->cfg.batch_size; b++)
        if (!d_evals[b]) return pkw::fail(s, PK_ERR_BAD_ARG, "null polynomial");
    return pkw::commit_checked(s, d_evals, PK_OK, out);
}

int pkw_commitment_root(const pkw_commitment* com, uint8_t root[32]) {
    if (!com || !root) return PK_ERR_BAD_ARG;
    memcpy(root, com->root, 32);
    return PK_OK;
}

int pkw_commitment_destroy(pkw_commitment* com) {
    if (!com) return PK_OK;
    if (com->block) {
        pk_ctx_sync(com->ctx);
        pk_free(com->ctx, com->block);
    }
    delete com;
    return PK_OK;
}

}  // extern "C"

namespace pkw {
namespace {

// What the three openings share once the entry's own count rule has passed.  open_refused: the pointers every opening needs and
// the commitment's owner.  open_checked: the pattern, the opening, the proof into (proof_out, cap, *len)
int open_refused(pkw_scheme* s, const pkw_commitment* com, const Statement& st, const uint8_t* proof_out, size_t cap, const size_t* len) {
    if (!com || (st.q && !st.points) || (st.l && !st.tags) || !len || (cap && !proof_out)) return fail(s, PK_ERR_BAD_ARG, "null pointer");
    if (com->scheme != s) return fail(s, PK_ERR_BAD_ARG, "the commitment belongs to another scheme");
    return PK_OK;
}
int open_checked(pkw_scheme* s, const pkw_commitment* com, const Statement& st, uint64_t* evals_out, uint64_t* sums_out, uint8_t* proof_out, size_t cap,
                 size_t* len) {
    try {
        constexpr unsigned HIDING_KEYS = (PKW_MAX_POINTS + 1) * (PKW_MAX_WEIGHTS + 1);  // one more than the largest plain key
        std::string& pattern = s->pattern_cache[st.hiding ? HIDING_KEYS + st.q : st.q * (PKW_MAX_WEIGHTS + 1) + st.l];
        if (pattern.empty()) pattern = io_pattern(s->cfg, st.q, st.l, st.hiding);
        pk::Transcript T(pattern);
        const size_t batch = s->cfg.batch_size;
        std::vector<fe> evals(batch * st.q + 1), sums(batch * st.l + 1);
        Opening op(*s, *com, T);
        s->err.clear();
        const int rc = op.run(st, evals.data(), sums.data());
        if (rc == RANKS_DISAGREE) return fail(s, PK_ERR_BAD_ARG, "ranks disagree on the statement: every rank of a device set opens with the same inputs");
        if (rc && !s->err.empty()) return rc;  // a status of the set, named by the exchange that found it
        if (rc) return fail(s, rc, rc == PK_ERR_OOM ? "the arena is too small for this opening" : std::string("open: ") + pk_last_error(s->ctx));
        if (!T.finished()) return fail(s, PK_ERR_IO_PATTERN, T.violation().empty() ? "the proof ended before its IO pattern did" : T.violation());
        *len = T.narg.size();
        if (cap < T.narg.size()) return fail(s, PK_ERR_BAD_ARG, "proof buffer too small: " + std::to_string(T.narg.size()) + " bytes needed");
        memcpy(proof_out, T.narg.data(), T.narg.size());
        if (evals_out) memcpy(evals_out, evals.data(), 32 * batch * st.q);
        if (sums_out) memcpy(sums_out, sums.data(), 32 * batch * st.l);
        return PK_OK;
    } catch (...) {
        return fail(s, PK_ERR_OOM, "out of memory");
    }
}

}  // namespace
}  // namespace pkw

extern "C" {

int pkw_open(pkw_scheme* s, const pkw_commitment* com, const uint64_t* points, unsigned q, uint64_t* evals_out, uint8_t* proof_out, size_t cap,
             size_t* len) {
    if (!s) return PK_ERR_BAD_ARG;
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::fail(s, PK_ERR_BAD_ARG, "the number of points must be 1..64");
    const pkw::Statement st{points, q};
    if (int rc = pkw::open_refused(s, com, st, proof_out, cap, len)) return rc;
    return pkw::open_checked(s, com, st, evals_out, nullptr, proof_out, cap, len);
}

// provekit_whir_linear.h
int pkw_open_linear(pkw_scheme* s, const pkw_commitment* com, const uint64_t* points, unsigned q, const uint64_t* const* d_weights, const uint64_t* tags,
                    unsigned l, uint64_t* evals_out, uint64_t* sums_out, uint8_t* proof_out, size_t cap, size_t* len) {
    if (!s) return PK_ERR_BAD_ARG;
    std::string why;
    if (!pkw::linear_counts_ok(q, l, why)) return pkw::fail(s, PK_ERR_BAD_ARG, why);
    const pkw::Statement st{points, q, tags, l, d_weights};
    if (int rc = pkw::open_refused(s, com, st, proof_out, cap, len)) return rc;
    if (!d_weights) return pkw::fail(s, PK_ERR_BAD_ARG, "null pointer");
    for (unsigned i = 0; i < l; i++)
        if (!d_weights[i]) return pkw::fail(s, PK_ERR_BAD_ARG, "weight " + std::to_string(i) + " is a null pointer");
    // the scratch both kernels borrow, checked before any work: the sums' partials go where the evaluation's do, the deferred
    // evaluation's (EVAL_MAX_BATCH tables per launch) into the commit scratch
    const unsigned n = s->cfg.n_vars, batch = s->cfg.batch_size;
    if (pkw::wsum_partial_fes(batch, n) > pkw::eval_partial_fes(batch, n) || pkw::eval_partial_fes(pkw::EVAL_MAX_BATCH, n) > s->plan.scratch)
        return pkw::fail(s, PK_ERR_BAD_ARG, "this config's arena is too small for a linear opening");
    return pkw::open_checked(s, com, st, evals_out, sums_out, proof_out, cap, len);
}

// provekit_whir_sparse.h: pkw_open_linear's counts, pattern and bytes; the lists are validated here, once (the 8 bytes the pass reports
// through are the arena's first: an opening starts from its front afterwards)
int pkw_open_sparse(pkw_scheme* s, const pkw_commitment* com, const uint64_t* points, unsigned q, const uint64_t* offsets, const uint32_t* d_index,
                    const uint64_t* d_value, const uint64_t* tags, unsigned l, uint64_t* evals_out, uint64_t* sums_out, uint8_t* proof_out, size_t cap,
                    size_t* len) {
    if (!s) return PK_ERR_BAD_ARG;
    std::string why;
    if (!pkw::linear_counts_ok(q, l, why)) return pkw::fail(s, PK_ERR_BAD_ARG, why);
    const pkw::SparseWeights w{offsets, d_index, d_value, l};
    const pkw::Statement st{points, q, tags, l, nullptr, &w};
    if (int rc = pkw::open_refused(s, com, st, proof_out, cap, len)) return rc;
    if (!offsets) return pkw::fail(s, PK_ERR_BAD_ARG, "null pointer");
    const unsigned n = s->cfg.n_vars, batch = s->cfg.batch_size;
    if (!pkw::sparse_offsets_ok(offsets, l, n, why)) return pkw::fail(s, PK_ERR_BAD_ARG, why);
    if (offsets[l] && (!d_index || !d_value)) return pkw::fail(s, PK_ERR_BAD_ARG, "null index or value list");
    if (pkw::sparse_partial_fes(batch, n) > pkw::eval_partial_fes(batch, n)) return pkw::fail(s, PK_ERR_OOM, "this config's arena is too small for a sparse opening");
    try {
        size_t bad = 0;
        uint32_t at = 0, prev = 0;
        int rc = pk_ctx_sync(s->ctx);  // the lists are the context's work: there before the pass reads them
        if (!rc) rc = pkw::sparse_validate(s->ctx, s->stream, w, n, s->arena, &bad, &at, &prev);
        // the pass and its readback are rank-local: the ranks of a device set exchange what they found and refuse or go on together
        s->err.clear();
        if (rc)
            s->err = std::string("open: ") + pk_last_error(s->ctx);
        else if (bad != ~(size_t)0)
            rc = pkw::fail(s, PK_ERR_BAD_ARG, pkw::sparse_index_reason(w, bad, at, prev, n));
        if ((rc = pkw::exchange(s, rc, nullptr, nullptr))) return rc;
    } catch (...) {
        return pkw::fail(s, PK_ERR_OOM, "out of memory");
    }
    return pkw::open_checked(s, com, st, evals_out, sums_out, proof_out, cap, len);
}

// ---- hiding commitments (include/provekit_whir_hiding.h) ------------------------------------------------------------------------

int pkw_hiding_scheme_create(pk_ctx* ctx, const pk_whir_config* cfg, pkw_scheme** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return pkw::refuse("null pointer");
    std::string why;
    if (!pkw::config_ok(cfg, why) || !pkw::hiding_config_ok(*cfg, why)) return pkw::refuse(why);
    return pkw_scheme_create(ctx, cfg, out);
}

// f^_b = [f_b || mask_b] and g in one temporary block: the lower halves are copies, the rest is hiding.hip's one launch on the scheme's
// stream; then pkw_commit, which keeps its own copies
int pkw_commit_hiding(pkw_scheme* s, const uint64_t* const* d_evals, const uint8_t* rng_seed32, pkw_hiding_commitment** out) {
    if (out) *out = nullptr;
    if (!s) return PK_ERR_BAD_ARG;
    if (!d_evals || !out) return pkw::fail(s, PK_ERR_BAD_ARG, "null pointer");
    std::string why;
    if (!pkw::hiding_config_ok(s->cfg, why)) return pkw::fail(s, PK_ERR_BAD_ARG, "not a hiding scheme: " + why);
    const unsigned polys = s->cfg.batch_size - 1, n = s->cfg.n_vars - 1;
    for (unsigned b = 0; b < polys; b++)
        if (!d_evals[b]) return pkw::fail(s, PK_ERR_BAD_ARG, "null polynomial");
    uint8_t key[32];
    int rc = PK_OK;
    s->err.clear();
    if (rng_seed32) {
        memcpy(key, rng_seed32, 32);
    } else {
        for (size_t got = 0; got < 32 && !rc;) {
            const ssize_t r = getrandom(key + got, 32 - got, 0);
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) rc = pkw::fail(s, PK_ERR_HIP, std::string("getrandom failed: ") + strerror(errno));
            got += r < 0 ? 0 : (size_t)r;
        }
        // a device set commits to ONE batch: every rank draws, rank 0's key is the set's (its block comes first)
        if (s->world > 1) {
            uint8_t all[32 * PK_MAX_RANKS];
            if (s->world > PK_MAX_RANKS) return pkw::fail(s, PK_ERR_BAD_ARG, "more ranks than PK_MAX_RANKS");
            rc = pkw::exchange(s, rc, key, all);
            if (!rc) memcpy(key, all, 32);
            explicit_bzero(all, sizeof all);
        }
        if (rc) {
            explicit_bzero(key, sizeof key);
            return rc;  // every rank alike
        }
    }
    // from here on a failure is this rank's alone: it travels into pkw_commit's exchange (commit_checked), where the ranks leave together
    pkw_hiding_commitment* com = nullptr;
    try {
        com = new pkw_hiding_commitment();
    } catch (...) {
        rc = pkw::fail(s, PK_ERR_OOM, "out of memory");
    }
    const size_t N = (size_t)1 << n;
    uint64_t* block = nullptr;
    if (!rc && (rc = pk_malloc(s->ctx, 32 * (size_t)(polys + 1) * 2 * N, (void**)&block))) s->err = std::string("commit: ") + pk_last_error(s->ctx);
    uint64_t* tables[pkw::HIDING_MAX_POLYS + 1] = {};
    for (unsigned b = 0; b <= polys && block; b++) tables[b] = block + 4 * (size_t)b * 2 * N;
    if (!rc && (rc = pk_ctx_sync(s->ctx)))  // also selects the device; the block is the context's allocation
        s->err = std::string("commit: ") + pk_last_error(s->ctx);
    hipError_t launched = hipSuccess;
    if (!rc && (rc = pkw::hiding_fill_launch(s->stream, tables, polys, n, key, 0, &launched)))
        s->err = std::string("commit: the launch that draws the masks: ") + hipGetErrorString(launched);
    for (unsigned b = 0; b < polys && !rc; b++)
        if ((rc = pk_memcpy_d2d(s->ctx, tables[b], d_evals[b], 32 * N))) s->err = std::string("commit: ") + pk_last_error(s->ctx);
    const hipError_t drawn = hipStreamSynchronize(s->stream);  // whatever failed above, the launch is over before the block goes
    if (!rc && drawn != hipSuccess) {
        rc = PK_ERR_HIP;
        s->err = std::string("commit: the kernel that draws the masks: ") + hipGetErrorString(drawn);
    }
    {  // sets the scheme's error itself, unless the failure is the one handed in
        pkw_commitment* inner = nullptr;
        rc = pkw::commit_checked(s, tables, rc, &inner);
        if (com) com->inner = inner;
    }
    pk_ctx_sync(s->ctx);  // the copies out of the block are done before it goes
    if (block) pk_free(s->ctx, block);
    explicit_bzero(key, sizeof key);
    if (rc) {
        delete com;
        return rc;
    }
    *out = com;
    return PK_OK;
}

int pkw_hiding_commitment_root(const pkw_hiding_commitment* com, uint8_t root[32]) { return com ? pkw_commitment_root(com->inner, root) : PK_ERR_BAD_ARG; }

int pkw_hiding_commitment_destroy(pkw_hiding_commitment* com) {
    if (!com) return PK_OK;
    pkw_commitment_destroy(com->inner);
    delete com;
    return PK_OK;
}

// pkw_open of the extended batch at the points (0, z_i), once
int pkw_open_hiding(pkw_scheme* s, pkw_hiding_commitment* com, const uint64_t* points, unsigned q, uint64_t* evals_out, uint8_t* proof_out, size_t cap,
                    size_t* len) {
    if (!s) return PK_ERR_BAD_ARG;
    if (q < 1 || q > PKW_MAX_POINTS) return pkw::fail(s, PK_ERR_BAD_ARG, "the number of points must be 1..64");
    if (!com) return pkw::fail(s, PK_ERR_BAD_ARG, "null pointer");
    try {
        const unsigned nv = s->cfg.n_vars, batch = s->cfg.batch_size;
        std::vector<uint64_t> ext(4 * (size_t)q * nv), evals(4 * (size_t)batch * q);
        pkw::Statement st{points ? ext.data() : nullptr, q};
        st.hiding = true;
        if (int rc = pkw::open_refused(s, com->inner, st, proof_out, cap, len)) return rc;
        if (com->opened) return pkw::fail(s, PK_ERR_BAD_ARG, "already opened: a hiding commitment is opened once");
        for (unsigned i = 0; i < q; i++)  // (0, z_i): the leading coordinate stays zero
            memcpy(&ext[4 * ((size_t)i * nv + 1)], points + 4 * (size_t)i * (nv - 1), 32 * (size_t)(nv - 1));
        if (int rc = pkw::open_checked(s, com->inner, st, evals.data(), nullptr, proof_out, cap, len)) return rc;
        com->opened = true;
        if (evals_out) memcpy(evals_out, evals.data(), 32 * (size_t)(batch - 1) * q);  // the first B rows: f_b(z_i)
        return PK_OK;
    } catch (...) {
        return pkw::fail(s, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
