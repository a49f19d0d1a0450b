// prover.cpp -- the device half of libprovekit_sumcheck.so's C ABI: the prover (one arena, the round loop over round.hip, the
// prover side of the transcript) and the round by itself, each written once for a lone context and for a rank of a device set; and
// the lone entry points (prover_sharded.cpp has the device set's), pks_* and the wide statements' pksw_*: the round loop and the round by
// itself are templates over the statement, and only the launch differs (round.hip, wide.hip).  Host code; of the product library it
// calls what provekit_hip.h declares.
//
// A lone prover is a device set of one: no round is sharded, and its exchange is the rank's own status and values.
//
// Failures and collectives.  A rank-local failure before a collective does not return: it becomes the status the rank sends into
// that collective, and every rank leaves with the first non-zero status in rank order -- a lone prover at once.  After the hand-over
// nothing is collective, and a failure returns at once.  A failure OF a collective is the communicator's: the product has poisoned
// it for every rank.
#include <chrono>

#include "../prover_transcript.hpp"
#include "lane.hpp"
#include "prover.hpp"

using pk::fail;
using pk::fe;

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
int hip_rc(hipError_t e) { return e == hipSuccess ? PK_OK : PK_ERR_HIP; }

}  // namespace

namespace pks {

namespace {

// what a prover holds of its statement, either kind (stmt null: of the smallest one), and its arena.  The reason of a failure goes to `slot`
template <class S>
int equip(pks_prover* p, pk_ctx* ctx, const S* stmt, unsigned rank, unsigned world, std::string& slot) {
    p->ctx = ctx;
    p->rank = rank, p->world = world;
    unsigned g = 0;
    while ((1u << g) < world) g++;
    p->lay = pkss::layout(stmt ? stmt->n : 1, stmt ? stmt->m : 1, g, scratch_fes(S{}));
    if (stmt) {
        p->D = degree(*stmt);
        p->pattern = io_pattern(*stmt);
        p->split = eq_split(stmt->n - 1);
    }
    void* base = nullptr;
    if (int rc = pk_malloc(ctx, 32 * p->lay.total, &base)) return slot = "pk_malloc of the arena failed", rc;
    p->arena = (uint64_t*)base;
    return PK_OK;
}

}  // namespace

int make_prover(pk_ctx* ctx, const pks_statement* stmt, unsigned rank, unsigned world, std::unique_ptr<pks_prover>& out) {
    std::unique_ptr<pks_prover> p(new pks_prover());  // its destructor gives back what a return or a throw below leaves behind
    if (stmt) p->st = *stmt;
    if (int rc = equip(p.get(), ctx, stmt, rank, world, g_error)) return rc;
    out = std::move(p);
    return PK_OK;
}

int exchange(pks_prover* p, int status, const fe* mine, unsigned k, std::vector<fe>& all) {
    if (p->world == 1) return all.assign(mine, mine + k), status;
    const pkss::Layout& L = p->lay;
    uint64_t block[4 * pkss::XCHG_FES] = {};
    memcpy(block, mine, 32 * (size_t)k);
    block[4 * k] = (uint64_t)(int64_t)status;
    const size_t per = 4 * ((size_t)k + 1);
    std::vector<uint64_t> got(per * p->world);
    uint64_t *send = p->arena + 4 * L.xchg_send, *recv = p->arena + 4 * L.xchg_recv;
    int rc = pk_memcpy_h2d(p->ctx, send, block, 8 * per);
    if (!rc) rc = pk_comm_all_gather(p->ctx, send, recv, 8 * per);
    if (!rc) rc = pk_memcpy_d2h(p->ctx, got.data(), recv, 8 * per * p->world);
    if (rc) return fail(p, rc, std::string("exchange between the ranks: ") + pk_last_error(p->ctx));
    for (unsigned r = 0; r < p->world; r++)
        if (const int theirs = (int)(int64_t)got[per * r + 4 * k]) {
            if (!status) p->err = "rank " + std::to_string(r) + " of the device set failed with status " + std::to_string(theirs);  // else: its own reason
            return theirs;
        }
    all.resize((size_t)p->world * k);
    for (unsigned r = 0; r < p->world; r++) memcpy(&all[(size_t)r * k], &got[per * r], 32 * (size_t)k);
    return PK_OK;
}

unsigned first_differing(const std::vector<fe>& all) {
    for (size_t r = 1; r < all.size(); r++)
        if (memcmp(&all[r], &all[0], 32)) return (unsigned)r;
    return 0;
}

namespace {

// the one round loop, of either statement: only the launch differs (round.hip's for a pks_statement, wide.hip's for a pksw_statement,
// which is never sharded)
template <class Stmt>
int prove_any(pks_prover* p, const Stmt& st, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap,
              size_t* len, uint64_t* point_out, uint64_t* finals_out) {
    const pkss::Layout& L = p->lay;
    const unsigned n = st.n, m = st.m, D = p->D, S = L.S, g = L.g;
    if (!d_tables || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t need = 32 * proof_elems(st);
    *len = need;
    p->err.clear();
    try {
        // the profile is a device set's (pkss_last_profile refuses a lone prover): a lone proof neither fills it nor reads the clock
        const bool profiled = p->world > 1;
        auto clock = [&] { return profiled ? now() : 0.0; };
        const double t_start = clock();
        if (profiled) p->profile.assign(n, pkss_round_profile{});
        p->handover_seconds = p->total_seconds = 0;
        uint64_t* const d_scratch = p->arena + 4 * L.scratch;
        uint64_t* const d_eq = p->arena + 4 * L.eq;
        const uint64_t* const d_results = d_scratch + 4 * results_at(st);
        auto compact = [&](unsigned j) { return p->arena + 4 * (L.compact + (size_t)j * L.local_half); };
        auto replicated = [&](unsigned j) { return p->arena + 4 * (L.replicated + (size_t)j * L.handover); };

        // ---- agreement: the arguments' checks and the caller's pending work are rank-local; then the absorbed prefix is compared
        int status = check_prove_arguments(st, d_tables, tau_or_null, bind, cap, need, p->err);
        if (!status && (status = pk_ctx_sync(p->ctx))) fail(p, status, "pk_ctx_sync failed");
        pk::Transcript tr(p->pattern);
        std::vector<fe> tau(n);
        fe digest = pk::fe_zero();
        if (!status) {
            for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
            if (st.has_tau) {
                for (unsigned i = 0; i < n; i++) tau[i] = pk::h_load(tau_or_null + 4 * i);
                tr.add_scalars(tau.data(), n);
            }
            for (unsigned t = 0; t < st.T; t++) tr.add_scalar(pk::h_load(st.coeffs[t]));
            if (p->world > 1) digest = tr.peek_challenge();
        }
        const size_t prefix = tr.narg.size();  // the statement's public part: absorbed, not part of the proof
        std::vector<fe> all;
        if (int rc = exchange(p, status, &digest, 1, all)) return rc;
        if (const unsigned r = first_differing(all))
            return fail(p, PK_ERR_BAD_ARG,
                        "the ranks disagree on bind, tau or the coefficients: rank " + std::to_string(r) + "'s differ from rank 0's; nothing was proved");
        if (st.has_tau) {
            eq_split_build(p->split, tau.data() + 1, p->eq_host);
            if (hipMemcpy(d_eq, p->eq_host.data(), 32 * p->eq_host.size(), hipMemcpyHostToDevice) != hipSuccess)
                status = fail(p, PK_ERR_HIP, "copying the eq tables failed");
        }
        if (status && !S) return status;  // no collective follows

        RoundTables rt{};
        std::vector<fe> point(n);
        fe h[MAX_ROUND_VALUES];
        for (unsigned i = 0; i < n; i++) {
            // round i: pairs of the tables at length 2^(n-i); from round 1 on they are folded by r_{i-1} on the way, into the arena
            const size_t pairs = (size_t)1 << (n - 1 - i);
            const uint64_t* const fold = i ? (const uint64_t*)point[i - 1].v : nullptr;
            size_t hi = 0, lo = 0;
            unsigned lo_bits = 0;
            p->split.round(i, hi, lo, lo_bits);
            const uint64_t *d_hi = st.has_tau ? d_eq + 4 * hi : nullptr, *d_lo = st.has_tau ? d_eq + 4 * lo : nullptr;
            pkss_round_profile unread{};
            pkss_round_profile& prof = profiled ? p->profile[i] : unread;
            double t0 = clock();
            if (i < S) {
                // the rank's slice: rounds 0 and 1 read the caller's tables at its own indices, round 1 stores compacted, later rounds
                // fold the compacted arena in place; the sums and the status travel in one all-gather and every rank adds the G blocks
                const size_t mine = pairs >> g;
                for (unsigned j = 0; j < m; j++) {
                    rt.in[j] = i <= 1 ? d_tables[j] : compact(j);
                    rt.out[j] = i == 0 ? nullptr : compact(j);
                }
                if (!status &&
                    (status = round_shard_launch(nullptr, st, rt, mine, fold, d_hi, d_lo, lo_bits, round_grid(mine), d_scratch, ShardSlice{g, p->rank, i <= 1})))
                    fail(p, status, "the sharded round kernel's launch failed");
                if (!status && hipMemcpy(h, d_results, 32 * (size_t)(D + 1), hipMemcpyDeviceToHost) != hipSuccess)
                    status = fail(p, PK_ERR_HIP, "a round's results did not arrive");
                prof.sharded = 1, prof.pairs = mine, prof.round_seconds = now() - t0;
                t0 = now();
                if (int rc = exchange(p, status, h, D + 1, all)) return rc;
                prof.exchange_seconds = now() - t0;
                for (unsigned k = 0; k <= D; k++) {
                    h[k] = all[k];
                    for (unsigned r = 1; r < p->world; r++) h[k] = pk::h_add(h[k], all[(size_t)r * (D + 1) + k]);
                }
            } else {
                if (i == S && S >= 2) {
                    // the hand-over: every rank's two chunks of each table, gathered and put into global order on every rank
                    uint64_t *send = p->arena + 4 * L.gather_send, *recv = p->arena + 4 * L.gather_recv;
                    const size_t row = (size_t)32 << (pkss::C + 1);
                    if (hipMemcpy2DAsync(send, row, compact(0), 32 * L.local_half, row, m, hipMemcpyDeviceToDevice, nullptr) != hipSuccess ||
                        hipStreamSynchronize(nullptr) != hipSuccess)
                        status = fail(p, PK_ERR_HIP, "packing the hand-over block failed");
                    int rc = pk_comm_all_gather(p->ctx, send, recv, row * m);
                    if (!rc) rc = pk_ctx_sync(p->ctx);
                    if (rc) return fail(p, rc, std::string("the hand-over's gather: ") + pk_last_error(p->ctx));
                    if (status) return status;
                    if (int rc2 = handover_launch(nullptr, recv, m, g, replicated(0), L.handover)) return fail(p, rc2, "the hand-over kernel's launch failed");
                    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(p, PK_ERR_HIP, "the hand-over kernel failed");
                    p->handover_seconds = now() - t0;
                    t0 = now();
                }
                // a replicated round, every round of a lone prover: on the replicated tables (the caller's in rounds 0 and 1 when
                // nothing was stored), folded in place
                const bool stored = S >= 2;
                for (unsigned j = 0; j < m; j++) {
                    rt.in[j] = !stored && i <= 1 ? d_tables[j] : replicated(j);
                    rt.out[j] = i == 0 ? nullptr : replicated(j);
                }
                if (int rc = round_launch(nullptr, st, rt, pairs, fold, d_hi, d_lo, lo_bits, round_grid(pairs), d_scratch))
                    return fail(p, rc, "the round kernel's launch failed");
                if (hipMemcpy(h, d_results, 32 * (size_t)(D + 1), hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "a round's results did not arrive");
                prof.pairs = pairs, prof.round_seconds = clock() - t0;
            }
            if (i == 0) tr.add_scalar(sum_from_round0(h, st.has_tau ? &tau[0] : nullptr));
            tr.add_scalars(h, D + 1);
            point[i] = tr.challenge_scalar();
        }
        // the last round is replicated (n - S >= 1): the tables' two entries are on every rank -- the caller's own for n = 1 -- and the
        // last challenge binds them
        std::vector<fe> finals(m);
        for (unsigned j = 0; j < m; j++) {
            fe pair[2];
            const uint64_t* src = n == 1 ? d_tables[j] : replicated(j);
            if (hipMemcpy(pair, src, 64, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the last tables did not arrive");
            finals[j] = fold_pair(pair[0], pair[1], point[n - 1]);
        }
        tr.add_scalars(finals.data(), m);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());
        if (tr.narg.size() - prefix != need) return fail(p, PK_ERR_IO_PATTERN, "the proof is not of its declared length");
        memcpy(proof_out, tr.narg.data() + prefix, need);
        if (point_out) memcpy(point_out, point.data(), 32 * (size_t)n);
        if (finals_out) memcpy(finals_out, finals.data(), 32 * (size_t)m);
        p->total_seconds = clock() - t_start;
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

// a round by itself, of either statement; a refusal's reason goes to `slot`
template <class S>
int round_any(pk_ctx* ctx, const S& st, std::string& slot, const uint64_t* const* d_tables, uint64_t* const* d_out_tables, size_t pairs, size_t mine,
              const uint64_t* tau_rest_or_null, const uint64_t* fold_or_null, unsigned grid, const ShardSlice* shard, uint64_t* out) {
    auto refuse = [&](const char* why) { return pk::refuse(slot, why); };
    if (grid > PKS_MAX_GRID) return refuse("grid must be 0..1024");
    if (fold_or_null && !d_out_tables) return refuse("a fold needs output tables");
    unsigned R = 0;  // the round's length is 2 * pairs = 2^(R + 1)
    while (((size_t)1 << R) < pairs) R++;
    if ((fold_or_null && !pk::is_canonical(pk::h_load(fold_or_null))) || (tau_rest_or_null && !elements_below_p(tau_rest_or_null, R)))
        return refuse("a fold or tau element is not below p");
    RoundTables rt{};
    for (unsigned j = 0; j < st.m; j++) {
        if (!d_tables[j] || (fold_or_null && !d_out_tables[j])) return refuse("null table");
        rt.in[j] = d_tables[j];
        rt.out[j] = fold_or_null ? d_out_tables[j] : nullptr;
    }
    try {
        const EqSplit split = eq_split(R);
        std::vector<fe> eq;
        if (tau_rest_or_null) {
            std::vector<fe> t(R);
            for (unsigned i = 0; i < R; i++) t[i] = pk::h_load(tau_rest_or_null + 4 * i);
            eq_split_build(split, t.data(), eq);
        }
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, 32 * (scratch_fes(st) + split.fes()), &base)) return rc;
        uint64_t* const d_scratch = (uint64_t*)base;
        uint64_t* const d_eq = d_scratch + 4 * scratch_fes(st);
        size_t hi = 0, lo = 0;
        unsigned lo_bits = 0;
        split.round(0, hi, lo, lo_bits);
        const uint64_t *d_hi = tau_rest_or_null ? d_eq + 4 * hi : nullptr, *d_lo = tau_rest_or_null ? d_eq + 4 * lo : nullptr;
        if (!grid) grid = round_grid(mine);
        int rc = pk_ctx_sync(ctx);
        if (!rc && tau_rest_or_null) rc = hip_rc(hipMemcpy(d_eq, eq.data(), 32 * eq.size(), hipMemcpyHostToDevice));
        if (!rc)
            rc = shard ? round_shard_launch(nullptr, st, rt, mine, fold_or_null, d_hi, d_lo, lo_bits, grid, d_scratch, *shard)
                       : round_launch(nullptr, st, rt, mine, fold_or_null, d_hi, d_lo, lo_bits, grid, d_scratch);
        if (!rc) rc = hip_rc(hipMemcpy(out, d_scratch + 4 * results_at(st), 32 * (size_t)(degree(st) + 1), hipMemcpyDeviceToHost));
        pk_free(ctx, base);
        return rc;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // namespace

int prove(pks_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len,
          uint64_t* point_out, uint64_t* finals_out) {
    return prove_any(p, p->st, d_tables, tau_or_null, bind, proof_out, cap, len, point_out, finals_out);
}

int round_alone(pk_ctx* ctx, const pks_statement& st, const uint64_t* const* d_tables, uint64_t* const* d_out_tables, size_t pairs, size_t mine,
                const uint64_t* tau_rest_or_null, const uint64_t* fold_or_null, unsigned grid, const ShardSlice* shard, uint64_t* out) {
    return round_any(ctx, st, g_error, d_tables, d_out_tables, pairs, mine, tau_rest_or_null, fold_or_null, grid, shard, out);
}

}  // namespace pks

extern "C" {

int pks_prover_create(pk_ctx* ctx, const pks_statement* stmt, pks_prover** out) {
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    try {
        std::unique_ptr<pks_prover> p;
        if (int rc = pks::make_prover(ctx, stmt, 0, 1, p)) return rc;
        *out = p.release();
        pks::g_error.clear();
        return PK_OK;
    } catch (...) {
        return pk::out_of_host_memory(pks::g_error);
    }
}

int pks_prover_destroy(pks_prover* p) {
    if (!p) return PK_OK;
    const int rc = p->give_back();
    delete p;
    return rc;
}

const char* pks_last_error(const pks_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pks_prove(pks_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap,
              size_t* len, uint64_t* point_out, uint64_t* finals_out) {
    if (!p) return PK_ERR_BAD_ARG;
    if (p->world > 1) return pk::fail(p, PK_ERR_BAD_ARG, "a prover of pkss_prover_create proves with pkss_prove");
    return pks::prove(p, d_tables, tau_or_null, bind, proof_out, cap, len, point_out, finals_out);
}

int pks_round(pk_ctx* ctx, const pks_statement* stmt, const uint64_t* const* d_tables, size_t len, const uint64_t* tau_rest_or_null,
              const uint64_t* fold_or_null, uint64_t* const* d_out_tables, unsigned grid, uint64_t* out) {
    std::string why;
    if (!ctx || !d_tables || !out) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    const size_t min_len = fold_or_null ? 4 : 2;
    if (len < min_len || (len & (len - 1)) || len > ((size_t)1 << stmt->n)) return pks::refuse("len must be a power of two, at least 2 (4 with a fold) and at most 2^n");
    const size_t pairs = fold_or_null ? len / 4 : len / 2;
    return pks::round_alone(ctx, *stmt, d_tables, d_out_tables, pairs, pairs, tau_rest_or_null, fold_or_null, grid, nullptr, out);
}

}  // extern "C"

// ---- the wide statements (include/provekit_sumcheck_wide.h): the same prover object, round loop and round by itself ------------------

struct pksw_prover : pks_prover {
    pksw_statement wide{};
};

extern "C" {

int pksw_prover_create(pk_ctx* ctx, const pksw_statement* stmt, pksw_prover** out) {
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return pks::refuse_wide("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse_wide(why);
    try {
        std::unique_ptr<pksw_prover> p(new pksw_prover());
        p->wide = *stmt;
        if (int rc = pks::equip(p.get(), ctx, stmt, 0, 1, pks::g_wide_error)) return rc;
        *out = p.release();
        pks::g_wide_error.clear();
        return PK_OK;
    } catch (...) {
        return pk::out_of_host_memory(pks::g_wide_error);
    }
}

int pksw_prover_destroy(pksw_prover* p) {
    if (!p) return PK_OK;
    const int rc = p->give_back();
    delete p;
    return rc;
}

const char* pksw_last_error(const pksw_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pksw_prove(pksw_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap,
               size_t* len, uint64_t* point_out, uint64_t* finals_out) {
    if (!p) return PK_ERR_BAD_ARG;
    return pks::prove_any(static_cast<pks_prover*>(p), p->wide, d_tables, tau_or_null, bind, proof_out, cap, len, point_out, finals_out);
}

int pksw_round(pk_ctx* ctx, const pksw_statement* stmt, const uint64_t* const* d_tables, size_t len, const uint64_t* tau_rest_or_null,
               const uint64_t* fold_or_null, uint64_t* const* d_out_tables, unsigned grid, uint64_t* out) {
    std::string why;
    if (!ctx || !d_tables || !out) return pks::refuse_wide("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse_wide(why);
    // the split eq weights are tables over the bits of the pair index: a weighted round needs a power of two.  Nothing else does
    const size_t unit = fold_or_null ? 4 : 2;
    if (len < unit || len % unit || len > ((size_t)1 << stmt->n))
        return pks::refuse_wide("len must be a multiple of 2 (of 4 with a fold), at least that and at most 2^n");
    if (tau_rest_or_null && (len & (len - 1))) return pks::refuse_wide("with tau_rest, len must be a power of two");
    const size_t pairs = len / unit;
    return pks::round_any(ctx, *stmt, pks::g_wide_error, d_tables, d_out_tables, pairs, pairs, tau_rest_or_null, fold_or_null, grid, nullptr, out);
}

}  // extern "C"
