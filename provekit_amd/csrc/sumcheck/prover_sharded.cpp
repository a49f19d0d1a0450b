// prover_sharded.cpp -- the prover of include/provekit_sumcheck_sharded.h: one product sumcheck over the ranks of a device set, and
// one rank's slice of a round by itself.  Host code above provekit_hip.h's C ABI, like prover.cpp, whose replicated rounds it shares
// (round.hpp's round_launch); shard.hpp states who owns what.
//
// Failures and collectives.  A rank-local failure before a collective does not return: it becomes the status the rank sends into
// that collective, and every rank leaves with the first non-zero status in rank order.  After the hand-over nothing is collective,
// and a failure returns at once.  A failure OF a collective is the communicator's: the product has poisoned it for every rank.
#include "../prover_transcript.hpp"
#include "lane.hpp"
#include "prover.hpp"

using pk::fe;

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int fail(pks_prover* p, int rc, const std::string& why) {
    p->err = why;
    return rc;
}

unsigned log2_of(size_t v) {
    unsigned k = 0;
    while (((size_t)1 << k) < v) k++;
    return k;
}

// One all-gather of 32 * (k + 1) bytes per rank: k elements (k < XCHG_FES) and the status of the rank's local work so far.
// all: world x k.  Returns the first non-zero status of the set in rank order, else PK_OK
int exchange(pks_prover* p, int status, const fe* mine, unsigned k, std::vector<fe>& all) {
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

// the first rank whose element differs from rank 0's, or 0
unsigned first_differing(const std::vector<fe>& all) {
    for (size_t r = 1; r < all.size(); r++)
        if (memcmp(&all[r], &all[0], 32)) return (unsigned)r;
    return 0;
}

// what the ranks compare at creation: a sponge over the statement's counts and masks, the coefficients absorbed
fe statement_digest(const pks_statement& st) {
    std::string pat = "provekit-hip/sumcheck-sharded/v1/statement/n" + std::to_string(st.n) + "/m" + std::to_string(st.m) + "/tau" + std::to_string(st.has_tau) +
                      "/bind" + std::to_string(st.n_bind) + "/masks";
    for (unsigned t = 0; t < st.T; t++) pat += (t ? "." : "") + std::to_string(st.masks[t]);
    pat.push_back('\0');
    pat += "A" + std::to_string(st.T) + "coefficients";
    pat.push_back('\0');
    pat += "S1digest";
    pk::Transcript tr(pat);
    for (unsigned t = 0; t < st.T; t++) tr.add_scalar(pk::h_load(st.coeffs[t]));
    return tr.challenge_scalar();
}

}  // namespace

extern "C" {

int pkss_prover_create(pk_ctx* ctx, const pks_statement* stmt, pks_prover** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return pks::refuse("null pointer");
    int rank = 0, world = 0, kind = PK_COMM_NONE;
    if (pk_comm_info(ctx, &rank, &world, &kind) != PK_OK || kind == PK_COMM_NONE || world < 2 || rank < 0 || rank >= world)
        return pks::refuse("the context is not in a device set: pks_prover_create proves on a lone context");
    if ((world & (world - 1)) || world > 1 << PKSS_MAX_WORLD_LOG2)
        return pks::refuse("a world of " + std::to_string(world) + " ranks: it must be a power of two, at most " + std::to_string(1 << PKSS_MAX_WORLD_LOG2) +
                           ", for every rank to own whole index bits");
    // collective from here: a rank that refuses its statement says so in the exchange, on the arena of the smallest statement
    std::string why;
    const bool ok = pks::statement_ok(stmt, why);
    try {
        pks_prover* p = new pks_prover();
        p->ctx = ctx;
        p->sharded = true;
        p->rank = (unsigned)rank, p->world = (unsigned)world;
        p->lay = pkss::layout(ok ? stmt->n : 1, ok ? stmt->m : 1, log2_of((size_t)world));
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, 32 * p->lay.total, &base)) {  // nothing to exchange on: the peers' wait ends at pk_comm's deadline
            delete p;
            pks::g_error = "pk_malloc of the arena failed";
            return rc;
        }
        p->arena = (uint64_t*)base;
        fe digest = pk::fe_zero();
        if (ok) {
            p->st = *stmt;
            p->D = pks::degree(*stmt);
            p->pattern = pks::io_pattern(*stmt);
            p->half = (size_t)1 << (stmt->n - 1);
            p->split = pks::eq_split(stmt->n - 1);
            digest = statement_digest(*stmt);
        } else {
            p->err = why;
        }
        std::vector<fe> all;
        int rc = exchange(p, ok ? PK_OK : PK_ERR_BAD_ARG, &digest, 1, all);
        if (!rc)
            if (const unsigned r = first_differing(all))
                rc = fail(p, PK_ERR_BAD_ARG, "the ranks disagree on the statement: rank " + std::to_string(r) + "'s differs from rank 0's");
        if (rc) {
            pks::g_error = p->err;
            pks_prover_destroy(p);
            return rc;
        }
        *out = p;
        pks::g_error.clear();
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pkss_prove(pks_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap,
               size_t* len, uint64_t* point_out, uint64_t* finals_out) {
    if (!p) return PK_ERR_BAD_ARG;
    if (!p->sharded) return fail(p, PK_ERR_BAD_ARG, "a prover of pks_prover_create proves with pks_prove");
    const pks_statement& st = p->st;
    const pkss::Layout& L = p->lay;
    const unsigned n = st.n, m = st.m, D = p->D, S = L.S, g = L.g;
    if (!d_tables || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t need = 32 * pks::proof_elems(st);
    *len = need;
    p->err.clear();
    try {
        const double t_start = now();
        p->profile.assign(n, pkss_round_profile{});
        p->handover_seconds = p->total_seconds = 0;
        uint64_t* const d_scratch = p->arena + 4 * L.scratch;
        uint64_t* const d_eq = p->arena + 4 * L.eq;
        const uint64_t* const d_results = d_scratch + 4 * (size_t)4 * PKS_MAX_GRID;
        auto compact = [&](unsigned j) { return p->arena + 4 * (L.compact + (size_t)j * L.local_half); };
        auto replicated = [&](unsigned j) { return p->arena + 4 * (L.replicated + (size_t)j * L.handover); };

        // ---- agreement: the arguments' checks and the caller's pending work are rank-local; then the absorbed prefix is compared
        int status = pks::check_prove_arguments(st, d_tables, tau_or_null, bind, cap, need, p->err);
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
            digest = tr.peek_challenge();
        }
        const size_t prefix = tr.narg.size();  // the statement's public part: absorbed, not part of the proof
        std::vector<fe> all;
        if (int rc = exchange(p, status, &digest, 1, all)) return rc;
        if (const unsigned r = first_differing(all))
            return fail(p, PK_ERR_BAD_ARG,
                        "the ranks disagree on bind, tau or the coefficients: rank " + std::to_string(r) + "'s differ from rank 0's; nothing was proved");
        if (st.has_tau) {
            pks::eq_split_build(p->split, tau.data() + 1, p->eq_host);
            if (hipMemcpy(d_eq, p->eq_host.data(), 32 * p->eq_host.size(), hipMemcpyHostToDevice) != hipSuccess)
                status = fail(p, PK_ERR_HIP, "copying the eq tables failed");
        }
        if (status && !S) return status;  // no collective follows

        pks::RoundTables rt{};
        std::vector<fe> point(n);
        fe h[PKS_MAX_TERM_TABLES + 1];
        for (unsigned i = 0; i < n; i++) {
            const size_t pairs = (size_t)1 << (n - 1 - i);
            const uint64_t* const fold = i ? (const uint64_t*)point[i - 1].v : nullptr;
            size_t hi = 0, lo = 0;
            unsigned lo_bits = 0;
            p->split.round(i, hi, lo, lo_bits);
            const uint64_t *d_hi = st.has_tau ? d_eq + 4 * hi : nullptr, *d_lo = st.has_tau ? d_eq + 4 * lo : nullptr;
            pkss_round_profile& prof = p->profile[i];
            double t0 = now();
            if (pkss::round_is_sharded(n, i, g)) {
                // the rank's slice: rounds 0 and 1 read the caller's tables at its own indices, round 1 stores compacted, later rounds
                // fold the compacted arena in place; the sums and the status travel in one all-gather and every rank adds the G blocks
                const size_t mine = pairs >> g;
                for (unsigned j = 0; j < m; j++) {
                    rt.in[j] = i <= 1 ? d_tables[j] : compact(j);
                    rt.out[j] = i == 0 ? nullptr : compact(j);
                }
                if (!status && (status = pks::round_shard_launch(nullptr, st, rt, mine, fold, d_hi, d_lo, lo_bits, pks::round_grid(mine), d_scratch,
                                                                 pks::ShardSlice{g, p->rank, i <= 1})))
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
                    if (int rc2 = pks::handover_launch(nullptr, recv, m, g, replicated(0), L.handover)) return fail(p, rc2, "the hand-over kernel's launch failed");
                    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(p, PK_ERR_HIP, "the hand-over kernel failed");
                    p->handover_seconds = now() - t0;
                    t0 = now();
                }
                // a replicated round: the lone prover's, on the replicated tables (the caller's in rounds 0 and 1 when nothing was stored)
                const bool stored = S >= 2;
                for (unsigned j = 0; j < m; j++) {
                    rt.in[j] = !stored && i <= 1 ? d_tables[j] : replicated(j);
                    rt.out[j] = i == 0 ? nullptr : replicated(j);
                }
                if (int rc = pks::round_launch(nullptr, st, rt, pairs, fold, d_hi, d_lo, lo_bits, pks::round_grid(pairs), d_scratch))
                    return fail(p, rc, "the round kernel's launch failed");
                if (hipMemcpy(h, d_results, 32 * (size_t)(D + 1), hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "a round's results did not arrive");
                prof.pairs = pairs, prof.round_seconds = now() - t0;
            }
            if (i == 0) tr.add_scalar(pks::sum_from_round0(h, st.has_tau ? &tau[0] : nullptr));
            tr.add_scalars(h, D + 1);
            point[i] = tr.challenge_scalar();
        }
        // the last round is replicated (n - S >= 1): the tables' two entries are on every rank -- the caller's own for n = 1
        std::vector<fe> finals(m);
        for (unsigned j = 0; j < m; j++) {
            fe pair[2];
            const uint64_t* src = n == 1 ? d_tables[j] : replicated(j);
            if (hipMemcpy(pair, src, 64, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the last tables did not arrive");
            finals[j] = pks::fold_pair(pair[0], pair[1], point[n - 1]);
        }
        tr.add_scalars(finals.data(), m);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());
        if (tr.narg.size() - prefix != need) return fail(p, PK_ERR_IO_PATTERN, "the proof is not of its declared length");
        memcpy(proof_out, tr.narg.data() + prefix, need);
        if (point_out) memcpy(point_out, point.data(), 32 * (size_t)n);
        if (finals_out) memcpy(finals_out, finals.data(), 32 * (size_t)m);
        p->total_seconds = now() - t_start;
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkss_last_profile(const pks_prover* p, pkss_round_profile* rounds, unsigned cap, double* handover_seconds, double* total_seconds) {
    if (!p || !p->sharded || (!rounds && cap)) return PK_ERR_BAD_ARG;
    for (unsigned i = 0; i < cap && i < p->profile.size(); i++) rounds[i] = p->profile[i];
    if (handover_seconds) *handover_seconds = p->handover_seconds;
    if (total_seconds) *total_seconds = p->total_seconds;
    return PK_OK;
}

int pkss_round_shard(pk_ctx* ctx, const pks_statement* stmt, const uint64_t* const* d_tables, size_t len, const uint64_t* tau_rest_or_null,
                     const uint64_t* fold_or_null, uint64_t* const* d_out_local, unsigned world, unsigned rank, unsigned grid, uint64_t* out) {
    if (!ctx || !d_tables || !out) return pks::refuse("null pointer");
    struct pkss_plan plan;
    if (int rc = pkss_plan(stmt, world, &plan)) return rc;  // the statement's and the world's refusals
    if (rank >= world) return pks::refuse("rank must be below world");
    const size_t round_len = fold_or_null ? len / 2 : len;
    if ((len & (len - 1)) || len > ((size_t)1 << stmt->n) || round_len < pkss::handover_len(plan.g))
        return pks::refuse("len must be a power of two, at most 2^n, and the round's length at least 2^(c+g+1) = " + std::to_string(pkss::handover_len(plan.g)) +
                           ": a shorter round is not sharded");
    if (grid > PKS_MAX_GRID) return pks::refuse("grid must be 0..1024");
    if (fold_or_null && !d_out_local) return pks::refuse("a fold needs output tables");
    const size_t pairs = round_len / 2, mine = pairs >> plan.g;
    const unsigned R = log2_of(pairs);
    if ((fold_or_null && !pk::is_canonical(pk::h_load(fold_or_null))) || (tau_rest_or_null && !pks::elements_below_p(tau_rest_or_null, R)))
        return pks::refuse("a fold or tau element is not below p");
    pks::RoundTables rt{};
    for (unsigned j = 0; j < stmt->m; j++) {
        if (!d_tables[j] || (fold_or_null && !d_out_local[j])) return pks::refuse("null table");
        rt.in[j] = d_tables[j];
        rt.out[j] = fold_or_null ? d_out_local[j] : nullptr;
    }
    try {
        const pks::EqSplit split = pks::eq_split(R);
        std::vector<fe> eq;
        if (tau_rest_or_null) {
            std::vector<fe> t(R);
            for (unsigned i = 0; i < R; i++) t[i] = pk::h_load(tau_rest_or_null + 4 * i);
            pks::eq_split_build(split, t.data(), eq);
        }
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, 32 * (pks::ROUND_SCRATCH_FES + split.fes()), &base)) return rc;
        uint64_t* const d_scratch = (uint64_t*)base;
        uint64_t* const d_eq = d_scratch + 4 * pks::ROUND_SCRATCH_FES;
        size_t hi = 0, lo = 0;
        unsigned lo_bits = 0;
        split.round(0, hi, lo, lo_bits);
        int rc = pk_ctx_sync(ctx);
        if (!rc && tau_rest_or_null && hipMemcpy(d_eq, eq.data(), 32 * eq.size(), hipMemcpyHostToDevice) != hipSuccess) rc = PK_ERR_HIP;
        if (!rc)
            rc = pks::round_shard_launch(nullptr, *stmt, rt, mine, fold_or_null, tau_rest_or_null ? d_eq + 4 * hi : nullptr,
                                         tau_rest_or_null ? d_eq + 4 * lo : nullptr, lo_bits, grid ? grid : pks::round_grid(mine), d_scratch,
                                         pks::ShardSlice{plan.g, rank, true});
        if (!rc && hipMemcpy(out, d_scratch + 4 * (size_t)4 * PKS_MAX_GRID, 32 * (size_t)(pks::degree(*stmt) + 1), hipMemcpyDeviceToHost) != hipSuccess) rc = PK_ERR_HIP;
        pk_free(ctx, base);
        return rc;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
