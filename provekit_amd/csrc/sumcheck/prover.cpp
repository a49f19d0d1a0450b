// prover.cpp -- the device half of libprovekit_sumcheck.so's C ABI: the prover (one arena, the round loop over round.hip, the
// prover side of the transcript) and the round by itself.  Host code; of the product library it calls what provekit_hip.h declares.
#include <cstdarg>

#include "../prover_transcript.hpp"
#include "lane.hpp"
#include "prover.hpp"

using pk::fe;

namespace {

int fail(pks_prover* p, int rc, const std::string& why) {
    p->err = why;
    return rc;
}
// the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
int hip_rc(hipError_t e) { return e == hipSuccess ? PK_OK : PK_ERR_HIP; }

}  // namespace

extern "C" {

int pks_prover_create(pk_ctx* ctx, const pks_statement* stmt, pks_prover** out) {
    if (out) *out = nullptr;
    std::string why;
    if (!ctx || !out) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    try {
        pks_prover* p = new pks_prover();
        p->ctx = ctx;
        p->st = *stmt;
        p->D = pks::degree(*stmt);
        p->pattern = pks::io_pattern(*stmt);
        p->half = (size_t)1 << (stmt->n - 1);
        p->split = pks::eq_split(stmt->n - 1);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, 32 * pks::lone_arena_fes(stmt->n, stmt->m), &base)) {
            delete p;
            pks::g_error = "pk_malloc of the arena failed";
            return rc;
        }
        p->arena = (uint64_t*)base;
        *out = p;
        pks::g_error.clear();
        return PK_OK;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

int pks_prover_destroy(pks_prover* p) {
    if (!p) return PK_OK;
    const int rc = p->arena ? pk_free(p->ctx, p->arena) : PK_OK;
    delete p;
    return rc;
}

const char* pks_last_error(const pks_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pks_prove(pks_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap,
              size_t* len, uint64_t* point_out, uint64_t* finals_out) {
    if (!p) return PK_ERR_BAD_ARG;
    if (p->sharded) return fail(p, PK_ERR_BAD_ARG, "a prover of pkss_prover_create proves with pkss_prove");
    const pks_statement& st = p->st;
    const unsigned n = st.n, m = st.m, D = p->D;
    if (!d_tables || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t need = 32 * pks::proof_elems(st);
    *len = need;
    if (int rc = pks::check_prove_arguments(st, d_tables, tau_or_null, bind, cap, need, p->err)) return rc;
    try {
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        uint64_t* const d_scratch = p->arena + 4 * (size_t)m * p->half;
        uint64_t* const d_eq = d_scratch + 4 * pks::ROUND_SCRATCH_FES;
        const uint64_t* const d_results = d_scratch + 4 * (size_t)4 * PKS_MAX_GRID;
        std::vector<fe> tau(n);
        if (st.has_tau) {
            for (unsigned i = 0; i < n; i++) tau[i] = pk::h_load(tau_or_null + 4 * i);
            pks::eq_split_build(p->split, tau.data() + 1, p->eq_host);
            if (hipMemcpy(d_eq, p->eq_host.data(), 32 * p->eq_host.size(), hipMemcpyHostToDevice) != hipSuccess)
                return fail(p, PK_ERR_HIP, "copying the eq tables failed");
        }

        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        if (st.has_tau) tr.add_scalars(tau.data(), n);
        for (unsigned t = 0; t < st.T; t++) tr.add_scalar(pk::h_load(st.coeffs[t]));
        const size_t prefix = tr.narg.size();  // the statement's public part: absorbed, not part of the proof

        pks::RoundTables rt{};
        std::vector<fe> point(n);
        fe h[PKS_MAX_TERM_TABLES + 1];
        for (unsigned i = 0; i < n; i++) {
            // round i: pairs of the tables at length 2^(n-i); from round 1 on they are folded by r_{i-1} on the way, into the arena
            const size_t pairs = (size_t)1 << (n - 1 - i);
            for (unsigned j = 0; j < m; j++) {
                rt.in[j] = i <= 1 ? d_tables[j] : p->arena + 4 * (size_t)j * p->half;
                rt.out[j] = i == 0 ? nullptr : p->arena + 4 * (size_t)j * p->half;
            }
            size_t hi = 0, lo = 0;
            unsigned lo_bits = 0;
            p->split.round(i, hi, lo, lo_bits);
            if (int rc = pks::round_launch(nullptr, st, rt, pairs, i ? (const uint64_t*)point[i - 1].v : nullptr, st.has_tau ? d_eq + 4 * hi : nullptr,
                                           st.has_tau ? d_eq + 4 * lo : nullptr, lo_bits, pks::round_grid(pairs), d_scratch))
                return fail(p, rc, "the round kernel's launch failed");
            if (hipMemcpy(h, d_results, 32 * (size_t)(D + 1), hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "a round's results did not arrive");
            if (i == 0) tr.add_scalar(pks::sum_from_round0(h, st.has_tau ? &tau[0] : nullptr));
            tr.add_scalars(h, D + 1);
            point[i] = tr.challenge_scalar();
        }
        // the tables now have two entries each -- the caller's own for n = 1 -- and the last challenge binds them
        std::vector<fe> finals(m);
        for (unsigned j = 0; j < m; j++) {
            fe pair[2];
            const uint64_t* src = n == 1 ? d_tables[j] : p->arena + 4 * (size_t)j * p->half;
            if (hipMemcpy(pair, src, 64, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the last tables did not arrive");
            finals[j] = pks::fold_pair(pair[0], pair[1], point[n - 1]);
        }
        tr.add_scalars(finals.data(), m);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());
        if (tr.narg.size() - prefix != need) return fail(p, PK_ERR_IO_PATTERN, "the proof is not of its declared length");
        memcpy(proof_out, tr.narg.data() + prefix, need);
        if (point_out) memcpy(point_out, point.data(), 32 * (size_t)n);
        if (finals_out) memcpy(finals_out, finals.data(), 32 * (size_t)m);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pks_round(pk_ctx* ctx, const pks_statement* stmt, const uint64_t* const* d_tables, size_t len, const uint64_t* tau_rest_or_null,
              const uint64_t* fold_or_null, uint64_t* const* d_out_tables, unsigned grid, uint64_t* out) {
    std::string why;
    if (!ctx || !d_tables || !out) return pks::refuse("null pointer");
    if (!pks::statement_ok(stmt, why)) return pks::refuse(why);
    const size_t min_len = fold_or_null ? 4 : 2;
    if (len < min_len || (len & (len - 1)) || len > ((size_t)1 << stmt->n)) return pks::refuse("len must be a power of two, at least 2 (4 with a fold) and at most 2^n");
    if (grid > PKS_MAX_GRID) return pks::refuse("grid must be 0..1024");
    if (fold_or_null && !d_out_tables) return pks::refuse("a fold needs output tables");
    const size_t pairs = fold_or_null ? len / 4 : len / 2;
    unsigned R = 0;  // the round's length is 2 * pairs = 2^(R + 1)
    while (((size_t)1 << R) < pairs) R++;
    if ((fold_or_null && !pk::is_canonical(pk::h_load(fold_or_null))) || (tau_rest_or_null && !pks::elements_below_p(tau_rest_or_null, R)))
        return pks::refuse("a fold or tau element is not below p");
    pks::RoundTables rt{};
    for (unsigned j = 0; j < stmt->m; j++) {
        if (!d_tables[j] || (fold_or_null && !d_out_tables[j])) return pks::refuse("null table");
        rt.in[j] = d_tables[j];
        rt.out[j] = fold_or_null ? d_out_tables[j] : nullptr;
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
        if (!rc && tau_rest_or_null) rc = hip_rc(hipMemcpy(d_eq, eq.data(), 32 * eq.size(), hipMemcpyHostToDevice));
        if (!rc)
            rc = pks::round_launch(nullptr, *stmt, rt, pairs, fold_or_null, tau_rest_or_null ? d_eq + 4 * hi : nullptr, tau_rest_or_null ? d_eq + 4 * lo : nullptr,
                                   lo_bits, grid ? grid : pks::round_grid(pairs), d_scratch);
        if (!rc) rc = hip_rc(hipMemcpy(out, d_scratch + 4 * (size_t)4 * PKS_MAX_GRID, 32 * (size_t)(pks::degree(*stmt) + 1), hipMemcpyDeviceToHost));
        pk_free(ctx, base);
        return rc;
    } catch (...) {
        return PK_ERR_OOM;
    }
}

}  // extern "C"
