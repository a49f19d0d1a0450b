// prover.cpp -- the device half of libprovekit_tuplelookup.so's C ABI: the prover (its arena, the launches of tuple.hip, the prover
// side of the outer transcript, the two pkf proofs and the comparison of their fractions), the multiplicities and the leaves by
// themselves.  Host code; of other libraries it calls what provekit_hip.h and provekit_fracsum.h declare.
#include "prover.hpp"

#include <algorithm>
#include <array>

using pk::fail;
using pk::fe;
using pk::host_ms_since;

namespace {

using pk::is_zero;

// the caller's c * w (or w) device pointers into the kernels' argument; false: one is NULL
bool take_columns(const uint64_t* const* d_cols, unsigned w, unsigned c, pkt::Columns& out) {
    for (unsigned g = 0; g < c; g++)
        for (unsigned j = 0; j < w; j++)
            if (!(out.col[g][j] = d_cols[g * w + j])) return false;
    return true;
}

// Why the two fractions differ, from the two leaf tables as they stand.  Equal rows compress to equal leaves, so a leaf of F that is
// no leaf of T is a row outside t for certain; when every leaf of F is one of T the rows are in t (up to a collision in beta) and the
// numerators are what is wrong.  Host work on the failure path only: T's leaves sorted, F's searched chunk by chunk.
std::string why_unequal(pkt_prover* p) {
    using Leaf = std::array<uint64_t, 4>;
    try {
        const size_t size = (size_t)1 << p->st.k, rows = (size_t)1 << pkt::stacked_vars(p->st), chunk = std::min<size_t>(rows, (size_t)1 << 16);
        std::vector<Leaf> table(size), part(chunk);
        if (hipMemcpy(table.data(), p->leaf(PKT_SIDE_T), 32 * size, hipMemcpyDeviceToHost) != hipSuccess) throw 0;
        std::sort(table.begin(), table.end());
        for (size_t at = 0; at < rows; at += chunk) {
            if (hipMemcpy(part.data(), p->leaf(PKT_SIDE_F) + 4 * at, 32 * chunk, hipMemcpyDeviceToHost) != hipSuccess) throw 0;
            for (size_t i = 0; i < chunk; i++)
                if (!std::binary_search(table.begin(), table.end(), part[i]))
                    return "the two sides' fractions differ: a row is not in t: stacked index " + std::to_string(at + i) + " (group " +
                           std::to_string((at + i) >> p->st.n) + ", row " + std::to_string((at + i) & (((size_t)1 << p->st.n) - 1)) + ")";
        }
        return "the two sides' fractions differ: m is wrong: every row is in t, m is not the rows' multiplicities";
    } catch (...) {
        return "the two sides' fractions differ: a row is not in t or m is wrong (the leaves could not be read back to tell which)";
    }
}

}  // namespace

extern "C" {

int pkt_prover_arena_bytes(const pkt_statement* stmt, size_t* bytes) {
    std::string why;
    if (!bytes) return pkt::refuse("null pointer");
    if (!pkt::statement_ok(stmt, why)) return pkt::refuse(why);
    const pkf_statement sides[2] = {pkt::side_f(*stmt), pkt::side_t(*stmt)};
    size_t total = pkt::layout(*stmt).total;
    for (const pkf_statement& s : sides) {
        size_t inner = 0;
        if (int rc = pkf_prover_arena_bytes(&s, &inner)) return pkt::g_error = std::string("pkf_prover_arena_bytes failed: ") + pkf_create_error(), rc;
        total += inner;
    }
    *bytes = total;
    return PK_OK;
}

int pkt_prover_create(pk_ctx* ctx, const pkt_statement* stmt, pkt_prover** out) {
    auto stop = [](int rc, const std::string& reason) { return pkt::g_error = reason, rc; };
    return pk::create<pkt::Lib>(ctx, stmt, out, [&](std::unique_ptr<pkt_prover>& p) {
        p.reset(new pkt_prover());  // its destructor gives back what a return or a throw below leaves behind
        p->ctx = ctx;
        p->st = *stmt;
        p->pattern = pkt::io_pattern(*stmt);
        p->at = pkt::layout(*stmt);
        void* base = nullptr;
        if (int rc = pk_malloc(ctx, p->at.total, &base)) return stop(rc, "pk_malloc of the arena failed");
        p->arena = (uint8_t*)base;
        for (hipEvent_t& e : p->ev)
            if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
        const pkf_statement sides[2] = {pkt::side_f(*stmt), pkt::side_t(*stmt)};
        for (int which = 0; which < 2; which++) {
            if (int rc = pkf_prover_create(ctx, &sides[which], &p->side[which])) return stop(rc, std::string("pkf_prover_create failed: ") + pkf_create_error());
            if (int rc = pkf_proof_bytes(&sides[which], &p->side_bytes[which])) return stop(rc, std::string("pkf_proof_bytes failed: ") + pkf_create_error());
        }
        p->staging.resize(p->side_bytes[0] + p->side_bytes[1]);
        return PK_OK;
    });
}

int pkt_prover_destroy(pkt_prover* p) { return pk::destroy(p); }

const char* pkt_last_error(const pkt_prover* p) { return p ? p->err.c_str() : "null prover"; }

int pkt_multiplicities(pkt_prover* p, const uint64_t* const* d_f, const uint64_t* const* d_t, const uint32_t* const* d_idx, uint64_t* d_m_out, uint64_t* first_bad) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkt_statement& st = p->st;
    if (first_bad) *first_bad = UINT64_MAX;
    if (!d_f || !d_t || !d_idx || !d_m_out) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    try {
        pkt::Columns f{};
        const uint64_t* t[PKT_MAX_WIDTH] = {};
        if (!take_columns(d_f, st.w, st.c, f)) return fail(p, PK_ERR_BAD_ARG, "a column of f is NULL");
        for (unsigned j = 0; j < st.w; j++)
            if (!(t[j] = d_t[j])) return fail(p, PK_ERR_BAD_ARG, "a column of t is NULL");
        for (unsigned g = 0; g < st.c; g++)
            if (!(f.idx[g] = d_idx[g])) return fail(p, PK_ERR_BAD_ARG, "an index column is NULL");
        // the caller's work on the context is finished before anything here reads its tables; the library's own launches go to the null stream
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkt::count_launch(nullptr, st.n, st.k, st.w, st.c, f, t, p->counts(), p->bad(), d_m_out, p->grid)) return fail(p, rc, "the count kernels' launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);
        unsigned long long bad = 0;
        if (hipMemcpy(&bad, p->bad(), 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(p, PK_ERR_HIP, "the first bad row did not arrive");
        p->prof.count_ms = pk::between(p->ev[0], p->ev[1]);
        if (bad != ~0ull) {
            if (first_bad) *first_bad = bad;
            return fail(p, PK_ERR_UNSATISFIED, "stacked index " + std::to_string(bad) + " (group " + std::to_string(bad >> st.n) + ", row " +
                                                   std::to_string(bad & ((1ull << st.n) - 1)) + "): its index is outside t or its row is not the row of t it names");
        }
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

int pkt_leaves(pk_ctx* ctx, unsigned n, unsigned w, unsigned c, const uint64_t* const* d_cols, const uint64_t* alpha, const uint64_t* beta, uint64_t* d_leaf_out) {
    if (!ctx || !d_cols || !alpha || !beta || !d_leaf_out) return pkt::refuse("null pointer");
    if (n < 1 || n > PKT_MAX_VARS) return pkt::refuse("n must be 1..28");
    if (w < 1 || w > PKT_MAX_WIDTH) return pkt::refuse("w must be 1..4");
    if (!pkt::groups_ok(c)) return pkt::refuse("c must be 1, 2 or 4");
    std::string why;
    if (!pkt::elements_below_p(alpha, 1, "alpha", why) || !pkt::elements_below_p(beta, 1, "beta", why)) return pkt::refuse(why);
    pkt::Columns cols{};
    if (!take_columns(d_cols, w, c, cols)) return pkt::refuse("a column is NULL");
    if (int rc = pk_ctx_sync(ctx)) return pkt::g_error = "pk_ctx_sync failed", rc;
    if (int rc = pkt::leaf_launch(nullptr, n, w, c, cols, alpha, beta, d_leaf_out, 0)) return pkt::g_error = "the leaf kernel's launch failed", rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return pkt::g_error = "the leaf kernel failed", PK_ERR_HIP;
    return PK_OK;
}

int pkt_prove(pkt_prover* p, const uint64_t* const* d_f, const uint64_t* const* d_t, const uint64_t* d_m, const uint64_t* bind, uint8_t* proof_out, size_t cap,
              size_t* len, pkt_claims* claims_out) {
    if (!p) return PK_ERR_BAD_ARG;
    const pkt_statement& st = p->st;
    if (!d_f || !d_t || !d_m || !len || (!proof_out && cap)) return fail(p, PK_ERR_BAD_ARG, "null pointer");
    const size_t len_f = p->side_bytes[PKT_SIDE_F], need = len_f + p->side_bytes[PKT_SIDE_T];
    if (int rc = pk::proof_room_and_bind(p, need, cap, len, bind, st.n_bind)) return rc;
    try {
        pkt::Columns f{}, t{};
        if (!take_columns(d_f, st.w, st.c, f)) return fail(p, PK_ERR_BAD_ARG, "a column of f is NULL");
        if (!take_columns(d_t, st.w, 1, t)) return fail(p, PK_ERR_BAD_ARG, "a column of t is NULL");
        pk::Transcript tr(p->pattern);
        for (unsigned i = 0; i < st.n_bind; i++) tr.add_scalar(pk::h_load(bind + 4 * i));
        pkt::Challenges ch;
        ch.alpha = tr.challenge_scalar();
        ch.beta = st.w > 1 ? tr.challenge_scalar() : pk::fe_one();
        tr.challenge_scalars(ch.seeds, 2);
        if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());

        // both leaf tables first: each has its own part of the arena, so both stand while the fractions are compared
        if (int rc = pk_ctx_sync(p->ctx)) return fail(p, rc, "pk_ctx_sync failed");
        (void)hipEventRecord(p->ev[0], nullptr);
        if (int rc = pkt::leaf_launch(nullptr, st.n, st.w, st.c, f, (const uint64_t*)ch.alpha.v, (const uint64_t*)ch.beta.v, p->leaf(PKT_SIDE_F), p->grid))
            return fail(p, rc, "side F's leaf launch failed");
        if (int rc = pkt::leaf_launch(nullptr, st.k, st.w, 1, t, (const uint64_t*)ch.alpha.v, (const uint64_t*)ch.beta.v, p->leaf(PKT_SIDE_T), p->grid))
            return fail(p, rc, "side T's leaf launch failed");
        (void)hipEventRecord(p->ev[1], nullptr);

        // both sides into the staging: pkf's own launches follow the leaves on the null stream.  Nothing of proof_out is written yet
        fe frac[2][2], z[2][PKT_MAX_VARS], cq[2], cp;
        for (int which = PKT_SIDE_F; which <= PKT_SIDE_T; which++) {
            const bool F = which == PKT_SIDE_F;
            size_t part = 0;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = pkf_prove(p->side[which], F ? nullptr : d_m, p->leaf(which), (const uint64_t*)ch.seeds[which].v, p->staging.data() + (F ? 0 : len_f),
                                     p->side_bytes[which], &part, (uint64_t*)frac[which], (uint64_t*)z[which], F ? nullptr : (uint64_t*)cp.v, (uint64_t*)cq[which].v);
            p->prof.side_ms[which] = host_ms_since(t0);
            if (rc == PK_ERR_UNSATISFIED)
                return fail(p, rc, std::string("a denominator is zero: alpha is a compressed row of ") + (F ? "f" : "t"));
            if (rc) return fail(p, rc, std::string("side ") + (F ? "F" : "T") + "'s fractional sum failed: " + pkf_last_error(p->side[which]));
        }
        p->prof.leaf_ms = pk::between(p->ev[0], p->ev[1]);  // pkf_prove is blocking: both events have completed
        if (is_zero(frac[0][1]) || is_zero(frac[1][1])) return fail(p, PK_ERR_UNSATISFIED, "a denominator is zero: alpha is a compressed row");
        if (!pkt::same_fraction(frac[0][0], frac[0][1], frac[1][0], frac[1][1])) return fail(p, PK_ERR_UNSATISFIED, why_unequal(p));
        memcpy(proof_out, p->staging.data(), need);
        if (claims_out) pkt::fill_claims(st, ch, z[0], cq[0], z[1], cp, cq[1], claims_out);
        p->err.clear();
        return PK_OK;
    } catch (...) {
        return fail(p, PK_ERR_OOM, "out of memory");
    }
}

}  // extern "C"
