// prover.hpp -- what prover.cpp (the prover, lone or on a device set, and the lone entry points) and prover_sharded.cpp (the device
// set's entry points) share: the prover object (layout.hpp states its arena).  Host only.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "layout.hpp"

namespace pks {

using pk::elements_below_p;

// what pks_prove, pkss_prove and pksw_prove refuse of their arguments, with the reason
template <class S>
int check_prove_arguments(const S& st, const uint64_t* const* d_tables, const uint64_t* tau, const uint64_t* bind, size_t cap, size_t need,
                                 std::string& why) {
    auto no = [&](const std::string& reason) { return why = reason, PK_ERR_BAD_ARG; };
    if (cap < need) return no("the proof buffer holds " + std::to_string(cap) + " bytes, the proof has " + std::to_string(need));
    for (unsigned j = 0; j < st.m; j++)
        if (!d_tables[j]) return no("null table");
    if (st.has_tau && !tau) return no("the statement has a tau: pass it");
    if (!st.has_tau && tau) return no("the statement has no tau: pass NULL");
    if (st.n_bind && !bind) return no("the statement binds elements: pass them");
    if (!elements_below_p(bind, st.n_bind) || !elements_below_p(tau, st.has_tau ? st.n : 0)) return no("a bind or tau element is not below p");
    return PK_OK;
}

// s from round 0's values: (1 - tau_0) h(0) + tau_0 h(1), or h(0) + h(1)
inline fe sum_from_round0(const fe* h, const fe* tau0) {
    return tau0 ? pk::h_add(h[0], pk::h_mul(*tau0, pk::h_sub(h[1], h[0]))) : pk::h_add(h[0], h[1]);
}

}  // namespace pks

// one statement's prover on a context: lone (pks_prover_create: world 1) or one rank of a device set (pkss_prover_create)
struct pks_prover {
    pk_ctx* ctx = nullptr;
    pks_statement st{};
    std::string pattern, err;
    unsigned D = 0;
    unsigned rank = 0, world = 1;
    pkss::Layout lay;
    uint64_t* arena = nullptr;
    pks::EqSplit split;
    std::vector<pk::fe> eq_host;
    std::vector<pkss_round_profile> profile;  // of the last proof (pkss_last_profile)
    double handover_seconds = 0, total_seconds = 0;

    pks_prover() = default;
    pks_prover(const pks_prover&) = delete;
    pks_prover& operator=(const pks_prover&) = delete;
    // gives the arena back, so a creation that stops half way leaks nothing
    int give_back() {
        const int rc = arena ? pk_free(ctx, arena) : PK_OK;
        arena = nullptr;
        return rc;
    }
    ~pks_prover() { (void)give_back(); }
};

namespace pks {

// prover.cpp, for the two sets of entry points.  A prover on rank `rank` of `world` with its arena: of `stmt`, or, where a rank of a
// device set has refused its statement (stmt null), of the smallest one, for the refusal to travel on.  The reason of a failure goes
// to g_error
int make_prover(pk_ctx* ctx, const pks_statement* stmt, unsigned rank, unsigned world, std::unique_ptr<pks_prover>& out);
// One all-gather of 32 * (k + 1) bytes per rank: k elements (k < XCHG_FES) and the status of the rank's local work so far.
// all: world x k.  Returns the first non-zero status of the set in rank order, else PK_OK.  A lone prover's is its own: no device
// memory is touched, nothing is collective
int exchange(pks_prover* p, int status, const fe* mine, unsigned k, std::vector<fe>& all);
// the first rank whose element differs from rank 0's, or 0
unsigned first_differing(const std::vector<fe>& all);
// pks_prove and pkss_prove
int prove(pks_prover* p, const uint64_t* const* d_tables, const uint64_t* tau_or_null, const uint64_t* bind, uint8_t* proof_out, size_t cap, size_t* len,
          uint64_t* point_out, uint64_t* finals_out);
// pks_round and pkss_round_shard after their own refusals: a round of `pairs` pairs by itself, or with `shard` that rank's `mine` of them
int round_alone(pk_ctx* ctx, const pks_statement& st, const uint64_t* const* d_tables, uint64_t* const* d_out_tables, size_t pairs, size_t mine,
                const uint64_t* tau_rest_or_null, const uint64_t* fold_or_null, unsigned grid, const ShardSlice* shard, uint64_t* out);

}  // namespace pks
