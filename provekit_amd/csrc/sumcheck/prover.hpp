// prover.hpp -- what prover.cpp (the lone prover) and prover_sharded.cpp (the prover on a device set) share: the prover object and
// the layout of a sharded prover's arena, which pkss_plan reports.  Host only.
#pragma once
#include <string>
#include <vector>

#include "round.hpp"
#include "shard.hpp"

namespace pks {

inline bool elements_below_p(const uint64_t* v, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!pk::is_canonical(pk::h_load(v + 4 * i))) return false;
    return true;
}

// what pks_prove and pkss_prove refuse of their arguments, with the reason
inline int check_prove_arguments(const pks_statement& st, const uint64_t* const* d_tables, const uint64_t* tau, const uint64_t* bind, size_t cap, size_t need,
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

namespace pkss {

// what a rank contributes to the exchange behind a sharded round: up to D + 1 sums, and one element whose first limb is its status
constexpr size_t XCHG_FES = PKS_MAX_TERM_TABLES + 2;

// A sharded prover's arena, in field elements from its start:
//   [compact: m tables of 2^(n-1) / G -- the rank's compacted tables from round 1 on; none with S < 2: nothing sharded is ever stored]
//   [replicated: m tables of 2^(c+g+1) -- the hand-over's global tables, and what the replicated rounds fold in place]
//   [gather: the rank's m x 2^(c+1) hand-over block, then the G gathered ones] [exchange: XCHG_FES, then G x XCHG_FES]
//   [round scratch] [split eq tables of n - 1 coordinates]
struct Layout {
    unsigned g = 0, S = 0;
    size_t local_half = 0, handover = 0;  // the strides of the compact and the replicated tables
    size_t compact = 0, replicated = 0, gather_send = 0, gather_recv = 0, xchg_send = 0, xchg_recv = 0, scratch = 0, eq = 0, total = 0;
};
inline Layout layout(unsigned n, unsigned m, unsigned g) {
    Layout L;
    L.g = g, L.S = sharded_rounds(n, g);
    L.local_half = L.S >= 2 ? ((size_t)1 << (n - 1)) >> g : 0;
    L.handover = handover_len(g);
    const size_t block = (size_t)m << (C + 1), G = (size_t)1 << g;
    L.replicated = L.compact + m * L.local_half;
    L.gather_send = L.replicated + m * L.handover;
    L.gather_recv = L.gather_send + block;
    L.xchg_send = L.gather_recv + G * block;
    L.xchg_recv = L.xchg_send + XCHG_FES;
    L.scratch = L.xchg_recv + G * XCHG_FES;
    L.eq = L.scratch + pks::ROUND_SCRATCH_FES;
    L.total = L.eq + pks::eq_split(n - 1).fes();
    return L;
}

}  // namespace pkss

struct pks_prover {
    pk_ctx* ctx = nullptr;
    pks_statement st{};
    std::string pattern, err;
    unsigned D = 0;
    uint64_t* arena = nullptr;  // lone: [m tables of 2^(n-1)] [round scratch] [split eq tables]; sharded: pkss::Layout
    size_t half = 0;            // 2^(n-1)
    pks::EqSplit split;
    std::vector<pk::fe> eq_host;
    // a prover made by pkss_prover_create
    bool sharded = false;
    unsigned rank = 0, world = 1;
    pkss::Layout lay;
    std::vector<pkss_round_profile> profile;  // of the last proof (pkss_last_profile)
    double handover_seconds = 0, total_seconds = 0;
};
