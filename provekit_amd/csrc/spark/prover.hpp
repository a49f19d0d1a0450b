// prover.hpp -- what a pkx_prover holds, for prover.cpp; and for the lab (tools/probes/spark.hip), which sets the grid of a prover's
// kernels and reads where its last calls' time went: test and benchmark knobs that the C ABI does not carry.
#pragma once
#include <memory>
#include <vector>

#include "../prover_transcript.hpp"
#include "../sumcheck/round.hpp"
#include "kernels.hpp"

namespace pkx {

// Where the last calls' time went, in milliseconds: the device time of the last pkx_matrix's two phases and of the last pkx_begin's
// gather (events around them), and the last proof's eq tables and three sides in host time -- two clocks.  What has not run reads 0.
struct Profile {
    double count_ms = 0, columns_ms = 0, gather_ms = 0, eq_ms = 0;
    double side_ms[3] = {};
};

// the pks prover's arena (sumcheck/round.hpp states what pks_prover_create allocates)
inline size_t val_arena_bytes(const pkx_statement& st) { return 32 * pks::lone_arena_fes(st.n, 3); }

}  // namespace pkx

struct pkx_prover {
    pk_ctx* ctx = nullptr;
    pkx_statement st{};
    std::string pattern, err;
    uint8_t* arena = nullptr;  // layout.hpp
    pkx::Layout at;
    pks_prover* val = nullptr;                 // PKX_SIDE_VAL: (n, 3 tables, one term)
    pkt_prover* look[2] = {nullptr, nullptr};  // PKX_SIDE_ROW: (n, s, w = 2), PKX_SIDE_COL: (n, t, w = 2)
    size_t side_bytes[3] = {0, 0, 0};          // the three parts of a proof
    std::vector<uint8_t> staging;              // all three, until the last side has been proved
    unsigned grid = 0;  // the workgroups of every kernel of spark.hip; 0: the rule.  No bit of a result depends on it
    hipEvent_t ev[3] = {};  // around a call's phases, on the null stream
    pkx::Profile prof;

    uint64_t* eq(int which) const { return (uint64_t*)(arena + at.eq[which]); }  // 0: eq(rx, .), 1: eq(ry, .)
    uint64_t* iota() const { return (uint64_t*)(arena + at.iota); }
    uint32_t* counts(int which) const { return (uint32_t*)(arena + at.counts[which]); }
    unsigned long long* bad() const { return (unsigned long long*)(arena + at.bad); }

    pkx_prover() = default;
    pkx_prover(const pkx_prover&) = delete;
    pkx_prover& operator=(const pkx_prover&) = delete;
    // gives back whatever the prover holds, so a creation that stops half way leaks nothing; rc: the first failure's code
    int give_back() {
        int rc = PK_OK;
        if (val)
            if (int r = pks_prover_destroy(val)) rc = rc ? rc : r;
        val = nullptr;
        for (pkt_prover*& l : look) {
            if (l)
                if (int r = pkt_prover_destroy(l)) rc = rc ? rc : r;
            l = nullptr;
        }
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (arena)
            if (int r = pk_free(ctx, arena)) rc = rc ? rc : r;
        arena = nullptr;
        return rc;
    }
    ~pkx_prover() { (void)give_back(); }
};
