// prover.hpp -- what a pkr_prover holds, for prover.cpp; and for the lab (tools/probes/rangecheck.hip), which sets the grid of a prover's
// kernels and reads where its last calls' time went: test and benchmark knobs that the C ABI does not carry.
#pragma once
#include <memory>
#include <vector>

#include "../prover_transcript.hpp"
#include "kernels.hpp"

namespace pkr {

// Where the last calls' time went, in milliseconds: the device time of the last pkr_decompose's launches and of the last proof's scale
// pass (events around them), and the last proof's pkt_prove in host time -- two clocks.  What has not run reads 0.
struct Profile {
    double decompose_ms = 0, scale_ms = 0, lookup_ms = 0;
};

}  // namespace pkr

struct pkr_prover {
    pk_ctx* ctx = nullptr;
    pkr_statement st{};
    pkr::Plan plan{};
    std::string pattern, err;
    uint8_t* arena = nullptr;  // layout.hpp
    pkr::Layout at;
    pkt_prover* look = nullptr;    // (n, k, w = 1, c, n_bind = 1)
    size_t proof_bytes = 0;        // pkt_proof_bytes of it
    std::vector<uint8_t> staging;  // the proof, until pkt_prove has accepted the columns
    unsigned grid = 0;  // the workgroups of every kernel of range.hip; 0: the rule.  No bit of a result depends on it
    hipEvent_t ev[2] = {nullptr, nullptr};  // around a call's launches, on the null stream
    pkr::Profile prof;

    uint64_t* iota() const { return (uint64_t*)(arena + at.iota); }
    uint64_t* scaled() const { return (uint64_t*)(arena + at.scaled); }  // only when plan.r < st.k
    uint32_t* counts() const { return (uint32_t*)(arena + at.counts); }
    unsigned long long* bad() const { return (unsigned long long*)(arena + at.bad); }

    pkr_prover() = default;
    pkr_prover(const pkr_prover&) = delete;
    pkr_prover& operator=(const pkr_prover&) = delete;
    // gives back whatever the prover holds, so a creation that stops half way leaks nothing; rc: the first failure's code
    int give_back() {
        int rc = PK_OK;
        if (look)
            if (int r = pkt_prover_destroy(look)) rc = rc ? rc : r;
        look = nullptr;
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (arena)
            if (int r = pk_free(ctx, arena)) rc = rc ? rc : r;
        arena = nullptr;
        return rc;
    }
    ~pkr_prover() { (void)give_back(); }
};
