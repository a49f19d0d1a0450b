// prover.hpp -- what a pkb_prover holds, for prover.cpp; and for the lab (tools/probes/bitwise.hip), which sets the grid of a prover's
// kernels and reads where its last calls' time went: test and benchmark knobs that the C ABI does not carry.
#pragma once
#include <memory>
#include <vector>

#include "../prover_transcript.hpp"
#include "kernels.hpp"

namespace pkb {

// Where the last calls' time went, in milliseconds: the device time of the last pkb_decompose's launches (events around them), and the
// last proof's pkt_prove in host time -- two clocks.  What has not run reads 0.
struct Profile {
    double decompose_ms = 0, lookup_ms = 0;
};

}  // namespace pkb

struct pkb_prover {
    pk_ctx* ctx = nullptr;
    pkb_statement st{};
    pkb::Plan plan{};
    std::string pattern, err;
    uint8_t* arena = nullptr;  // layout.hpp
    pkb::Layout at;
    pkt_prover* look = nullptr;    // (n, 2 d, w = 3, c, n_bind = 1)
    size_t proof_bytes = 0;        // pkt_proof_bytes of it
    std::vector<uint8_t> staging;  // the proof, until pkt_prove has accepted the columns
    unsigned grid = 0;  // the workgroups of every kernel of bitwise.hip; 0: the rule.  No bit of a result depends on it
    hipEvent_t ev[2] = {nullptr, nullptr};  // around a call's launches, on the null stream
    pkb::Profile prof;

    uint64_t* table(int j) const { return (uint64_t*)(arena + at.table[j]); }
    uint32_t* counts() const { return (uint32_t*)(arena + at.counts); }
    unsigned long long* bad() const { return (unsigned long long*)(arena + at.bad); }

    pkb_prover() = default;
    pkb_prover(const pkb_prover&) = delete;
    pkb_prover& operator=(const pkb_prover&) = delete;
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
    ~pkb_prover() { (void)give_back(); }
};
