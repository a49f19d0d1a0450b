// prover.hpp -- what a pkt_prover holds, for prover.cpp; and for the lab (tools/probes/tuplelookup.hip), which sets the grid of a
// prover's two kernels and reads where its last calls' time went: test and benchmark knobs that the C ABI does not carry.
#pragma once
#include <memory>
#include <vector>

#include "../prover_transcript.hpp"
#include "kernels.hpp"

namespace pkt {

// Where the last calls' time went, in milliseconds: the device time of the last proof's two leaf launches and of the last
// pkt_multiplicities' count and mont launches (events around them), and the two sides' pkf_prove in host time -- two clocks.  What has
// not run reads 0.
struct Profile {
    double leaf_ms = 0, count_ms = 0;
    double side_ms[2] = {};
};

}  // namespace pkt

struct pkt_prover {
    pk_ctx* ctx = nullptr;
    pkt_statement st{};
    std::string pattern, err;
    uint8_t* arena = nullptr;  // layout.hpp
    pkt::Layout at;
    pkf_prover* side[2] = {nullptr, nullptr};  // PKT_SIDE_F: (n + log2 c, unit), PKT_SIDE_T: (k, numerators m)
    size_t side_bytes[2] = {0, 0};             // pkf_proof_bytes of the two
    std::vector<uint8_t> staging;              // both sides' proofs, until the two fractions have been compared
    unsigned grid = 0;  // the workgroups per group of the leaf and count kernels; 0: the rule.  No bit of a result depends on it
    hipEvent_t ev[2] = {nullptr, nullptr};  // around a phase's launches, on the null stream
    pkt::Profile prof;

    uint64_t* leaf(int which) const { return (uint64_t*)(arena + (which == PKT_SIDE_F ? at.leaf_f : at.leaf_t)); }
    uint32_t* counts() const { return (uint32_t*)(arena + at.counts); }
    unsigned long long* bad() const { return (unsigned long long*)(arena + at.bad); }

    pkt_prover() = default;
    pkt_prover(const pkt_prover&) = delete;
    pkt_prover& operator=(const pkt_prover&) = delete;
    // gives back whatever the prover holds, so a creation that stops half way leaks nothing; rc: the first failure's code
    int give_back() {
        int rc = PK_OK;
        for (pkf_prover*& s : side) {
            if (s)
                if (int r = pkf_prover_destroy(s)) rc = rc ? rc : r;
            s = nullptr;
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
    ~pkt_prover() { (void)give_back(); }
};
