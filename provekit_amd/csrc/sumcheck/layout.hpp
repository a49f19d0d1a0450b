// layout.hpp -- the layout of a prover's arena, lone or on a device set: what the prover allocates and walks, what pkss_plan reports and
// what the sanitizer driver prints.  Host only; no prover object, no product call.
#pragma once
#include "round.hpp"
#include "shard.hpp"

namespace pkss {

// what a rank contributes to the exchange behind a sharded round: up to D + 1 sums, and one element whose first limb is its status
constexpr size_t XCHG_FES = PKS_MAX_TERM_TABLES + 2;

// A prover's arena, in field elements from its start:
//   [compact: m tables of 2^(n-1) / G -- the rank's compacted tables from round 1 on; none with S < 2: nothing sharded is ever stored]
//   [replicated: m tables of 2^(c+g+1) -- the hand-over's global tables, and what the replicated rounds fold in place]
//   [gather: the rank's m x 2^(c+1) hand-over block, then the G gathered ones] [exchange: XCHG_FES, then G x XCHG_FES]
//   [round scratch] [split eq tables of n - 1 coordinates]
// The lone prover is a device set of one, g = 0: no round is sharded, nothing is compacted, gathered or exchanged, and the replicated
// tables are the folded copies of half length -- [m tables of 2^(n-1)] [round scratch] [split eq tables], pks::lone_arena_fes in all.
struct Layout {
    unsigned g = 0, S = 0;
    size_t local_half = 0, handover = 0;  // the strides of the compact and the replicated tables
    size_t compact = 0, replicated = 0, gather_send = 0, gather_recv = 0, xchg_send = 0, xchg_recv = 0, scratch = 0, eq = 0, total = 0;
};
// scratch_fes: one round's scratch, ROUND_SCRATCH_FES or the wide statements' WIDE_SCRATCH_FES
inline Layout layout(unsigned n, unsigned m, unsigned g, size_t scratch_fes = pks::ROUND_SCRATCH_FES) {
    Layout L;
    L.g = g, L.S = g ? sharded_rounds(n, g) : 0;
    L.local_half = L.S >= 2 ? ((size_t)1 << (n - 1)) >> g : 0;
    L.handover = g ? handover_len(g) : (size_t)1 << (n - 1);
    const size_t block = g ? (size_t)m << (C + 1) : 0, xchg = g ? XCHG_FES : 0, G = (size_t)1 << g;
    L.replicated = L.compact + m * L.local_half;
    L.gather_send = L.replicated + m * L.handover;
    L.gather_recv = L.gather_send + block;
    L.xchg_send = L.gather_recv + G * block;
    L.xchg_recv = L.xchg_send + xchg;
    L.scratch = L.xchg_recv + G * xchg;
    L.eq = L.scratch + scratch_fes;
    L.total = L.eq + pks::eq_split(n - 1).fes();
    return L;
}

}  // namespace pkss
