/*
 * provekit_sumcheck_sharded.h -- libprovekit_sumcheck.so on the contexts of a device set: one product sumcheck (provekit_sumcheck.h)
 * sharded over the G ranks of the set.  Opt-in, under its own prefix: pks_prover_create on a context of a set keeps running whole on
 * its rank.  The proof is pks_prove's, byte for byte, on every rank; pks_verify verifies it.
 *
 * The ownership rule (csrc/sumcheck/shard.hpp, from which the kernel, the prover and pkss_plan are compiled).  Rounds bind the most
 * significant index bit first, so the low index bits outlive every fold.  With G = 2^g ranks (g >= 1) and c = PKSS_CHUNK_LOG2 = 8,
 * rank r owns the indices x whose bits [c, c + g) spell r -- every G-th chunk of 256 elements -- and its compacted index is
 *     y = (x >> (c + g)) << c | (x & (2^c - 1)).
 * Compaction maps the pair (x, x + len/2) to (y, y + len_local/2): a rank's compacted table is an ordinary sumcheck table of length
 * len / G.  Round i is sharded iff n - 1 - i >= c + g: S = max(0, n - c - g) sharded rounds, then n - S replicated ones.
 *
 * A sharded round: each rank runs its slice (round.hip's sharded kernel: rounds 0 and 1 read the caller's full tables at the rank's
 * own indices, round 1 folds them into the rank's compacted arena, later rounds fold that arena in place; the eq weights are indexed
 * by the global pair index), then ONE pk_comm_all_gather of 32 * (D + 2) bytes per rank carries its D + 1 sums and the status of
 * its rank-local work so far.  Every rank adds the G blocks -- field addition is exact, so the sums' bits are the lone prover's --
 * feeds them to its own transcript and squeezes the same challenge.  Every rank leaves with the first non-zero status in rank order,
 * so that no rank enters a collective another rank has left.  After round S - 1 the ranks' arenas hold the tables at global length
 * 2^(c+g+1); one all-gather and one kernel put them into global order on every rank, and the remaining rounds are the lone prover's
 * (with S <= 1 nothing has been written yet and they read the caller's tables; with S = 0 the whole proof is replicated and the only
 * collectives are the agreement exchanges).  Every wait is under pk_comm's deadline (provekit_hip.h, "device sets").
 *
 * Agreement.  pkss_prover_create exchanges a digest of the statement, pkss_prove a digest of what the transcript absorbed before
 * the proof (bind, tau, coefficients).  If the ranks disagree, all of them refuse with PK_ERR_BAD_ARG and a reason that names the
 * first rank that differs from rank 0; nothing is proved.  NOT DETECTED: ranks handed different table contents.  The proof is then
 * a proof of no table, and openings at its point fail.
 *
 * Memory: the arena of a rank holds m * 2^(n-1) / G elements of compacted tables (from S = 2 on) where the lone prover's holds
 * m * 2^(n-1); everything else (pkss_plan) does not grow with the tables.  The caller's tables are full on every rank and never written.
 */
#ifndef PROVEKIT_SUMCHECK_SHARDED_H
#define PROVEKIT_SUMCHECK_SHARDED_H

#include "provekit_sumcheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKSS_CHUNK_LOG2 8
#define PKSS_MAX_WORLD_LOG2 4 /* PK_MAX_RANKS = 16 */

struct pkss_plan {
    unsigned g;           /* log2 of the world */
    unsigned c;           /* PKSS_CHUNK_LOG2 */
    unsigned S;           /* sharded rounds: 0 .. S-1; S .. n-1 are replicated */
    size_t local_len;     /* a rank's share of a table: 2^n / G elements (0 with S = 0: nothing is sharded) */
    size_t handover_len;  /* 2^(c+g+1): each table of the replicated rounds' region; with S >= 2 the global length at the hand-over */
    size_t arena_bytes;   /* the prover's one device allocation on each rank */
};

int pkss_abi_version(void);

/* Host only (the struct and the call share their name, as stat does: write `struct pkss_plan`).  PK_ERR_BAD_ARG with a reason
 * (pks_create_error): a null pointer, whatever pks_proof_bytes refuses of the statement, a world below 2, above
 * 2^PKSS_MAX_WORLD_LOG2, or not a power of two. */
int pkss_plan(const pks_statement *stmt, unsigned world, struct pkss_plan *out);

/* Collective: every rank of ctx's device set calls it with the same statement (rank and world are pk_comm_info's).  Refused at once,
 * with a reason, outside a set and for a world pkss_plan refuses; ranks whose statements differ all refuse.  The prover is a
 * pks_prover: pks_prover_destroy and pks_last_error serve it, pks_create_error reports a refused creation; pks_prove refuses it. */
int pkss_prover_create(pk_ctx *ctx, const pks_statement *stmt, pks_prover **out);

/* Collective; pks_prove's arguments, the same on every rank, and pks_prove's bytes, point and finals on every rank.  A short proof
 * buffer, a missing tau and the like are refused on every rank and the prover stays usable. */
int pkss_prove(pks_prover *p, const uint64_t *const *d_tables, const uint64_t *tau_or_null, const uint64_t *bind, uint8_t *proof_out,
               size_t cap, size_t *len, uint64_t *point_out, uint64_t *finals_out);

/* What this rank's last successful pkss_prove did, round by round (tools/sumcheck_sharded_profile.py): whether the round was sharded,
 * the pairs this rank's launch covered (the round's / G when sharded: the launch argument the bytes read follow from), the host
 * time from the launch to its sums on the host, and the time of the exchange behind it.  rounds: up to cap of the n entries.
 * handover_seconds: pack, gather and reorder; total_seconds: the whole call.  Host wall time of blocking steps. */
typedef struct pkss_round_profile {
    unsigned sharded;
    uint64_t pairs;
    double round_seconds, exchange_seconds;
} pkss_round_profile;
int pkss_last_profile(const pks_prover *p, pkss_round_profile *rounds, unsigned cap, double *handover_seconds, double *total_seconds);

/* ONE rank's slice of ONE sharded round on a lone context, no communicator (tests, tools; as pks_round).  d_tables: m FULL tables of
 * current length len = 2^k.  fold NULL: out = the rank's D + 1 partial sums over its own pairs (x, x + len/2); the round's length is
 * len.  fold given: the rank's part of the tables folded to length len/2 goes, compacted, to d_out_local (m device pointers of
 * len / 2 / world elements), and the sums are those of the folded tables; the round's length is len/2.  The round's length must be
 * at least 2^(c+g+1) (the round is sharded).  tau_rest, grid, out: pks_round's.  The field sum of the ranks' outs is pks_round's out. */
int pkss_round_shard(pk_ctx *ctx, const pks_statement *stmt, const uint64_t *const *d_tables, size_t len, const uint64_t *tau_rest_or_null,
                     const uint64_t *fold_or_null, uint64_t *const *d_out_local, unsigned world, unsigned rank, unsigned grid, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_SUMCHECK_SHARDED_H */
