/*
 * provekit_engine.h -- C ABI of libprovekit_engine.so: many proofs in flight from ONE caller thread.
 *
 * The reference calls WhirR1CSProver::prove from one thread and lets its engine (rayon) supply the parallelism.
 * libprovekit_hip.so gives one caller thread one proof at a time; the chip is full only with a dozen or more provers in
 * flight, each with a pk_ctx, a pk_scheme and an arena of its own (INTEGRATION.md "Threading").  This library owns those
 * provers ("lanes"), one worker thread per lane and a job queue, so that a binder with a single thread reaches the same
 * throughput.  It is a layer ABOVE the product's C ABI: plain host code that calls only what provekit_hip.h declares
 * (plus the HIP runtime's free-memory query, hipMemGetInfo, to size itself); it holds no kernel and the product library does not know it.
 *
 * Conventions
 *   - Every call returns PK_OK (0) or a negative PK_ERR_* of provekit_hip.h (PKE_ERR_CANCELLED is the one code added here).
 *   - Pointers named d_* are DEVICE pointers on the engine's device, the rest are host pointers.  Every buffer a job names
 *     (witness, seed, transcript_out, len, status) is the caller's and must stay valid until the job is final: until the
 *     pke_wait / pke_wait_all / pke_prove_many that covers it returns, or pke_engine_destroy does.  Witness buffers are
 *     only read; several jobs may share one.
 *   - A job's proof depends on (scheme, witness, seed) alone, never on the lane that ran it or on the order of completion.
 *   - pke_submit, pke_wait, pke_wait_all and the *_many calls may be made from any thread, also concurrently.
 *     pke_engine_destroy must be the last call: nothing else may be in progress or follow it.
 *   - Worker threads are created once, in pke_engine_create; an idle lane sleeps on a condition variable.
 */
#ifndef PROVEKIT_ENGINE_H
#define PROVEKIT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#include "provekit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PKE_MAX_LANES 32      /* hard cap on the lanes of one engine */
#define PKE_AUTO_LANES_MAX 16 /* what lanes == 0 picks at most */
/* status of a job that pke_engine_destroy found still queued: it never ran, its transcript_out is untouched */
#define PKE_ERR_CANCELLED (-100)
/* pke_engine_create flags */
#define PKE_KEEP_HOST_WAIT 1u /* leave the device's host-wait mode as the caller set it (default: PK_WAIT_POLL is selected) */
/* the "job" of pke_engine_last_error that names the engine itself (pke_engine_set_* failures) */
#define PKE_NO_JOB UINT64_MAX

typedef struct pke_engine pke_engine;
/* a job's ticket: tickets of one engine count up from 0 in submission order */
typedef uint64_t pke_job;

/* Builds `lanes` provers of the scheme {m, m_0, whir_witness, whir_for_hiding_spartan} (the arguments of pk_scheme_create)
 * over the uploaded `r1cs` -- a pk_r1cs serves every context of its device, so the caller uploads it once and destroys it
 * after the engine -- each lane a pk_ctx + pk_scheme of its own, and one worker thread per lane.
 * lanes == 0 picks a count: min(PKE_AUTO_LANES_MAX, floor(0.8 * free device memory / per-lane bytes)) with per-lane bytes =
 * pk_scheme_arena_bytes + 8 * 32 * 2^m_0 (the statement's working copy) + 256 MiB (workspace); PK_ERR_OOM if not even one fits.
 * (The query selects `device` on the calling thread and puts the thread's previous current device back before it returns.)
 * lanes > PKE_MAX_LANES is PK_ERR_BAD_ARG.  A lane that cannot be built (PK_ERR_OOM at lane k, ...) tears down the lanes
 * before it; the product library's code is returned and its message is kept for pke_create_error().
 * Unless flags has PKE_KEEP_HOST_WAIT the device is put in PK_WAIT_POLL (pk_device_set_host_wait) before the first lane's
 * context exists: a lane thread then sleeps between stream queries instead of spinning on a core of its own.  The engine
 * never selects PK_WAIT_BLOCK. */
int pke_engine_create(int device, const pk_r1cs *r1cs, size_t num_constraints, size_t num_witnesses, unsigned m, unsigned m_0,
                      const pk_whir_config *whir_witness, const pk_whir_config *whir_for_hiding_spartan, unsigned lanes,
                      unsigned flags, pke_engine **out);
/* message of the calling thread's last failed pke_engine_create ("" if none) */
const char *pke_create_error(void);
/* Cancels the jobs still queued (status PKE_ERR_CANCELLED), lets the running ones finish, joins the workers, destroys the
 * witness programs, the schemes, then the contexts.  Every job's status and len are final when it returns. */
int pke_engine_destroy(pke_engine *engine);
int pke_engine_lanes(const pke_engine *engine);

/* The three below wait until the engine is idle, then apply the setting to every lane from the calling thread; a failure
 * leaves the message under pke_engine_last_error(engine, PKE_NO_JOB).
 * pke_engine_set_io_pattern: pk_scheme_set_io_pattern on every lane (NULL / 0 restores the library's restatement).
 * pke_engine_set_hash_version: pk_ctx_set_hash_version on every lane.
 * pke_engine_set_witness_builders: pk_witness_builders_from_postcard on every lane (a witness program belongs to one
 * context), replacing an earlier list; what pke_noir_submit / pke_noir_prove_many run.  NULL / 0 removes it. */
int pke_engine_set_io_pattern(pke_engine *engine, const uint8_t *pattern, size_t n);
int pke_engine_set_hash_version(pke_engine *engine, int version);
int pke_engine_set_witness_builders(pke_engine *engine, const uint8_t *postcard, size_t len, size_t *n_witnesses,
                                    size_t *n_challenges, size_t *n_acir);
/* the domain separator in force on every lane (pk_scheme_domain_separator of lane 0) */
int pke_engine_domain_separator(const pke_engine *engine, char *buf, size_t cap, size_t *len);

/* Queues one pk_prove(lane ctx, lane scheme, d_witness, n_witness, rng_seed32, transcript_out, cap, len) and returns at
 * once; the next idle lane runs it.  *status (may be NULL) receives pk_prove's return code and *len (may be NULL) the
 * proof's length when the job is final.  *job (may be NULL) receives the ticket. */
int pke_submit(pke_engine *engine, const uint64_t *d_witness, size_t n_witness, const uint8_t *rng_seed32,
               uint8_t *transcript_out, size_t cap, size_t *len, int *status, pke_job *job);
/* the same over pk_noir_prove with the lane's witness program (PK_ERR_BAD_ARG if none is set) */
int pke_noir_submit(pke_engine *engine, const uint64_t *d_acir, size_t n_acir, const uint32_t *public_acir_idx, size_t n_public,
                    const uint8_t *rng_seed32, uint8_t *transcript_out, size_t cap, size_t *len, int *status, pke_job *job);
/* Blocks until `job` is final and returns ITS status (PK_ERR_BAD_ARG for a ticket never issued).  The job's status slot is the
 * lasting record: the engine itself remembers the codes and messages of the last 1024 failed jobs only, so a failed job waited on
 * after 1024 later failures reads PK_OK here (as pke_engine_last_error reads ""). */
int pke_wait(pke_engine *engine, pke_job job);
/* Blocks until every job submitted so far is final.  PK_OK; the jobs' own results are in their status slots. */
int pke_wait_all(pke_engine *engine);

/* n jobs in one blocking call: pke_submit for each, then pke_wait for each.  d_witness[i], n_witness[i], transcript_out[i],
 * cap[i] describe job i; rng_seed32 may be NULL, and so may any rng_seed32[i] (fresh OS randomness, the production form);
 * len and status may be NULL.  Returns PK_OK iff every job did, otherwise the status of the first job (by index) that
 * failed; a failed job does not stop the others -- a job the queue itself refuses (transcript_out[i] == NULL with cap[i] != 0:
 * PK_ERR_BAD_ARG, it has no ticket) included.  n may be below, equal to or above the lane count; n == 0 is PK_OK.
 * *first_job (may be NULL): job i has ticket *first_job + i when nobody else submits meanwhile and no job was refused by the queue. */
int pke_prove_many(pke_engine *engine, size_t n, const uint64_t *const *d_witness, const size_t *n_witness,
                   const uint8_t *const *rng_seed32, uint8_t *const *transcript_out, const size_t *cap, size_t *len, int *status,
                   pke_job *first_job);
int pke_noir_prove_many(pke_engine *engine, size_t n, const uint64_t *const *d_acir, const size_t *n_acir,
                        const uint32_t *public_acir_idx, size_t n_public, const uint8_t *const *rng_seed32,
                        uint8_t *const *transcript_out, const size_t *cap, size_t *len, int *status, pke_job *first_job);

/* pk_last_error of the lane that ran `job`, copied when the job failed ("" for a job that succeeded, is not final, or
 * failed more than 1024 failures ago); PKE_NO_JOB: the last failure of a pke_engine_set_* call.  The pointer stays valid
 * until 1024 later failures or pke_engine_destroy. */
const char *pke_engine_last_error(const pke_engine *engine, pke_job job);

#ifdef __cplusplus
}
#endif
#endif /* PROVEKIT_ENGINE_H */
