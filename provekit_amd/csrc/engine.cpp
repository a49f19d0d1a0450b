// engine.cpp -- libprovekit_engine.so (include/provekit_engine.h): K provers of libprovekit_hip.so kept in flight for ONE caller
// thread.  Host code only, above the product's C ABI: every pk_* call below is declared in provekit_hip.h, nothing in this
// directory is included, and the product library neither exports anything for this file nor knows it exists.
//
// Shape: one mutex, a FIFO of jobs, one worker thread per lane.  A lane is a pk_ctx + pk_scheme (+ pk_witness_program) of its own --
// contexts are single-caller, so a lane's handles are touched by its worker while jobs run and by the caller only while the engine
// is idle (the pke_engine_set_* calls wait for that under the same mutex).  A worker sleeps on `work` when the queue is empty; a
// waiter sleeps on `done`.  Job results go straight to the caller's slots; the engine keeps only the tickets still open and the
// messages of the jobs that failed.
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

// The one thing provekit_hip.h does not offer is the device's free memory, which lanes == 0 needs: hipMemGetInfo, from the HIP
// runtime's C API header (plain C, read by the host compiler; the runtime is in the process already, the product library links it).
#include <hip/hip_runtime_api.h>

#include "provekit_engine.h"

namespace {

constexpr size_t kMaxKeptErrors = 1024;

struct Lane {
    pk_ctx *ctx = nullptr;
    pk_scheme *scheme = nullptr;
    pk_witness_program *builders = nullptr;
    std::thread worker;
};

struct Job {
    pke_job ticket;
    bool noir;
    const uint64_t *d_in;  // witness, or the dense ACIR witness map
    size_t n_in;
    const uint32_t *public_idx;
    size_t n_public;
    const uint8_t *seed;
    uint8_t *out;
    size_t cap;
    size_t *len;
    int *status;
};

struct Failure {
    int code;
    std::string msg;
};

thread_local std::string t_create_error;

}  // namespace

struct pke_engine {
    int device = 0;
    std::vector<Lane> lanes;
    mutable std::mutex mu;
    std::condition_variable work, done;
    std::deque<Job> queue;
    std::set<pke_job> open;  // submitted, not final (queued or running)
    pke_job next_ticket = 0;
    bool stopping = false;
    std::map<pke_job, Failure> failures;  // the last kMaxKeptErrors failed jobs, by ticket
    std::string engine_error;

    // mu held
    void finish(const Job &j, int rc, size_t len, const char *msg) {
        if (j.len) *j.len = len;
        if (j.status) *j.status = rc;
        if (rc != PK_OK) {
            failures[j.ticket] = Failure{rc, msg ? msg : ""};
            while (failures.size() > kMaxKeptErrors) failures.erase(failures.begin());
        }
        open.erase(j.ticket);
    }

    void run_lane(size_t k) {
        Lane &ln = lanes[k];
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            work.wait(lk, [&] { return stopping || !queue.empty(); });
            if (queue.empty()) return;  // stopping: pke_engine_destroy has cancelled what was queued
            const Job j = queue.front();
            queue.pop_front();
            lk.unlock();
            size_t len = 0;
            int rc;
            if (!j.noir)
                rc = pk_prove(ln.ctx, ln.scheme, j.d_in, j.n_in, j.seed, j.out, j.cap, &len);
            else if (!ln.builders)
                rc = PK_ERR_BAD_ARG;
            else
                rc = pk_noir_prove(ln.ctx, ln.scheme, ln.builders, j.d_in, j.n_in, j.public_idx, j.n_public, j.seed, j.out, j.cap, &len);
            const std::string msg = rc == PK_OK ? "" : (j.noir && !ln.builders ? "no witness builders set (pke_engine_set_witness_builders)" : pk_last_error(ln.ctx));
            lk.lock();
            finish(j, rc, rc == PK_OK ? len : 0, msg.c_str());
            done.notify_all();
        }
    }

    // mu held through lk; returns with the queue empty and no lane running
    void wait_idle(std::unique_lock<std::mutex> &lk) {
        done.wait(lk, [&] { return open.empty(); });
    }

    int submit(Job j, pke_job *ticket) {
        if (!j.out && j.cap) return PK_ERR_BAD_ARG;
        std::lock_guard<std::mutex> lk(mu);
        if (stopping) return PK_ERR_BAD_ARG;
        j.ticket = next_ticket;
        try {
            open.insert(j.ticket);
            queue.push_back(j);
        } catch (const std::exception &) {
            open.erase(j.ticket);
            return PK_ERR_OOM;
        }
        next_ticket++;
        if (j.status) *j.status = PK_OK;
        if (j.len) *j.len = 0;
        if (ticket) *ticket = j.ticket;
        work.notify_one();
        return PK_OK;
    }

    void destroy_lanes() {
        for (Lane &ln : lanes)
            if (ln.builders) pk_witness_program_destroy(ln.ctx, ln.builders);
        for (Lane &ln : lanes)
            if (ln.scheme) pk_scheme_destroy(ln.ctx, ln.scheme);
        for (Lane &ln : lanes)
            if (ln.ctx) pk_ctx_destroy(ln.ctx);
        lanes.clear();
    }
};

extern "C" {

const char *pke_create_error(void) { return t_create_error.c_str(); }

int pke_engine_create(int device, const pk_r1cs *r1cs, size_t num_constraints, size_t num_witnesses, unsigned m, unsigned m_0,
                      const pk_whir_config *whir_witness, const pk_whir_config *whir_for_hiding_spartan, unsigned lanes, unsigned flags,
                      pke_engine **out) {
    t_create_error.clear();
    auto fail = [&](int rc, const std::string &msg) {
        t_create_error = msg;
        return rc;
    };
    if (out) *out = nullptr;
    int n_dev = 0;
    if (int rc = pk_device_count(&n_dev)) return fail(rc, "pk_device_count failed: no HIP device (libprovekit_engine has no CPU fallback)");
    if (n_dev <= 0) return fail(PK_ERR_NO_DEVICE, "no HIP device visible (libprovekit_engine has no CPU fallback)");
    if (device < 0 || device >= n_dev) return fail(PK_ERR_NO_DEVICE, "bad device ordinal");
    if (!out || !r1cs || !whir_witness || !whir_for_hiding_spartan) return fail(PK_ERR_BAD_ARG, "pke_engine_create: NULL argument");
    if (lanes > PKE_MAX_LANES) return fail(PK_ERR_BAD_ARG, "pke_engine_create: more than PKE_MAX_LANES lanes");
    if (flags & ~PKE_KEEP_HOST_WAIT) return fail(PK_ERR_BAD_ARG, "pke_engine_create: unknown flag");
    if (!(flags & PKE_KEEP_HOST_WAIT))
        if (int rc = pk_device_set_host_wait(device, PK_WAIT_POLL)) return fail(rc, "pk_device_set_host_wait(PK_WAIT_POLL) failed");
    if (lanes == 0) {
        size_t arena = 0, free_b = 0, total_b = 0;
        if (int rc = pk_scheme_arena_bytes(m, m_0, num_witnesses, whir_witness, &arena)) return fail(rc, "pk_scheme_arena_bytes: bad scheme shape");
        if (m_0 >= 48) return fail(PK_ERR_BAD_ARG, "pke_engine_create: m_0 out of range");
        int before = -1;
        const bool had_device = hipGetDevice(&before) == hipSuccess;
        const bool asked = hipSetDevice(device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        if (had_device && before != device) (void)hipSetDevice(before);  // the caller's current device is the caller's
        if (!asked) {
            (void)hipGetLastError();
            return fail(PK_ERR_HIP, "hipMemGetInfo failed");
        }
        const double per_lane = (double)arena + 8.0 * 32.0 * (double)((size_t)1 << m_0) + (double)((size_t)256 << 20);
        const double fit = 0.8 * (double)free_b / per_lane;
        if (fit < 1.0) return fail(PK_ERR_OOM, "pke_engine_create: not even one lane fits in 80 % of the free device memory");
        lanes = fit >= (double)PKE_AUTO_LANES_MAX ? (unsigned)PKE_AUTO_LANES_MAX : (unsigned)fit;
    }
    // nothing may throw across the C boundary: allocation and thread creation failures tear down what exists and become a status
    pke_engine *e = nullptr;
    try {
        e = new pke_engine;
        e->lanes.resize(lanes);
    } catch (const std::exception &ex) {
        delete e;
        return fail(PK_ERR_OOM, std::string("pke_engine_create: ") + ex.what());
    }
    e->device = device;
    for (unsigned k = 0; k < lanes; k++) {
        Lane &ln = e->lanes[k];
        int rc = pk_ctx_create(device, &ln.ctx);
        std::string msg;
        if (rc) {
            ln.ctx = nullptr;
            msg = "pk_ctx_create failed";
        } else if ((rc = pk_scheme_create(ln.ctx, r1cs, num_constraints, num_witnesses, m, m_0, whir_witness, whir_for_hiding_spartan, &ln.scheme))) {
            ln.scheme = nullptr;
            msg = pk_last_error(ln.ctx);
        }
        if (rc) {
            e->destroy_lanes();
            delete e;
            return fail(rc, "lane " + std::to_string(k) + " of " + std::to_string(lanes) + ": " + msg);
        }
    }
    try {
        for (unsigned k = 0; k < lanes; k++) e->lanes[k].worker = std::thread([e, k] { e->run_lane(k); });
    } catch (const std::exception &ex) {
        const std::string why = std::string("pke_engine_create: worker thread: ") + ex.what();
        pke_engine_destroy(e);  // stops and joins the workers that did start, frees every lane
        return fail(PK_ERR_OOM, why);
    }
    *out = e;
    return PK_OK;
}

int pke_engine_destroy(pke_engine *e) {
    if (!e) return PK_OK;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        e->stopping = true;
        for (const Job &j : e->queue) e->finish(j, PKE_ERR_CANCELLED, 0, "cancelled by pke_engine_destroy before a lane took it");
        e->queue.clear();
    }
    e->work.notify_all();
    e->done.notify_all();
    for (Lane &ln : e->lanes)
        if (ln.worker.joinable()) ln.worker.join();
    e->destroy_lanes();
    delete e;
    return PK_OK;
}

int pke_engine_lanes(const pke_engine *e) { return e ? (int)e->lanes.size() : 0; }

int pke_engine_set_io_pattern(pke_engine *e, const uint8_t *pattern, size_t n) {
    if (!e) return PK_ERR_BAD_ARG;
    std::unique_lock<std::mutex> lk(e->mu);
    e->wait_idle(lk);
    for (Lane &ln : e->lanes)
        if (int rc = pk_scheme_set_io_pattern(ln.ctx, ln.scheme, pattern, n)) {
            e->engine_error = pk_last_error(ln.ctx);  // a refusal depends on the scheme's shape alone: lane 0 refuses, nothing has changed
            return rc;
        }
    return PK_OK;
}

int pke_engine_set_hash_version(pke_engine *e, int version) {
    if (!e) return PK_ERR_BAD_ARG;
    std::unique_lock<std::mutex> lk(e->mu);
    e->wait_idle(lk);
    for (Lane &ln : e->lanes)
        if (int rc = pk_ctx_set_hash_version(ln.ctx, version)) {
            e->engine_error = pk_last_error(ln.ctx);
            return rc;
        }
    return PK_OK;
}

int pke_engine_set_witness_builders(pke_engine *e, const uint8_t *postcard, size_t len, size_t *n_witnesses, size_t *n_challenges, size_t *n_acir) {
    if (!e) return PK_ERR_BAD_ARG;
    std::unique_lock<std::mutex> lk(e->mu);
    e->wait_idle(lk);
    std::vector<pk_witness_program *> fresh(e->lanes.size(), nullptr);
    size_t nw = 0, nch = 0, nac = 0;
    int rc = PK_OK;
    if (postcard && len)
        for (size_t k = 0; k < e->lanes.size() && !rc; k++)
            if ((rc = pk_witness_builders_from_postcard(e->lanes[k].ctx, postcard, len, &fresh[k], &nw, &nch, &nac))) {
                fresh[k] = nullptr;
                e->engine_error = pk_last_error(e->lanes[k].ctx);
            }
    for (size_t k = 0; k < e->lanes.size(); k++) {  // success: the new list replaces the old; failure: the new ones go, the old stay
        pk_witness_program *&drop = rc ? fresh[k] : e->lanes[k].builders;
        if (drop) pk_witness_program_destroy(e->lanes[k].ctx, drop);
        if (!rc) e->lanes[k].builders = fresh[k];
    }
    if (rc) return rc;
    if (n_witnesses) *n_witnesses = nw;
    if (n_challenges) *n_challenges = nch;
    if (n_acir) *n_acir = nac;
    return PK_OK;
}

int pke_engine_domain_separator(const pke_engine *e, char *buf, size_t cap, size_t *len) {
    if (!e || e->lanes.empty()) return PK_ERR_BAD_ARG;
    return pk_scheme_domain_separator(e->lanes[0].scheme, buf, cap, len);
}

int pke_submit(pke_engine *e, const uint64_t *d_witness, size_t n_witness, const uint8_t *rng_seed32, uint8_t *transcript_out, size_t cap,
               size_t *len, int *status, pke_job *job) {
    if (!e) return PK_ERR_BAD_ARG;
    return e->submit(Job{0, false, d_witness, n_witness, nullptr, 0, rng_seed32, transcript_out, cap, len, status}, job);
}

int pke_noir_submit(pke_engine *e, const uint64_t *d_acir, size_t n_acir, const uint32_t *public_acir_idx, size_t n_public,
                    const uint8_t *rng_seed32, uint8_t *transcript_out, size_t cap, size_t *len, int *status, pke_job *job) {
    if (!e) return PK_ERR_BAD_ARG;
    return e->submit(Job{0, true, d_acir, n_acir, public_acir_idx, n_public, rng_seed32, transcript_out, cap, len, status}, job);
}

int pke_wait(pke_engine *e, pke_job job) {
    if (!e) return PK_ERR_BAD_ARG;
    std::unique_lock<std::mutex> lk(e->mu);
    if (job >= e->next_ticket) return PK_ERR_BAD_ARG;
    e->done.wait(lk, [&] { return !e->open.count(job); });
    auto it = e->failures.find(job);
    return it == e->failures.end() ? PK_OK : it->second.code;
}

int pke_wait_all(pke_engine *e) {
    if (!e) return PK_ERR_BAD_ARG;
    std::unique_lock<std::mutex> lk(e->mu);
    const pke_job upto = e->next_ticket;  // the jobs submitted so far, not the ones other threads add while this one waits
    e->done.wait(lk, [&] { return e->open.empty() || *e->open.begin() >= upto; });
    return PK_OK;
}

static int many(pke_engine *e, size_t n, bool noir, const uint64_t *const *d_in, const size_t *n_in, const uint32_t *public_idx, size_t n_public,
                const uint8_t *const *seeds, uint8_t *const *out, const size_t *cap, size_t *len, int *status, pke_job *first_job) {
    if (!e || (n && (!d_in || !n_in || !out || !cap))) return PK_ERR_BAD_ARG;
    std::vector<pke_job> tickets;
    std::vector<int> own_status;
    std::vector<bool> queued;
    try {
        tickets.resize(n);
        queued.resize(n, false);
        if (!status) own_status.resize(n);
    } catch (const std::exception &) {
        return PK_ERR_OOM;
    }
    int *st = status ? status : own_status.data();
    pke_job first = 0;
    bool have_first = false;
    for (size_t i = 0; i < n; i++) {
        const Job j{0, noir, d_in[i], n_in[i], public_idx, n_public, seeds ? seeds[i] : nullptr, out[i], cap[i], len ? len + i : nullptr, st + i};
        const int rc = e->submit(j, &tickets[i]);
        if (rc) {  // refused by the queue (a NULL buffer): this job fails alone, the others go on
            st[i] = rc;
            if (len) len[i] = 0;
            continue;
        }
        queued[i] = true;
        if (!have_first) first = tickets[i] - i, have_first = true;
    }
    for (size_t i = 0; i < n; i++)
        if (queued[i]) pke_wait(e, tickets[i]);
    if (first_job) *first_job = first;
    for (size_t i = 0; i < n; i++)
        if (st[i]) return st[i];
    return PK_OK;
}

int pke_prove_many(pke_engine *e, size_t n, const uint64_t *const *d_witness, const size_t *n_witness, const uint8_t *const *rng_seed32,
                   uint8_t *const *transcript_out, const size_t *cap, size_t *len, int *status, pke_job *first_job) {
    return many(e, n, false, d_witness, n_witness, nullptr, 0, rng_seed32, transcript_out, cap, len, status, first_job);
}

int pke_noir_prove_many(pke_engine *e, size_t n, const uint64_t *const *d_acir, const size_t *n_acir, const uint32_t *public_acir_idx,
                        size_t n_public, const uint8_t *const *rng_seed32, uint8_t *const *transcript_out, const size_t *cap, size_t *len,
                        int *status, pke_job *first_job) {
    return many(e, n, true, d_acir, n_acir, public_acir_idx, n_public, rng_seed32, transcript_out, cap, len, status, first_job);
}

const char *pke_engine_last_error(const pke_engine *e, pke_job job) {
    if (!e) return "";
    std::lock_guard<std::mutex> lk(e->mu);
    if (job == PKE_NO_JOB) return e->engine_error.c_str();
    auto it = e->failures.find(job);
    return it == e->failures.end() ? "" : it->second.msg.c_str();
}

}  // extern "C"
