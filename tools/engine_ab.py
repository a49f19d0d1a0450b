#!/usr/bin/env python3
"""A/B: the threaded Python driver against the proof engine, on one GPU in one process.

  A  K Python threads, K contexts / schemes / arenas, work handed out dynamically -- the loop bench.py times (restated here;
     bench.py itself is not touched), proofs written without a Python-side copy
  B  ONE caller thread into a K-lane engine (pke_prove_many straight through ctypes, buffers allocated once)
  C  the single caller without the engine: pk_prove in a loop on one context (spinning waits, the best case for one at a time)

Same instance (bench.py's synthetic statement, m = 21 / m_0 = 20 by default), same seeds, the polling host wait in A and B.
Every alternation runs A, B, B' (the same jobs through pke_submit / pke_wait), A: the two A's give the A-vs-A spread that a B-vs-A
difference has to exceed to mean anything (the summary records the largest of them and B minus the mean of its two A's per alternation).
Host CPU is the whole process's user + system time (getrusage) over the timed window.  The digest pass (untimed) proves the same
2K (witness, seed) jobs through each arm and compares sha256 over the proofs in job order: they must be equal.

    python tools/engine_ab.py [--k 16] [--steps 40] [--warmup 2] [--alternations 5] [--log2-size 21] [--out profiles/r08_engine_ab.json]
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import resource
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16, help="provers in flight: threads of arm A, lanes of arm B")
    ap.add_argument("--steps", type=int, default=40, help="timed waves per run; one wave = K proofs")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--log2-size", type=int, default=21, dest="m")
    ap.add_argument("--single-proofs", type=int, default=60, help="proofs of arm C per run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_engine_ab.json"))
    args = ap.parse_args()

    import torch

    torch.cuda.is_available()  # torch's HIP runtime first: one runtime serves both
    import provekit_amd
    from bench import satisfying_witness, synth_r1cs
    from provekit_amd import engine as E
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for

    K, m, m_0 = args.k, args.m, args.m - 1
    n_wit = (1 << (m - 1)) - 5
    cfg_w, cfg_b = WhirConfig.derive(m), blinding_config_for(m_0)
    ctx0 = provekit_amd.Context(0)
    r1cs, _, _, nc, n_in = synth_r1cs(ctx0, m_0, n_wit, seed=1234)  # one upload serves every context of the device
    d_z0, z_host = satisfying_witness(ctx0, r1cs, n_wit, nc, n_in, 99)

    # ---- arm C first, before this process holds K idle queues (spinning waits: one proof at a time) --------------------
    lone = WhirR1CSScheme(ctx0, r1cs, m, m_0, cfg_w, cfg_b)

    def run_c(mode):
        provekit_amd.Context.set_host_wait(0, mode)
        for i in range(4):
            lone.prove_nocopy(d_z0, seed=900000 + i)
        ctx0.sync()
        c0, t0 = cpu_seconds(), time.perf_counter()
        for i in range(args.single_proofs):
            lone.prove_nocopy(d_z0, seed=1 + i)
        ctx0.sync()
        dt = time.perf_counter() - t0
        return {"wait": mode, "proofs": args.single_proofs, "proofs_per_s": args.single_proofs / dt, "ms_per_proof": 1e3 * dt / args.single_proofs,
                "host_cpu_s_per_proof": (cpu_seconds() - c0) / args.single_proofs}

    arm_c = [run_c("spin"), run_c("poll")]
    provekit_amd.Context.set_host_wait(0, "poll")

    # ---- arm A: K contexts, K threads -----------------------------------------------------------------------------------
    workers = []
    for _ in range(K):
        c = provekit_amd.Context(0)
        workers.append((c, WhirR1CSScheme(c, r1cs, m, m_0, cfg_w, cfg_b), c.upload(z_host)))

    def run_a(first_seed, count, keep=None):
        nxt, lock = itertools.count(), threading.Lock()

        def work(w):
            _, prover, d_z = workers[w]
            while True:
                with lock:
                    i = next(nxt)
                if i >= count:
                    return
                if keep is not None:
                    keep[i] = prover.prove(d_z, seed=first_seed + i)
                else:
                    prover.prove_nocopy(d_z, seed=first_seed + i)

        ths = [threading.Thread(target=work, args=(w,)) for w in range(K)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()

    # ---- arm B: one thread, K lanes ---------------------------------------------------------------------------------------
    eng = provekit_amd.ProofEngine(r1cs, m, m_0, cfg_w, cfg_b, lanes=K)
    assert eng.lanes == K
    n_max = max(args.steps, args.warmup, 2) * K
    cap = 512 << 10  # a proof of the bench size is ~269 KB; pages a proof does not reach are never touched
    bufs = [(C.c_uint8 * cap)() for _ in range(n_max)]
    b_w = (C.c_void_p * n_max)(*[d_z0.ptr] * n_max)  # witnesses are only read: every job names the same device vector
    b_nw = (C.c_size_t * n_max)(*[n_wit] * n_max)
    b_cap = (C.c_size_t * n_max)(*[cap] * n_max)
    b_out = (C.c_void_p * n_max)(*[C.addressof(b) for b in bufs])
    b_len, b_status = (C.c_size_t * n_max)(), (C.c_int * n_max)()
    b_seeds = (C.c_uint8 * (32 * n_max))()
    b_sd = (C.c_void_p * n_max)(*[C.addressof(b_seeds) + 32 * i for i in range(n_max)])

    def run_b(first_seed, count, keep=None):
        """`count` jobs in ONE blocking call from this thread, which sleeps inside it"""
        for i in range(count):
            C.memmove(C.addressof(b_seeds) + 32 * i, (first_seed + i).to_bytes(32, "little"), 32)
        rc = E.lib.pke_prove_many(eng.handle, count, b_w, b_nw, b_sd, b_out, b_cap, b_len, b_status, None)
        if rc != 0:
            raise RuntimeError(f"pke_prove_many: {rc} {list(b_status[:count])}")
        if keep is not None:
            for i in range(count):
                keep[i] = C.string_at(bufs[i], b_len[i])

    def run_b_pipelined(first_seed, count):
        """the same through pke_submit / pke_wait with 2K jobs kept in flight and a ring of 2K buffers (what a binder that overlaps its
        witness generation with proving would do)"""
        depth = 2 * K
        tickets = (C.c_uint64 * depth)()

        def at(arr, i, typ):
            return C.cast(C.addressof(arr) + C.sizeof(typ) * i, C.POINTER(typ))

        for i in range(count + depth):
            slot = i % depth
            if i >= depth:
                rc = E.lib.pke_wait(eng.handle, tickets[slot])
                if rc != 0:
                    raise RuntimeError(f"pke_wait: {rc}")
            if i < count:
                C.memmove(C.addressof(b_seeds) + 32 * slot, (first_seed + i).to_bytes(32, "little"), 32)
                rc = E.lib.pke_submit(eng.handle, d_z0.ptr, n_wit, C.addressof(b_seeds) + 32 * slot, bufs[slot], cap, at(b_len, slot, C.c_size_t),
                                      at(b_status, slot, C.c_int), at(tickets, slot, C.c_uint64))
                if rc != 0:
                    raise RuntimeError(f"pke_submit: {rc}")

    # ---- digest pass (untimed): the same 2K jobs through A, B and C ---------------------------------------------------------
    def digest(proofs):
        h = hashlib.sha256()
        for i in sorted(proofs):
            h.update(proofs[i])
        return h.hexdigest()

    nd = 2 * K
    ka, kb = {}, {}
    run_a(1, nd, ka)
    run_b(1, nd, kb)
    kc = {i: lone.prove(d_z0, seed=1 + i) for i in range(nd)}
    digests = {"A": digest(ka), "B": digest(kb), "C": digest(kc), "jobs": nd, "proof_bytes": len(ka[0])}
    digests["equal"] = digests["A"] == digests["B"] == digests["C"]

    # ---- timed alternations ------------------------------------------------------------------------------------------------
    def timed(fn, count):
        torch.cuda.synchronize()
        c0, t0 = cpu_seconds(), time.perf_counter()
        fn(1, count)
        torch.cuda.synchronize()
        dt, cpu = time.perf_counter() - t0, cpu_seconds() - c0
        return {"proofs": count, "seconds": dt, "proofs_per_s": count / dt, "host_cpu_s_per_proof": cpu / count, "host_cores_busy": cpu / dt}

    run_a(100000, args.warmup * K)
    run_b(100000, args.warmup * K)
    run_b_pipelined(100000, args.warmup * K)
    count = args.steps * K
    rounds = []
    for alt in range(args.alternations):
        rounds.append({"A1": timed(run_a, count), "B": timed(run_b, count), "B_submit_wait": timed(run_b_pipelined, count), "A2": timed(run_a, count)})
        print(f"[engine_ab] alternation {alt}: " + "  ".join(f"{k} {v['proofs_per_s']:.1f}/s {v['host_cores_busy']:.2f} cores" for k, v in rounds[-1].items()),
              file=sys.stderr, flush=True)
    arm_c.append(run_c("spin"))  # and once more at the end, with K + K idle provers' queues open
    provekit_amd.Context.set_host_wait(0, "poll")

    def med(key, field):
        return statistics.median(r[key][field] for r in rounds)

    a_all = [r[k]["proofs_per_s"] for r in rounds for k in ("A1", "A2")]
    a_med = statistics.median(a_all)
    spread = max(abs(r["A1"]["proofs_per_s"] - r["A2"]["proofs_per_s"]) for r in rounds)
    summary = {
        "A_proofs_per_s": a_med, "A_min": min(a_all), "A_max": max(a_all), "A_vs_A_spread_max": spread, "A_vs_A_spread_rel": spread / a_med,
        "B_proofs_per_s": med("B", "proofs_per_s"), "B_submit_wait_proofs_per_s": med("B_submit_wait", "proofs_per_s"),
        "C_proofs_per_s_spin_first": arm_c[0]["proofs_per_s"], "C_proofs_per_s_poll": arm_c[1]["proofs_per_s"], "C_proofs_per_s_spin_last": arm_c[2]["proofs_per_s"],
        "B_over_A": med("B", "proofs_per_s") / a_med, "B_over_C": med("B", "proofs_per_s") / arm_c[0]["proofs_per_s"],
        "B_minus_A_per_alternation": [r["B"]["proofs_per_s"] - 0.5 * (r["A1"]["proofs_per_s"] + r["A2"]["proofs_per_s"]) for r in rounds],
        "A_host_cpu_ms_per_proof": 1e3 * statistics.median(r[k]["host_cpu_s_per_proof"] for r in rounds for k in ("A1", "A2")),
        "B_host_cpu_ms_per_proof": 1e3 * med("B", "host_cpu_s_per_proof"),
        "A_host_cores_busy": statistics.median(r[k]["host_cores_busy"] for r in rounds for k in ("A1", "A2")),
        "B_host_cores_busy": med("B", "host_cores_busy"), "B_submit_wait_host_cores_busy": med("B_submit_wait", "host_cores_busy"),
    }
    result = {"tool": "tools/engine_ab.py", "device": torch.cuda.get_device_name(0), "m": m, "m_0": m_0, "k": K, "steps": args.steps, "warmup": args.warmup,
              "alternations": args.alternations, "host_wait": "poll (A, B); C as listed", "digests": digests, "summary": summary, "arm_c": arm_c, "rounds": rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"digests_equal": digests["equal"], **summary}))
    eng.close()
    lone.close()
    for c, s, _ in workers:
        s.close()
        c.close()
    r1cs.close()
    ctx0.close()
    return 0 if digests["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
