#!/usr/bin/env python3
"""Proofs verified per second at the bench statement (m = 21, the reference's derived schedule): the compiled verifier's host core on
one thread, its device path at K = 1, 16, 64 proofs per call and -- where asked for, it is pure Python -- oracle/verifier.py on the same
proofs as the yardstick.  Every arm must give the same verdicts: the digest of (accepted, check) over the proofs all arms saw is
compared.  Writes profiles/r11_verify.json.

    python tools/verify_bench.py [--m 21] [--proofs 64] [--host-proofs 8] [--oracle-proofs 0] [--out profiles/r11_verify.json]

The driver starts every GPU step as a process of its own under `timeout -k 10`, chained with &&; nothing uses more than 16 threads."""
import argparse
import hashlib
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
os.environ.setdefault("OMP_NUM_THREADS", "16")


def digest(results):
    return hashlib.sha256(repr([(bool(r.accepted), r.check) for r in results]).encode()).hexdigest()[:16]


def statement(ctx, m):
    import bench
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for

    m_0 = m - 1
    n_wit = (1 << (m - 1)) - 5
    r1cs, mats, interner, nc, n_in = bench.synth_r1cs(ctx, m_0, n_wit, seed=1234)
    scheme = WhirR1CSScheme(ctx, r1cs, m, m_0, WhirConfig.derive(m), blinding_config_for(m_0))
    return r1cs, mats, interner, nc, n_in, n_wit, scheme


def step_prove(a, work):
    import bench
    import provekit_amd

    ctx = provekit_amd.Context(0)
    r1cs, mats, interner, nc, n_in, n_wit, scheme = statement(ctx, a.m)
    d_z, _ = bench.satisfying_witness(ctx, r1cs, n_wit, nc, n_in, 99)
    proofs = [scheme.prove(d_z, seed=1000 + i) for i in range(a.proofs)]
    for i in range(3, a.proofs, 7):  # a few tampered members, so that the verdict digest says something
        t = bytearray(proofs[i])
        t[(len(t) * (i % 5 + 1)) // 7] ^= 1
        proofs[i] = bytes(t)
    pickle.dump(dict(proofs=proofs, ds=scheme.domain_separator), open(os.path.join(work, "proofs.pkl"), "wb"))
    print(f"proved {len(proofs)} proofs of {len(proofs[0])} bytes")


def make_verifier(a, ctx, work, attach):
    from provekit_amd.verify import Verifier

    r1cs, mats, interner, nc, n_in, n_wit, scheme = statement(ctx, a.m)
    d = pickle.load(open(os.path.join(work, "proofs.pkl"), "rb"))
    v = Verifier.for_scheme(scheme, mats, interner, attach=attach)
    return v, d["proofs"], (scheme, mats, interner, nc, n_wit)


def step_host(a, work):
    import provekit_amd

    ctx = provekit_amd.Context(0)  # only to build the statement's matrices the way bench.py does
    v, proofs, _ = make_verifier(a, ctx, work, attach=False)
    sub = proofs[: a.host_proofs]
    t0 = time.perf_counter()
    res = [v.verify(p) for p in sub]
    dt = time.perf_counter() - t0
    json.dump(dict(arm="host_core_1_thread", proofs=len(sub), seconds=round(dt, 4), proofs_per_s=round(len(sub) / dt, 3), digest=digest(res),
                   accepted=sum(r.accepted for r in res)), open(os.path.join(work, "host.json"), "w"))


def step_device(a, work):
    import provekit_amd

    ctx = provekit_amd.Context(0)
    v, proofs, _ = make_verifier(a, ctx, work, attach=True)
    out = []
    v.verify_many(proofs[:1])  # first call: buffers are allocated
    for K in (1, 16, 64):
        if K > len(proofs):
            continue
        best, res = None, None
        for _ in range(3):
            t0 = time.perf_counter()
            res = []
            for s in range(0, len(proofs) - K + 1, K):
                res += v.verify_many(proofs[s : s + K])
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out.append(dict(arm=f"device_K{K}", proofs=len(res), seconds=round(best, 4), proofs_per_s=round(len(res) / best, 2),
                        digest=digest(res[: a.host_proofs]), digest_all=digest(res), accepted=sum(r.accepted for r in res)))
    json.dump(out, open(os.path.join(work, "device.json"), "w"))


def step_oracle(a, work):
    import oracle_lib as oracle
    import provekit_amd
    import verifier as V

    ctx = provekit_amd.Context(0)
    _, proofs, (scheme, mats, interner, nc, n_wit) = make_verifier(a, ctx, work, attach=False)

    def vcfg(c):
        return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, c.num_queries, c.ood_samples, c.pow_bits,
                            c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)

    class R:
        def __init__(self, ok):
            self.accepted, self.check = ok, None

    ev = oracle.matrix_evaluator(nc, n_wit, [(M.new_row_indices, M.col_indices, M.values) for M in mats], interner)
    sub = proofs[: a.oracle_proofs]
    t0 = time.perf_counter()
    ok = []
    for p in sub:
        try:
            ok.append(bool(V.verify(p, scheme.domain_separator, a.m, a.m - 1, vcfg(scheme.whir_witness), vcfg(scheme.whir_for_hiding_spartan), r1cs=ev)))
        except V.VerifyError:
            ok.append(False)
    dt = time.perf_counter() - t0
    json.dump(dict(arm="oracle_python", proofs=len(sub), seconds=round(dt, 3), proofs_per_s=round(len(sub) / dt, 4), verdicts=ok),
              open(os.path.join(work, "oracle.json"), "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=21)
    ap.add_argument("--proofs", type=int, default=64)
    ap.add_argument("--host-proofs", type=int, default=8)
    ap.add_argument("--oracle-proofs", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_verify.json"))
    ap.add_argument("--step")
    ap.add_argument("--work")
    a = ap.parse_args()
    if a.step:
        return {"prove": step_prove, "host": step_host, "device": step_device, "oracle": step_oracle}[a.step](a, a.work)
    work = tempfile.mkdtemp(prefix="verify_bench_")
    common = f"--m {a.m} --proofs {a.proofs} --host-proofs {a.host_proofs} --oracle-proofs {a.oracle_proofs} --work {work}"
    steps = [("prove", 300), ("host", 300), ("device", 300)] + ([("oracle", 900)] if a.oracle_proofs else [])
    cmd = " && ".join(f"timeout -k 10 {limit} {sys.executable} {os.path.abspath(__file__)} --step {name} {common}" for name, limit in steps)
    rc = subprocess.call(cmd, shell=True)
    if rc:
        sys.exit(f"a step failed or ran out of time (exit status {rc}); nothing was written")
    host = json.load(open(os.path.join(work, "host.json")))
    device = json.load(open(os.path.join(work, "device.json")))
    arms = [host] + device
    note = "oracle/verifier.py: not measured (pure Python; pass --oracle-proofs N)"
    if a.oracle_proofs:
        o = json.load(open(os.path.join(work, "oracle.json")))
        arms.append(o)
        note = "oracle/verifier.py measured on the first %d proofs" % o["proofs"]
    same = len({x["digest"] for x in arms if "digest" in x}) == 1 and len({x["digest_all"] for x in device}) == 1
    result = dict(tool="tools/verify_bench.py", m=a.m, m_0=a.m - 1, proofs=a.proofs, tampered_members=len(range(3, a.proofs, 7)), arms=arms,
                  verdict_digests_equal=same, note=note)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))
    if not same:
        sys.exit("the arms disagree on a verdict")


if __name__ == "__main__":
    main()
