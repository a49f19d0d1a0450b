#!/usr/bin/env python3
"""The sharded product sumcheck (provekit_amd.prodcheck_sharded) round by round: eq (a b - c) over three tables of 2^n on G ranks of
ONE GPU (the in-process transport, one host thread per rank), against the lone prover on the same device.  Writes
profiles/r23_sumcheck_sharded_profile.json.

    python tools/sumcheck_sharded_profile.py [--out ...] [--reps 5] [--sizes 20,22,24] [--worlds 2,4,8]

Per (n, G): per rank and per sharded round the pairs its launch covered (pkss_last_profile: the launch argument) and the bytes that
launch reads -- m tables at 2 (round 0) or 4 (with a fold) elements per pair, plus the split eq entries -- next to the lone prover's
for the same round, and their ratio (1/G by the ownership rule); the time of the slice and of the exchange behind it; the hand-over;
the replicated rounds; and the replicated share of the whole proof's time.  Times are host wall time of blocking steps, the median
over the repetitions after one warm-up, taken on every rank.

WHAT THE TIMES ARE NOT: G ranks on one GPU share its memory bandwidth and run their kernels one after another on one queue, so a
rank's slice here is not faster than the lone round, and the total says nothing about scaling over G devices.  No multi-GPU run of
this library exists: its speed-up is unmeasured.  The byte counts and the shares of the rounds are what this file is for.
Without a GPU the file is written with null times and says so."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M, D = 3, 2


def round_read_bytes(n, i, pairs):
    """what a launch over `pairs` pairs of round i reads: the tables, and the split eq tables' entries of the round"""
    per_pair = 2 if i == 0 else 4
    R = n - 1
    L = R // 2
    H = R - L
    hi_bits, lo_bits = (H - i, L) if i <= H else (0, R - i)
    return M * 32 * per_pair * pairs + 32 * ((1 << hi_bits) + (1 << lo_bits))


def statement(n):
    from provekit_amd import prodcheck

    return prodcheck.Statement(n, M, [(1, 0b011), (P - 1, 0b100)], has_tau=True)


def run_set(n, G, tables, tau, reps):
    """-> per rank: the median profile over reps proofs"""
    import provekit_amd
    from provekit_amd import prodcheck_sharded

    ctxs = provekit_amd.Context.create_set([0] * G)
    out, err = [None] * G, []

    def rank(r):
        try:
            c = ctxs[r]
            d = [c.upload(t) for t in tables]
            prover = prodcheck_sharded.Prover(c, statement(n))
            prover.prove(d, tau)
            runs = []
            for _ in range(reps):
                proof = prover.prove(d, tau)
                runs.append(prover.last_profile())
            med = lambda f: statistics.median(f(x) for x in runs)  # noqa: E731
            out[r] = {"proof": proof.bytes, "total_s": med(lambda x: x["total_s"]), "handover_s": med(lambda x: x["handover_s"]),
                      "rounds": [{"sharded": runs[0]["rounds"][i]["sharded"], "pairs": runs[0]["rounds"][i]["pairs"],
                                  "round_s": med(lambda x: x["rounds"][i]["round_s"]), "exchange_s": med(lambda x: x["rounds"][i]["exchange_s"])}
                                 for i in range(n)]}
            prover.close()
            for b in d:
                b.free()
        except BaseException as e:  # noqa: BLE001
            err.append(e)

    ths = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=600)
    if err:
        raise err[0]
    if any(t.is_alive() for t in ths):
        raise RuntimeError("a rank did not come back")
    for c in ctxs:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_sumcheck_sharded_profile.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--worlds", default="2,4,8")
    args = ap.parse_args()
    sizes, worlds = [int(x) for x in args.sizes.split(",")], [int(x) for x in args.worlds.split(",")]
    result = {"tool": "tools/sumcheck_sharded_profile.py", "statement": "eq (a b - c), m = 3, D = 2", "reps": args.reps,
              "ranks_share_one_gpu": True, "multi_gpu_speedup": "unmeasured", "cases": []}
    try:
        import torch

        torch.cuda.is_available()
        import provekit_amd
        from provekit_amd import prodcheck, prodcheck_sharded
        from provekit_amd.field import random_field

        ctx = provekit_amd.Context(0)
    except Exception as e:  # no device: the byte counts alone, from the plan
        from provekit_amd import prodcheck_sharded

        result["measured_on_mi355x"] = False
        result["note"] = f"not run on a GPU ({type(e).__name__}: {e}); times are null, pairs are the plan's"
        for n in sizes:
            for G in worlds:
                p = prodcheck_sharded.plan(statement(n), G)
                rounds = [{"round": i, "rank_read_bytes": round_read_bytes(n, i, (1 << (n - 1 - i)) >> p.g), "lone_read_bytes": round_read_bytes(n, i, 1 << (n - 1 - i))}
                          for i in range(p.S)]
                result["cases"].append({"n": n, "G": G, "S": p.S, "arena_bytes": p.arena_bytes, "lone_arena_table_bytes": M * 32 << (n - 1), "total_ms": None,
                                        "sharded_rounds": rounds[:3]})
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    result["measured_on_mi355x"] = True
    for n in sizes:
        N = 1 << n
        tables = [random_field(N, 40 + j) for j in range(M)]
        tau = random_field(n, 50)
        d = [ctx.upload(t) for t in tables]
        lone = prodcheck.Prover(ctx, statement(n))
        want = lone.prove(d, tau).bytes
        lone_s = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            lone.prove(d, tau)
            lone_s.append(time.perf_counter() - t0)
        lone.close()
        for b in d:
            b.free()
        for G in worlds:
            p = prodcheck_sharded.plan(statement(n), G)
            ranks = run_set(n, G, tables, tau, args.reps)
            assert all(r["proof"] == want for r in ranks), "a rank's bytes are not the lone prover's"
            rounds = []
            for i in range(p.S):
                assert all(r["rounds"][i]["sharded"] and r["rounds"][i]["pairs"] == (1 << (n - 1 - i)) >> p.g for r in ranks)
                mine, whole = round_read_bytes(n, i, ranks[0]["rounds"][i]["pairs"]), round_read_bytes(n, i, 1 << (n - 1 - i))
                rounds.append({"round": i, "pairs_per_rank": ranks[0]["rounds"][i]["pairs"], "rank_read_bytes": mine, "lone_read_bytes": whole,
                               "ratio": round(mine / whole, 5), "slice_ms_per_rank": [round(1e3 * r["rounds"][i]["round_s"], 4) for r in ranks],
                               "exchange_ms_per_rank": [round(1e3 * r["rounds"][i]["exchange_s"], 4) for r in ranks]})
            total = statistics.median(r["total_s"] for r in ranks)
            replicated = statistics.median(sum(x["round_s"] for x in r["rounds"][p.S:]) for r in ranks)
            exchanges = statistics.median(sum(x["exchange_s"] for x in r["rounds"][: p.S]) for r in ranks)
            handover = statistics.median(r["handover_s"] for r in ranks)
            result["cases"].append({
                "n": n, "G": G, "S": p.S, "arena_bytes": p.arena_bytes, "lone_arena_table_bytes": M * 32 << (n - 1),
                "total_ms": round(1e3 * total, 4), "lone_total_ms": round(1e3 * statistics.median(lone_s), 4),
                "sharded_slices_ms": round(1e3 * statistics.median(sum(x["round_s"] for x in r["rounds"][: p.S]) for r in ranks), 4),
                "exchanges_ms": round(1e3 * exchanges, 4), "handover_ms": round(1e3 * handover, 4), "replicated_rounds_ms": round(1e3 * replicated, 4),
                "replicated_share": round((replicated + handover) / total, 4),
                "sharded_read_bytes_per_rank": sum(r["rank_read_bytes"] for r in rounds), "sharded_read_bytes_lone": sum(r["lone_read_bytes"] for r in rounds),
                "sharded_rounds": rounds})
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "cases"}))
    for c in result["cases"]:
        print(json.dumps({k: v for k, v in c.items() if k != "sharded_rounds"}))


if __name__ == "__main__":
    main()
