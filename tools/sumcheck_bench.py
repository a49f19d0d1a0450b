#!/usr/bin/env python3
"""One whole R1CS-shape sumcheck -- eq (a b - c) over three tables of 2^n, all n rounds -- through libprovekit_sumcheck.so's generic
kernel (pks_prove, transcript included) against the product's own specialised kernel for the same statement: pk_sumcheck_cubic_round
driven over the same n rounds with pk_eq_table's table as its eq array (no transcript: its challenges are fixed elements).  Writes
profiles/r21_sumcheck_bench.json.

    python tools/sumcheck_bench.py [--out profiles/r21_sumcheck_bench.json] [--reps 9] [--sizes 20,22,24]

Both sides run in one process on one device, alternating, after one warm-up each; every figure is host wall time of blocking calls
(each round ends in a device synchronise).  The specialised side folds its arrays in place, so each repetition starts from fresh
device copies made outside the timed window.  The bytes are computed from the shapes: per folding round the algorithm moves
m * 32 * (len + len/2) (each table read once at its length, written once at half); the generic kernel adds the two split eq tables
and the workgroups' partial sums, the specialised one a fourth array (the folded eq table).  Without a GPU the file is written with
null times and says so."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def round_bytes(n, m=3, D=2):
    """per round: (len the round reads, algorithmic bytes, generic kernel bytes, specialised kernel bytes)"""
    rows = []
    for i in range(n):
        pairs = 1 << (n - 1 - i)
        length = 2 * pairs if i == 0 else 4 * pairs
        moved = 32 * length if i == 0 else 32 * (length + length // 2)
        R = n - 1
        L = R // 2
        H = R - L
        hi_bits, lo_bits = (H - i, L) if i <= H else (0, R - i)
        grid = min(max((pairs + 511) // 512, 1), 1024)
        generic = m * moved + 32 * ((1 << hi_bits) + (1 << lo_bits)) + 2 * 32 * (D + 1) * grid
        rows.append({"round": i, "len": length, "algorithmic_bytes": m * moved, "generic_kernel_bytes": generic, "specialised_kernel_bytes": (m + 1) * moved})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_sumcheck_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="20,22,24")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    result = {"tool": "tools/sumcheck_bench.py", "statement": "eq (a b - c), m = 3, D = 2", "reps": args.reps, "sizes": []}
    try:
        import torch

        torch.cuda.is_available()
        import provekit_amd
        from provekit_amd import prodcheck
        from provekit_amd import sumcheck as S
        from provekit_amd._lib import lib
        from provekit_amd.field import random_field

        ctx = provekit_amd.Context(0)
    except Exception as e:  # no device: the shape of the file without figures
        result["measured_on_mi355x"] = False
        result["note"] = f"not run on a GPU ({type(e).__name__}: {e}); times are null"
        for n in sizes:
            rows = round_bytes(n)
            result["sizes"].append({"n": n, "generic_ms": None, "specialised_ms": None, "ratio": None, "algorithmic_bytes": sum(r["algorithmic_bytes"] for r in rows),
                                    "rounds": rows[:3]})
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    result["measured_on_mi355x"] = True
    for n in sizes:
        N = 1 << n
        src = [ctx.upload(random_field(N, 40 + j)) for j in range(3)]
        tau = random_field(n, 50)
        folds = random_field(n, 51)
        stmt = prodcheck.Statement(n, 3, [(1, 0b011), (P - 1, 0b100)], has_tau=True)
        prover = prodcheck.Prover(ctx, stmt)
        work = [ctx.alloc_fe(N) for _ in range(4)]

        def generic():
            t0 = time.perf_counter()
            prover.prove(src, tau)
            return time.perf_counter() - t0

        def specialised():
            for w, s in zip(work, src):  # the rounds fold in place: fresh copies, outside the timed window
                ctx._check(lib.pk_memcpy_d2d(ctx.handle, w.ptr, s.ptr, 32 * N))
            ctx.sync()
            t0 = time.perf_counter()
            S.calculate_evaluations_over_boolean_hypercube_for_eq(ctx, tau, work[3])
            S.sumcheck_fold_map_reduce(ctx, work[0], work[1], work[2], work[3], N)
            for i in range(1, n):
                S.sumcheck_fold_map_reduce(ctx, work[0], work[1], work[2], work[3], N >> (i - 1), folds[i - 1])
            return time.perf_counter() - t0

        generic(), specialised()
        t = {"generic": [], "specialised": []}
        for _ in range(args.reps):  # alternating: both sides see the same box at the same time
            t["generic"].append(generic())
            t["specialised"].append(specialised())
        rows = round_bytes(n)
        algorithmic = sum(r["algorithmic_bytes"] for r in rows)
        g, s = statistics.median(t["generic"]), statistics.median(t["specialised"])
        spread = {k: round((max(v) - min(v)) / statistics.median(v), 3) for k, v in t.items()}
        result["sizes"].append({
            "n": n, "generic_ms": round(1e3 * g, 4), "specialised_ms": round(1e3 * s, 4), "ratio": round(g / s, 3),
            "generic_min_ms": round(1e3 * min(t["generic"]), 4), "specialised_min_ms": round(1e3 * min(t["specialised"]), 4), "spread": spread,
            "algorithmic_bytes": algorithmic, "generic_kernel_bytes": sum(r["generic_kernel_bytes"] for r in rows),
            "specialised_kernel_bytes": sum(r["specialised_kernel_bytes"] for r in rows) + 32 * N,  # ... and pk_eq_table writes its table once
            "generic_algorithmic_gbps": round(algorithmic / g / 1e9, 1), "rounds": rows[:3]})
        prover.close()
        for b in src + work:
            b.free()
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
