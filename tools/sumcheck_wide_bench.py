#!/usr/bin/env python3
"""The wide product sumcheck (pksw_prove, csrc/sumcheck/wide.hip) measured on one device.  Writes profiles/r37_sumcheck_wide_bench.json.

    python tools/sumcheck_wide_bench.py [--out profiles/r37_sumcheck_wide_bench.json] [--reps 9] [--sizes 20,22,24]

(a) the two statements both interfaces state -- `r1cs`, eq (a b - c), and `four`, four terms over four tables at degree 3 -- through
    pksw_prove and through the unchanged pks_prove, alternating after one warm-up each: the ratio tells a user which interface to pick
    when both fit.  The wide route re-reads a table per term and is specialised on the degree only; it is expected to lose.
(b) the statements only the wide interface states -- the Plonk gate (8 tables, 5 terms, degree 3), x^5 (1 table) and 16 tables in 16
    terms -- with their algorithmic bytes and GB/s, next to pks_prove's figure at the same n from (a).

Every figure is host wall time of one blocking prove call, transcript included; medians, minima and the spread (max - min) / median over
the repetitions.  Algorithmic bytes are computed from the shapes: round 0 reads every table once at its length, each later round reads
every table once at its length and writes it once at half.  The tables are distinct device buffers (two random uploads copied on the
device), so that a table read a second time in a round comes from cache only where the kernel's own re-read does.  Without a GPU a
file of null times is written only to an --out other than the default: the measured profile is never overwritten."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r37_sumcheck_wide_bench.json")

# name -> (m, [(coefficient, [tables])], the same statement's masks for pks_prove or None)
BOTH = {
    "r1cs": (3, [(1, [0, 1]), (P - 1, [2])], [0b011, 0b100]),
    "four": (4, [(3, [0, 1, 2]), (P - 5, [1, 2, 3]), (1, [0, 3]), (7, [2])], [0b0111, 0b1110, 0b1001, 0b0100]),
}
WIDE_ONLY = {
    "plonk": (8, [(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (1, [3, 7]), (1, [4])], None),
    "pow5": (1, [(1, [0, 0, 0, 0, 0])], None),
    "wide16": (16, [(3, [0])] + [((1, P - 1, 5)[t % 3], [0, t]) for t in range(1, 16)], None),
}


def algorithmic_bytes(n, m):
    total = 0
    for i in range(n):
        length = 1 << (n - i) if i == 0 else 1 << (n - i + 1)
        total += m * (32 * length if i == 0 else 32 * (length + length // 2))
    return total


def table_reads_per_round(terms):
    """how often the wide kernel loads a table's pair per round: once per term it stands in (a power is loaded once)"""
    return sum(len(set(f)) for _, f in terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="20,22,24")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    result = {"tool": "tools/sumcheck_wide_bench.py", "reps": args.reps, "sizes": []}
    import torch

    torch.cuda.is_available()
    import provekit_amd
    from provekit_amd import prodcheck, prodcheck_wide
    from provekit_amd._lib import ProveKitHipError, lib
    from provekit_amd.field import random_field

    try:
        ctx = provekit_amd.Context(0)
    except ProveKitHipError as e:  # no device: the shape of the file without figures, never over the measured profile
        if os.path.abspath(args.out) == DEFAULT_OUT:
            sys.exit(f"no device ({e}): not overwriting {DEFAULT_OUT}; pass --out to write a file of null times elsewhere")
        result["measured_on_mi355x"] = False
        result["note"] = f"not run on a GPU ({e}); times are null"
        for n in sizes:
            result["sizes"].append({"n": n, "statements": {name: {"m": m, "T": len(terms), "algorithmic_bytes": algorithmic_bytes(n, m), "wide_ms": None}
                                                           for name, (m, terms, _) in {**BOTH, **WIDE_ONLY}.items()}})
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    result["measured_on_mi355x"] = True
    for n in sizes:
        N = 1 << n
        seeds = [ctx.upload(random_field(N, 60 + j)) for j in range(2)]
        tables = [ctx.alloc_fe(N) for _ in range(16)]
        for j, t in enumerate(tables):
            ctx._check(lib.pk_memcpy_d2d(ctx.handle, t.ptr, seeds[j % 2].ptr, 32 * N))
        ctx.sync()
        tau = random_field(n, 70)
        row = {"n": n, "statements": {}}
        for name, (m, terms, masks) in {**BOTH, **WIDE_ONLY}.items():
            wide = prodcheck_wide.Prover(ctx, prodcheck_wide.Statement(n, m, terms, has_tau=True))
            narrow = prodcheck.Prover(ctx, prodcheck.Statement(n, m, [(c, mask) for (c, _), mask in zip(terms, masks)], has_tau=True)) if masks else None
            sides = {"wide": wide} if narrow is None else {"wide": wide, "pks": narrow}

            def once(prover):
                t0 = time.perf_counter()
                prover.prove(tables[:m], tau)
                return time.perf_counter() - t0

            for p in sides.values():
                once(p)
            t = {k: [] for k in sides}
            for _ in range(args.reps):  # alternating: both sides see the same box at the same time
                for k, p in sides.items():
                    t[k].append(once(p))
            alg = algorithmic_bytes(n, m)
            entry = {"m": m, "T": len(terms), "D": max(len(f) for _, f in terms), "table_loads_per_pair": table_reads_per_round(terms), "algorithmic_bytes": alg}
            for k, v in t.items():
                med = statistics.median(v)
                entry[k + "_ms"] = round(1e3 * med, 4)
                entry[k + "_min_ms"] = round(1e3 * min(v), 4)
                entry[k + "_spread"] = round((max(v) - min(v)) / med, 3)
                entry[k + "_algorithmic_gbps"] = round(alg / med / 1e9, 1)
            if narrow is not None:
                entry["wide_over_pks"] = round(statistics.median(t["wide"]) / statistics.median(t["pks"]), 3)
                narrow.close()
            wide.close()
            row["statements"][name] = entry
        result["sizes"].append(row)
        for b in seeds + tables:
            b.free()
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
