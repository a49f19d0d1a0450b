#!/usr/bin/env python3
"""pkw_evaluate against the route the product's public API offers for the same values -- q x (pk_eq_table + pk_dot) per polynomial --
and the wall time of pkw_commit / pkw_open.  Writes profiles/r12_whir_pcs.json.

    python tools/whir_pcs_bench.py [--out profiles/r12_whir_pcs.json] [--reps 7]

Every figure is host wall time of the blocking call (median of --reps after one warm-up), which is what a caller sees; the
evaluation's achieved bandwidth counts the bytes the kernel must read: batch * 2^n * 32 * ceil(q / 8).  Without a GPU the file is
written with null rates and says so."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
ACHIEVABLE_GBPS = 6300.0  # what the project takes as achievable HBM bandwidth on MI355X

from whir_pcs_helpers import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_whir_pcs.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="20,24")
    args = ap.parse_args()
    result = {"tool": "tools/whir_pcs_bench.py", "achievable_gbps": ACHIEVABLE_GBPS, "evaluate": [], "commit_open": []}
    try:
        import torch

        torch.cuda.is_available()
        import provekit_amd
        from provekit_amd import whir_pcs
        from provekit_amd._lib import lib
        from provekit_amd.field import random_field
        from provekit_amd.scheme import WhirConfig

        ctx = provekit_amd.Context(0)
    except Exception as e:  # no device: the shape of the file without figures
        result["measured_on_mi355x"] = False
        result["note"] = f"not run on a GPU ({type(e).__name__}: {e}); rates are null"
        for n in (20, 24):
            for batch in (1, 2):
                for q in (1, 8, 16):
                    result["evaluate"].append({"n_vars": n, "batch": batch, "q": q, "pkw_evaluate_ms": None, "eq_table_dot_ms": None, "ratio": None, "gbps": None})
        result["commit_open"].append({"n_vars": 20, "batch": 2, "q": 8, "commit_ms": None, "open_ms": None})
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    result["measured_on_mi355x"] = True
    for n in (int(x) for x in args.sizes.split(",")):
        N = 1 << n
        polys = [ctx.upload(random_field(N, 10 + b)) for b in range(2)]
        table = ctx.alloc_fe(N)
        out4 = np.zeros(4, dtype=np.uint64)
        for batch in (1, 2):
            for q in (1, 8, 16):
                pts = random_field(q * n, 7 * q + n).reshape(q, n, 4)

                def ours():
                    return whir_pcs.evaluate(ctx, polys[:batch], n, pts)

                def theirs():
                    vals = np.zeros((batch, q, 4), dtype=np.uint64)
                    for b in range(batch):
                        for i in range(q):
                            ctx._check(lib.pk_eq_table(ctx.handle, pts[i].ctypes.data, n, table.ptr))
                            ctx._check(lib.pk_dot(ctx.handle, table.ptr, polys[b].ptr, N, out4.ctypes.data))
                            vals[b, i] = out4
                    return vals

                assert np.array_equal(ours(), theirs()), "the two routes disagree"
                t_ours, min_ours = timed(ours, args.reps)
                t_theirs, _ = timed(theirs, max(3, args.reps // 2))
                passes = (q + 7) // 8
                row = {"n_vars": n, "batch": batch, "q": q, "pkw_evaluate_ms": round(1e3 * t_ours, 4), "pkw_evaluate_min_ms": round(1e3 * min_ours, 4),
                       "eq_table_dot_ms": round(1e3 * t_theirs, 4), "ratio": round(t_ours / t_theirs, 4),
                       "gbps": round(batch * N * 32 * passes / t_ours / 1e9, 1)}
                row["fraction_of_achievable"] = round(row["gbps"] / ACHIEVABLE_GBPS, 3)
                result["evaluate"].append(row)
                print(json.dumps(row), flush=True)
        if n == 20:
            cfg = WhirConfig.derive(n, batch_size=2)
            scheme = whir_pcs.Scheme(ctx, cfg)
            pts = random_field(8 * n, 5).reshape(8, n, 4)
            holder = {}

            def commit():
                if "c" in holder:
                    holder["c"].close()
                holder["c"] = scheme.commit(polys)

            t_commit, _ = timed(commit, args.reps)
            t_open, _ = timed(lambda: scheme.open(holder["c"], pts), args.reps)
            evals, proof = scheme.open(holder["c"], pts)
            ok = whir_pcs.verify(cfg, pts, proof, expected_root=holder["c"].root())[0].accepted
            row = {"n_vars": n, "batch": 2, "q": 8, "commit_ms": round(1e3 * t_commit, 3), "open_ms": round(1e3 * t_open, 3), "proof_bytes": len(proof),
                   "arena_bytes": whir_pcs.arena_bytes(cfg), "verified": bool(ok)}
            result["commit_open"].append(row)
            print(json.dumps(row), flush=True)
            holder["c"].close()
            scheme.close()
        for p in polys:
            p.free()
        table.free()
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
