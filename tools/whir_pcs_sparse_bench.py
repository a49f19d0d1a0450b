#!/usr/bin/env python3
"""Sparse weights (index/value lists) against the dense route on the densified tables of the SAME statement:

  sums          pkw_sparse_sums        against  pkw_weighted_sums
  accumulation  pkw_sparse_accumulate  against  linear.hip's combine kernel, accumulating (through tools/probes: it has no C ABI)
  evaluation    pkw_sparse_evaluate    against  pkw_evaluate over the l tables
  opening       pkw_open_sparse        against  pkw_open_linear
  verification  pkw_verify_sparse      against  pkw_verify_linear with the tables given (host only)

at n_vars = 20 and 22, batch 1 and 2, l = 4 weights of nnz = 2^10, 2^16, 2^n / 4 and 2^n entries each, and the density at which the dense
route overtakes the sparse one.  Writes profiles/r15_whir_pcs_sparse.json.

    python tools/whir_pcs_sparse_bench.py [--out profiles/r15_whir_pcs_sparse.json] [--reps 7] [--sizes 20,22]

A/B on one box in one process: per shape both sides are warmed, then timed ALTERNATING for --reps rounds.  Every figure is host wall
time of the blocking call(s), which is what a caller sees (the three kernel entry points allocate, validate the indexes, launch and
copy the result back; the dense ones allocate, launch and copy); each side's spread is (max - min) / median of its rounds.  The
outputs of the two routes are compared bit for bit before anything is timed.  Without a GPU the result's shape is printed with null
figures and no file is written."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
L_WEIGHTS = 4
OPS = ("sums", "accumulation", "evaluation", "opening", "verification")

from whir_pcs_helpers import ab, ptrs  # noqa: E402


def densities(n):
    return [1 << 10, 1 << 16, (1 << n) // 4, 1 << n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_whir_pcs_sparse.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="20,22")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    result = {"tool": "tools/whir_pcs_sparse_bench.py", "reps": args.reps, "l": L_WEIGHTS, "rows": [], "crossover": []}
    try:
        import torch

        torch.cuda.is_available()
        import pk_probes
        import provekit_amd
        from provekit_amd import whir_pcs
        from provekit_amd.field import random_field
        from provekit_amd.scheme import WhirConfig

        ctx = provekit_amd.Context(0)
    except Exception as e:  # no device: the shape of the file without figures
        result["measured_on_mi355x"] = False
        result["note"] = f"not run on a GPU ({type(e).__name__}: {e}); every figure is null"
        for n in sizes:
            for batch in (1, 2):
                for nnz in densities(n):
                    result["rows"].append({"n_vars": n, "batch": batch, "nnz": nnz, **{op: None for op in OPS}})
        print(json.dumps(result))  # no file: profiles/ holds measurements only
        return
    result["measured_on_mi355x"] = True
    probes = pk_probes.lib
    for n in sizes:
        N = 1 << n
        rng = np.random.default_rng(n)
        polys = [random_field(N, 10 + b) for b in range(2)]
        d_polys = [ctx.upload(p) for p in polys]
        point, tags, scales = random_field(n, 3), random_field(L_WEIGHTS, 4), random_field(L_WEIGHTS, 5)
        table = ctx.upload(random_field(N, 6))
        for nnz in densities(n):
            lists, dense = [], []
            for i in range(L_WEIGHTS):
                idx = np.arange(N, dtype=np.uint32) if nnz == N else np.sort(rng.choice(N, size=nnz, replace=False)).astype(np.uint32)
                val = random_field(nnz, 100 + i)
                t = np.zeros((N, 4), dtype=np.uint64)
                t[idx] = val
                lists.append((idx, val))
                dense.append(t)
            sw = whir_pcs.SparseWeights(lists).upload(ctx)
            d_w = [ctx.upload(t) for t in dense]
            for batch in (1, 2):
                f = d_polys[:batch]
                row = {"n_vars": n, "batch": batch, "nnz": nnz, "density": nnz / N}

                def dense_accumulate():
                    ctx._check(probes.pk_probe_whir_combine(ctx.handle, table.ptr, N, ptrs(d_w), scales.ctypes.data, L_WEIGHTS, 1))

                def dense_evaluate():
                    return whir_pcs.evaluate(ctx, d_w, n, point.reshape(1, n, 4))[:, 0]

                kernels = {
                    "sums": (lambda: whir_pcs.sparse_sums(ctx, f, n, sw), lambda: whir_pcs.weighted_sums(ctx, f, n, d_w)),
                    "accumulation": (lambda: whir_pcs.sparse_accumulate(ctx, table, n, sw, scales), dense_accumulate),
                    "evaluation": (lambda: whir_pcs.sparse_evaluate(ctx, n, sw, point), dense_evaluate),
                }
                assert np.array_equal(kernels["sums"][0](), kernels["sums"][1]()), "the two sums disagree"
                assert np.array_equal(kernels["evaluation"][0](), kernels["evaluation"][1]()), "the two evaluations disagree"
                before = ctx.download_fe(table.ptr, N)
                kernels["accumulation"][0]()
                a = ctx.download_fe(table.ptr, N)
                ctx.upload_into(table.ptr, before)
                kernels["accumulation"][1]()
                assert np.array_equal(a, ctx.download_fe(table.ptr, N)), "the two accumulations disagree"
                if batch == 1:  # the accumulation and the evaluation do not see the polynomials: measured once per density
                    for op in ("accumulation", "evaluation"):
                        row[op] = ab({"sparse": kernels[op][0], "dense": kernels[op][1]}, args.reps)
                row["sums"] = ab({"sparse": kernels["sums"][0], "dense": kernels["sums"][1]}, args.reps)

                cfg = WhirConfig.derive(n, batch_size=batch)
                scheme = whir_pcs.Scheme(ctx, cfg)
                com = scheme.commit(f)
                root = com.root()
                sparse_open = scheme.open_sparse(com, None, sw, tags)
                dense_open = scheme.open_linear(com, None, d_w, tags)
                assert sparse_open[2] == dense_open[2], "the two openings disagree"
                proof = sparse_open[2]
                row["proof_bytes"] = len(proof)
                row["opening"] = ab({"sparse": lambda: scheme.open_sparse(com, None, sw, tags), "dense": lambda: scheme.open_linear(com, None, d_w, tags)}, args.reps)
                vs = whir_pcs.verify_sparse(cfg, None, tags, sw, proof, expected_root=root)
                vd = whir_pcs.verify_linear(cfg, None, tags, dense, proof, expected_root=root)
                assert vs.result.accepted and vd.result.accepted and vd.unchecked == 0 and np.array_equal(vs.deferred, vd.deferred)
                row["verification"] = ab({"sparse": lambda: whir_pcs.verify_sparse(cfg, None, tags, sw, proof, expected_root=root),
                                          "dense": lambda: whir_pcs.verify_linear(cfg, None, tags, dense, proof, expected_root=root)}, max(3, args.reps // 2))
                com.close()
                scheme.close()
                for op in OPS:
                    if op in row:
                        row[op]["sparse_over_dense"] = round(row[op]["sparse"]["median_ms"] / row[op]["dense"]["median_ms"], 4)
                result["rows"].append(row)
                print(json.dumps(row), flush=True)
            for x in d_w + [sw]:
                x.free()
        for x in d_polys + [table]:
            x.free()
    # the crossover: between which two measured densities the dense route overtakes the sparse one, per size, batch and operation
    for n in sizes:
        for batch in (1, 2):
            rows = [r for r in result["rows"] if r["n_vars"] == n and r["batch"] == batch]
            for op in OPS:
                have = [(r["density"], r[op]["sparse_over_dense"]) for r in rows if op in r]
                if not have:
                    continue
                wins = [d for d, ratio in have if ratio < 1.0]
                loses = [d for d, ratio in have if ratio >= 1.0]
                result["crossover"].append({"n_vars": n, "batch": batch, "op": op, "sparse_faster_up_to_density": max(wins) if wins else None,
                                            "dense_faster_from_density": min(loses) if loses else None, "sparse_over_dense_at_full": have[-1][1]})
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result["crossover"]))


if __name__ == "__main__":
    main()
