#!/usr/bin/env python3
"""What a memory check costs on one device (libprovekit_memcheck.so), per (n, k), in runs that alternate between the ways compared on
the same tables.  Medians with the spread (min .. max) of `--reps` runs after one warm-up; the warm-up's proof is verified.

  (a) pkm_prove against the sum of its three inner calls timed by themselves in the same run -- pkf_prove (n + 1), pkf_prove (k + 1),
      pkf_lookup_prove (n, n) on the very tables pkm_prove forms (pkm_leaves writes them out): the difference is what the leaves, the
      staging and the comparison cost;
  (b) pkm_trace split into key, sort, resolve and count (device events), with the TB/s of the bytes the resolve and the leaf passes
      move; for scale tuple_leaf_kernel (w = 4) and the fractional sum's tree kernels on 2^n rows in the same run;
  (c) the route a caller has without this library: four pkg_prove calls on leaf tables of the same sizes (write set, read set, init set,
      final set) plus one pkf_lookup_prove, against pkm_prove; `separated` says whether the two spreads overlap.

usage: python tools/memcheck_bench.py [--sizes 16:12,20:16,24:20] [--reps 5] [--out profiles/r32_memcheck_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import provekit_amd  # noqa: E402
from provekit_amd import fracsum as fs, grandproduct as gp, memcheck as mc  # noqa: E402
from provekit_amd._lib import lib as product  # noqa: E402
from provekit_amd.field import random_field  # noqa: E402
from tools.pk_probes import lib as probes  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def separated(a, b):
    return a["max"] < b["min"] or b["max"] < a["min"]


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def profile(prover):
    trace_ms, leaf_ms, side_ms = (C.c_double * 4)(), C.c_double(), (C.c_double * 3)()
    assert probes.pk_probe_mem_profile(prover.handle, trace_ms, C.byref(leaf_ms), side_ms) == 0
    out = dict(zip(("key_ms", "sort_ms", "resolve_ms", "count_ms"), trace_ms))
    out.update(leaf_ms=leaf_ms.value, side_ops_ms=side_ms[0], side_mem_ms=side_ms[1], side_time_ms=side_ms[2])
    return out


def small(ctx, values):
    """a device column of small integers as Montgomery elements"""
    limbs = np.zeros((len(values), 4), dtype=np.uint64)
    limbs[:, 0] = values
    buf = ctx.upload(limbs)
    assert product.pk_fe_to_mont(ctx.handle, buf.ptr, buf.ptr, len(values)) == 0
    return buf


def signs(ctx, v):
    """+1 on the first 2^v entries, -1 on the second"""
    from provekit_amd.prodcheck import P, _R

    def image(x):
        return np.array([((x * _R % P) >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)

    table = np.empty((2 << v, 4), dtype=np.uint64)
    table[: 1 << v], table[1 << v :] = image(1), image(P - 1)
    return ctx.upload(table)


def run(ctx, n, k, reps):
    rows, cells = 1 << n, 1 << k
    rng = np.random.default_rng(n)
    d_addr = ctx.upload(rng.integers(0, cells, size=rows, dtype=np.uint32))
    d = {"wv": ctx.upload(random_field(rows, 1).reshape(-1, 4)), "init": ctx.upload(random_field(cells, 2).reshape(-1, 4))}
    for name in ("a", "rv", "rt", "m"):
        d[name] = ctx.alloc_fe(rows)
    for name in ("fin", "ft"):
        d[name] = ctx.alloc_fe(cells)
    stmt = mc.Statement(n, k, 2)
    prover = mc.Prover(ctx, stmt)
    bind = random_field(2, 3).reshape(-1, 4)

    def trace():
        prover.trace(d_addr, d["wv"], d["init"], d["a"], d["rv"], d["rt"], d["fin"], d["ft"], d["m"])

    trace()
    # the inner statements' own provers on the tables pkm_prove forms: gamma and beta are the proof's
    _, claims = prover.prove(d, bind)
    d_q_ops, d_q_mem, d_f = ctx.alloc_fe(2 * rows), ctx.alloc_fe(2 * cells), ctx.alloc_fe(rows)
    mc.leaves(ctx, n, k, d, claims.gamma, claims.beta, d_q_ops, d_q_mem, d_f)
    d_sign_ops, d_sign_mem, d_t = signs(ctx, n), signs(ctx, k), small(ctx, np.arange(rows, dtype=np.uint64))
    seed = random_field(1, 4).reshape(-1, 4)
    sum_ops, sum_mem = fs.FractionalSumProver(ctx, fs.Statement(n + 1, 1, 0)), fs.FractionalSumProver(ctx, fs.Statement(k + 1, 1, 0))
    look = fs.LookupProver(ctx, fs.LookupStatement(n, n, 1))
    # today's route: a grand product per set, on leaf tables of the sets' sizes (the halves of the stacked tables)
    prod_n, prod_k = gp.GrandProductProver(ctx, gp.Statement(n, 1)), gp.GrandProductProver(ctx, gp.Statement(k, 1))
    halves = [(prod_n, d_q_ops.ptr), (prod_n, d_q_ops.ptr + 32 * rows), (prod_k, d_q_mem.ptr), (prod_k, d_q_mem.ptr + 32 * cells)]

    def inner():
        return (timed(lambda: sum_ops.prove(d_sign_ops, d_q_ops, seed))[0], timed(lambda: sum_mem.prove(d_sign_mem, d_q_mem, seed))[0],
                timed(lambda: look.prove(d_f, d_t, d["m"], seed))[0])

    def today():
        for p, ptr in halves:
            p.prove(ptr, seed)
        look.prove(d_f, d_t, d["m"], seed)

    # the yardsticks: tuple_leaf_kernel at w = 4 and the fractional sum's trees, on 2^n rows
    tuple_ms, d_leaf, d_tree = C.c_float(), ctx.alloc_fe(rows), [ctx.alloc_fe(2 * rows), ctx.alloc_fe(2 * rows)]
    four = (C.c_void_p * 4)(d["a"].ptr, d["wv"].ptr, d["rv"].ptr, d["rt"].ptr)
    g, b = np.ascontiguousarray(claims.gamma), np.ascontiguousarray(claims.beta)
    cols = mc.columns(d)
    leaf2 = (C.c_float * 2)()
    t = {key: [] for key in ("pkm_prove", "inner_sum", "pkf_prove_ops", "pkf_prove_mem", "pkf_lookup_prove", "today", "pkm_trace", "tuple_leaf_w4_ms", "tree_n1_ms",
                             "ops_leaf_ms", "cells_leaf_ms")}
    profs = []
    for rep in range(reps + 1):
        ms_trace, _ = timed(trace)
        prof = profile(prover)
        ms_prove, (proof, _) = timed(lambda: prover.prove(d, bind))
        prof.update({key: v for key, v in profile(prover).items() if key.startswith(("leaf", "side"))})
        ms_inner = inner()
        ms_today, _ = timed(today)
        assert probes.pk_probe_tuple_leaves(ctx.handle, n, 4, 1, four, g.ctypes.data, b.ctypes.data, d_leaf.ptr, 0, C.byref(tuple_ms)) == 0
        ms_tree, _ = timed(lambda: fs.tree(ctx, n + 1, d_sign_ops, d_q_ops, d_tree[0], d_tree[1]))
        assert probes.pk_probe_mem_leaves(ctx.handle, n, k, C.addressof(cols), g.ctypes.data, b.ctypes.data, d_q_ops.ptr, d_q_mem.ptr, d_f.ptr, 0, leaf2) == 0
        if rep == 0:  # warm-up, and the proof is a proof
            assert mc.verify(stmt, proof, bind)[0].accepted
            continue
        for key, v in (("pkm_prove", ms_prove), ("inner_sum", sum(ms_inner)), ("pkf_prove_ops", ms_inner[0]), ("pkf_prove_mem", ms_inner[1]), ("pkf_lookup_prove", ms_inner[2]),
                       ("today", ms_today), ("pkm_trace", ms_trace), ("tuple_leaf_w4_ms", tuple_ms.value), ("tree_n1_ms", ms_tree), ("ops_leaf_ms", leaf2[0]),
                       ("cells_leaf_ms", leaf2[1])):
            t[key].append(v)
        profs.append(prof)
    ms = {key: spread(v) for key, v in t.items()}
    split = {key: spread([p[key] for p in profs]) for key in profs[0]}
    bytes_moved = {"key": rows * (4 + 32 + 8) + cells * 96, "resolve": rows * (8 + 32 + 32 + 32 + 4) + cells * 64, "ops_leaf": rows * 32 * 7, "cells_leaf": cells * 32 * 5,
                   "tuple_leaf_w4": rows * 32 * 5, "tree_n1": rows * 32 * 2 * 4}

    def tbps(what, ms_value):
        return bytes_moved[what] / (ms_value * 1e-3) / 1e12 if ms_value else None

    row = {"n": n, "k": k, "proof_bytes": prover.proof_bytes, "ms": ms, "split": split, "bytes": bytes_moved,
           "TB_per_s": {"resolve": tbps("resolve", split["resolve_ms"]["median"]), "key": tbps("key", split["key_ms"]["median"]),
                        "ops_leaf": tbps("ops_leaf", ms["ops_leaf_ms"]["median"]), "cells_leaf": tbps("cells_leaf", ms["cells_leaf_ms"]["median"]),
                        "tuple_leaf_w4": tbps("tuple_leaf_w4", ms["tuple_leaf_w4_ms"]["median"]), "tree_n1_host_clock": tbps("tree_n1", ms["tree_n1_ms"]["median"])},
           "pkm_minus_inner_ms": ms["pkm_prove"]["median"] - ms["inner_sum"]["median"],
           "overhead_share_of_proof": (ms["pkm_prove"]["median"] - ms["inner_sum"]["median"]) / ms["pkm_prove"]["median"],
           "leaf_share_of_proof": split["leaf_ms"]["median"] / ms["pkm_prove"]["median"],
           "pkm_over_today": ms["pkm_prove"]["median"] / ms["today"]["median"], "separated_from_today": separated(ms["pkm_prove"], ms["today"]),
           "separated_from_inner": separated(ms["pkm_prove"], ms["inner_sum"])}
    print(json.dumps(row), flush=True)
    for p in (prover, sum_ops, sum_mem, look, prod_n, prod_k):
        p.close()
    for buf in list(d.values()) + [d_addr, d_q_ops, d_q_mem, d_f, d_sign_ops, d_sign_mem, d_t, d_leaf] + d_tree:
        buf.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16:12,20:16,24:20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in pair.split(":")) for pair in args.sizes.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/memcheck_bench.py", "reps": args.reps, "count_lds_max_n": probes.pk_probe_mem_count_lds_max_n(),
              "leaf_rows_per_lane": probes.pk_probe_mem_leaf_items(),
              "clocks": "ms: host clock around blocking calls, except *_leaf_ms and tuple_leaf_w4_ms (device events); split: key/sort/resolve/count/leaf_ms device "
                        "events, side_*_ms host clock", "sizes": []}
    for n, k in sizes:
        result["sizes"].append(run(ctx, n, k, args.reps))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
