#!/usr/bin/env python3
"""Where a grand-product proof's time goes on one device (libprovekit_grandproduct.so, provekit_amd.grandproduct): per n the host time
of pkg_prove, the device time of its tree phase and the host time of every layer's pks_prove (pk_probe_grandproduct_profile: two
clocks), and per (n, w) the host time of pkg_multiset_prove with the same split for the side it proves last.  Medians with the spread
(min .. max) of `--reps` runs after one warm-up; every proof of the warm-up is verified.

One yardstick rides along: the tree kernels by themselves (tools/probes/grandproduct.hip) at 1, 2 and 3 layers per launch, alternating
on the same table, from a plain table and from w columns through the leaf kernel, with the bytes each variant moves and its GB/s.

usage: python tools/grandproduct_bench.py [--sizes 16,20,24] [--widths 1,2] [--reps 5] [--out profiles/r25_grandproduct_bench.json]"""
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
from provekit_amd import grandproduct as gp  # noqa: E402
from provekit_amd.field import random_field  # noqa: E402
from tools.pk_probes import lib as probes  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def tree_bytes(n, s, w=0):
    """what the tree kernels move at s layers per launch: every launch reads the layer it starts from and writes the layers it makes;
    with w > 0 the first launch reads w columns instead and writes the leaves too"""
    t, d, total, first = gp.tail_max_n(), n, 0, True
    while d > 0:
        step = min(s, d - t) if d > t else d  # the tail takes everything that is left
        if first and w:
            step = min(s, d - t) if d > t else 0
            total += 32 * (w + 1) * (1 << d)
        else:
            total += 32 * (1 << d)
        total += 32 * sum(1 << (d - k) for k in range(1, step + 1))
        d -= step
        first = False
    return total


def profile(handle, n):
    tree_ms, layer_ms = C.c_double(), (C.c_double * 28)()
    assert probes.pk_probe_grandproduct_profile(handle, C.byref(tree_ms), layer_ms) == 0
    return tree_ms.value, [layer_ms[d] for d in range(1, n)]


def summarise(n, host, tree, layers):
    layer_medians = [statistics.median(v) for v in layers]
    row = {"host_ms": spread(host), "tree_ms": spread(tree), "layer_ms": {str(d + 1): spread(v) for d, v in enumerate(layers)}}
    total = statistics.median(host)
    row["sumchecks_ms_median_sum"] = sum(layer_medians)
    row["tree_share_of_host"] = statistics.median(tree) / total
    row["sumchecks_share_of_host"] = sum(layer_medians) / total
    small = [v for d, v in enumerate(layer_medians, start=1) if d <= gp.tail_max_n()]
    row["layers_up_to_tail_ms"], row["layers_up_to_tail_share_of_host"] = sum(small), sum(small) / total
    return row


def bench_product(ctx, n, reps):
    d_v = ctx.upload(random_field(1 << n, 1).reshape(-1, 4))
    prover = gp.GrandProductProver(ctx, gp.Statement(n))
    host, tree, layers = [], [], [[] for _ in range(n - 1)]
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        proof, product, _, _ = prover.prove(d_v)  # blocking: ends in a device-to-host copy of the last layer's tables
        ms = (time.perf_counter() - t0) * 1e3
        if rep == 0:  # warm-up, and the proof is a proof
            assert gp.verify(prover.stmt, proof, expected_product=product)[0].accepted
            continue
        t, per_layer = profile(prover.handle, n)
        host.append(ms), tree.append(t)
        for acc, v in zip(layers, per_layer):
            acc.append(v)
    row = {"call": "pkg_prove", "n": n, "arena_bytes": gp.arena_bytes(prover.stmt), "proof_bytes": prover.proof_bytes, **summarise(n, host, tree, layers)}
    print(json.dumps(row), flush=True)
    prover.close()
    d_v.free()
    return row


def bench_multiset(ctx, n, w, reps):
    cols = [random_field(1 << n, 10 + j).reshape(-1, 4) for j in range(w)]
    perm = np.random.default_rng(5).permutation(1 << n)
    d_a, d_b = [ctx.upload(c) for c in cols], [ctx.upload(c[perm]) for c in cols]
    prover = gp.MultisetProver(ctx, gp.MultisetStatement(n, w))
    inner = probes.pk_probe_multiset_inner(prover.handle)
    host, tree, layers = [], [], [[] for _ in range(n - 1)]
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        proof, _ = prover.prove(d_a, d_b)
        ms = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            assert gp.multiset_verify(prover.stmt, proof)[0].accepted
            continue
        t, per_layer = profile(inner, n)
        host.append(ms), tree.append(t)
        for acc, v in zip(layers, per_layer):
            acc.append(v)
    # the profile is of the side proved last: one of three leaf-and-tree passes and one of two chains
    row = {"call": "pkg_multiset_prove", "n": n, "w": w, "proof_bytes": prover.proof_bytes, "profile_of": "side B: one leaf-and-tree pass of three, one chain of two"}
    s = summarise(n, host, tree, layers)
    for key in ("tree_share_of_host", "sumchecks_share_of_host", "layers_up_to_tail_share_of_host"):
        del s[key]
    total = statistics.median(host)
    s["tree_share_of_host_all_three_passes"] = 3 * statistics.median(tree) / total
    s["sumchecks_share_of_host_both_chains"] = 2 * s["sumchecks_ms_median_sum"] / total
    row.update(s)
    print(json.dumps(row), flush=True)
    prover.close()
    for b in d_a + d_b:
        b.free()
    return row


def tree_ab(ctx, n, widths, reps):
    """1, 2 and 3 layers per launch, alternating, from a table and through the leaf kernel"""
    rows = []
    d_tree, d_leaf = ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n)
    d_cols = [ctx.upload(random_field(1 << n, 20 + j).reshape(-1, 4)) for j in range(max(widths))]
    ptrs = (C.c_void_p * len(d_cols))(*(b.ptr for b in d_cols))
    gamma, beta = random_field(1, 30).reshape(-1, 4), random_field(1, 31).reshape(-1, 4)
    ms = C.c_float()
    for w in [0] + list(widths):
        ts = {s: [] for s in (1, 2, 3)}
        for rep in range(reps + 1):
            for s in ts:  # alternating
                if w:
                    rc = probes.pk_probe_grandproduct_leaf_tree(ctx.handle, n, w, ptrs, gamma.ctypes.data, beta.ctypes.data, d_leaf.ptr, d_tree.ptr, s, 0, C.byref(ms))
                else:
                    rc = probes.pk_probe_grandproduct_tree(ctx.handle, n, d_cols[0].ptr, d_tree.ptr, s, 0, C.byref(ms))
                ctx._check(rc)
                if rep:
                    ts[s].append(ms.value)
        row = {"tree_ab": True, "n": n, "from": f"{w} columns through leaf_kernel" if w else "a table", "layers_per_launch": {}}
        for s, v in ts.items():
            nbytes = tree_bytes(n, s, w)
            row["layers_per_launch"][str(s)] = {"ms": spread(v), "bytes": nbytes, "GB_per_s": nbytes / (statistics.median(v) * 1e-3) / 1e9}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for b in d_cols + [d_tree, d_leaf]:
        b.free()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--widths", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes, widths = [int(v) for v in args.sizes.split(",")], [int(v) for v in args.widths.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/grandproduct_bench.py", "reps": args.reps, "tail_max_n": gp.tail_max_n(), "default_layers_per_launch": probes.pk_probe_grandproduct_default_layers(),
              "clocks": "host_ms and layer_ms: host clock around blocking calls; tree_ms and tree_ab: device events", "products": [], "multisets": [], "tree_ab": []}
    for n in sizes:
        result["products"].append(bench_product(ctx, n, args.reps))
        for w in widths:
            result["multisets"].append(bench_multiset(ctx, n, w, args.reps))
        result["tree_ab"] += tree_ab(ctx, n, widths, args.reps)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
