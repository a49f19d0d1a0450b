#!/usr/bin/env python3
"""Where a lookup proof's time goes on one device (libprovekit_lookup.so, provekit_amd.lookup): per (n, k) and per idx distribution
(uniform, and fully skewed: every lookup one entry) the five phases of the prover's profile (pk_probe_lookup_profile) -- count, table,
gather (device time between events) and the two sumchecks (host time of pks_prove): two clocks -- with each kernel phase's
algorithmic bytes and achieved GB/s.  The two distributions of a size alternate run by run on the same prover; medians with the
spread (min .. max) of `--reps` runs after one warm-up.

Two yardsticks ride along:
  * the inverse: tools/inverse_time.py's per-element figure (pk_probe_arith_device op 23, 2^20 elements) against the table kernel's
    per-element time at the library's lane batch;
  * the gather's LDS-staged kernel against the same pass without staging (the library's kernel for larger tables, through
    tools/probes/lookup.hip), alternating, for every k the staged kernel takes: each at its own grid rule, and the staged one at one and
    two workgroups per CU and at 1024 workgroups.

usage: python tools/lookup_bench.py [--sizes 20:8,20:16,...] [--reps 5] [--out profiles/r24_lookup_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import provekit_amd  # noqa: E402
from provekit_amd import lookup  # noqa: E402
from provekit_amd.field import random_field  # noqa: E402
from tools.pk_probes import lib as probes  # noqa: E402

PHASES = ("count", "table", "gather", "sumcheck_f", "sumcheck_t")


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def phase_bytes(n, k):
    """what each kernel phase must move: count reads idx, f and the gathered t, writes the counts and m; table reads t and the counts,
    writes d_t, g and h_t; gather reads idx and two gathered elements, writes two"""
    N, K = 1 << n, 1 << k
    return {"count": N * (4 + 32 + 32) + K * (4 + 32), "table": K * (32 + 4 + 96), "gather": N * (4 + 64 + 64)}


def bench_size(ctx, n, k, reps):
    t = random_field(1 << k, 1).reshape(-1, 4)
    d_t, d_m = ctx.upload(t), ctx.alloc_fe(1 << k)
    rng = np.random.default_rng(2)
    cols = {}
    for name, idx in (("uniform", rng.integers(0, 1 << k, size=1 << n, dtype=np.uint32)), ("skewed", np.full(1 << n, (1 << k) // 3, dtype=np.uint32))):
        cols[name] = (ctx.upload(t[idx]), ctx.upload(idx))
    prover = lookup.LookupProver(ctx, lookup.Statement(n, k))
    times = {name: {ph: [] for ph in PHASES} for name in cols}
    ms = (C.c_double * len(PHASES))()
    for rep in range(reps + 1):
        for name, (d_f, d_idx) in cols.items():  # alternating
            prover.multiplicities(d_f, d_t, d_idx, d_m)
            prover.begin(d_t, d_idx)
            proof, _ = prover.finish()
            if rep == 0:  # warm-up, and the proof is a proof
                res, _, _ = lookup.verify(prover.stmt, proof)
                assert res.accepted, res
                continue
            ctx._check(probes.pk_probe_lookup_profile(prover.handle, ms))
            for ph, v in zip(PHASES, ms):
                times[name][ph].append(v)
    nbytes = phase_bytes(n, k)
    rows = []
    for name in cols:
        row = {"n": n, "k": k, "idx": name, "arena_bytes": lookup.arena_bytes(prover.stmt), "phases": {}}
        for ph in PHASES:
            entry = {"ms": spread(times[name][ph])}
            if ph in nbytes:
                entry["bytes"] = nbytes[ph]
                entry["GB_per_s"] = nbytes[ph] / (entry["ms"]["median"] * 1e-3) / 1e9
            row["phases"][ph] = entry
        if k >= 16:
            row["table_ns_per_element"] = row["phases"]["table"]["ms"]["median"] * 1e6 / (1 << k)
        rows.append(row)
        print(json.dumps(row), flush=True)
    prover.close()
    for b in [d_t, d_m] + [b for pair in cols.values() for b in pair]:
        b.free()
    return rows


def inverse_yardstick(ctx, reps):
    """tools/inverse_time.py's figure: the variable-time inverse of 2^20 elements, one per lane, ns per element"""
    n = 1 << 20
    a, o = ctx.upload(random_field(n, 1)), ctx.alloc_fe(n)
    for _ in range(2):
        ctx._check(probes.pk_probe_arith_device(ctx.handle, 23, a.ptr, a.ptr, o.ptr, n))
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        ctx._check(probes.pk_probe_arith_device(ctx.handle, 23, a.ptr, a.ptr, o.ptr, n))
        ts.append(ctx.timer_stop())  # milliseconds
    a.free()
    o.free()
    return {"elements": n, "ms": spread(ts), "ns_per_element": statistics.median(ts) * 1e6 / n}


def gather_ab(ctx, n, reps):
    """the LDS-staged gather against the gather through L2, alternating, per k the staged kernel takes"""
    cus = C.c_int()
    ctx._check(probes.pk_probe_num_cus(ctx.handle, C.byref(cus)))
    cus = cus.value
    rows = []
    rng = np.random.default_rng(3)
    d_hf, d_df = ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n)
    for k in range(4, lookup.gather_lds_max_k() + 1):
        d_g, d_dt = ctx.upload(random_field(1 << k, 4)), ctx.upload(random_field(1 << k, 5))
        d_idx = ctx.upload(rng.integers(0, 1 << k, size=1 << n, dtype=np.uint32))
        variants = {"through L2": (0, 0), "staged, own rule": (1, 0), f"staged, {cus} workgroups": (1, cus), f"staged, {2 * cus} workgroups": (1, min(2 * cus, 1024)),
                    "staged, 1024 workgroups": (1, 1024)}
        ts = {name: [] for name in variants}
        ms = C.c_float()
        for rep in range(reps + 1):
            for name, (staged, grid) in variants.items():  # alternating
                ctx._check(probes.pk_probe_lookup_gather(ctx.handle, d_idx.ptr, d_g.ptr, d_dt.ptr, n, k, d_hf.ptr, d_df.ptr, staged, grid, C.byref(ms)))
                if rep:
                    ts[name].append(ms.value)
        row = {"gather_ab": True, "n": n, "k": k, "lds_bytes": 64 << k, "ms": {name: spread(v) for name, v in ts.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for b in (d_g, d_dt, d_idx):
            b.free()
    d_hf.free()
    d_df.free()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="20:8,20:16,20:20,24:8,24:16,24:20", help="n:k pairs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gather-n", default="20,24", help="column sizes of the gather A/B; empty: skip it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/lookup_bench.py", "reps": args.reps, "count_lds_max_k": lookup.count_lds_max_k(), "gather_lds_max_k": lookup.gather_lds_max_k(), "sizes": [], "gather_ab": []}
    result["inverse_yardstick"] = inverse_yardstick(ctx, args.reps)
    print(json.dumps({"inverse_yardstick": result["inverse_yardstick"]}), flush=True)
    for pair in args.sizes.split(","):
        n, k = (int(v) for v in pair.split(":"))
        result["sizes"] += bench_size(ctx, n, k, args.reps)
    for n in [int(v) for v in args.gather_n.split(",") if v]:
        result["gather_ab"] += gather_ab(ctx, n, args.reps)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
