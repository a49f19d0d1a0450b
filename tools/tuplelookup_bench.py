#!/usr/bin/env python3
"""What a tuple lookup costs on one device (libprovekit_tuplelookup.so against libprovekit_fracsum.so's single-column lookup), per
(n, k), in runs that alternate between the ways compared on the same tables.  Medians with the spread (min .. max) of `--reps` runs
after one warm-up; every proof of the warm-up is verified.

  (a) pkt_prove at w = 1, c = 1 against pkf_lookup_prove on the same column: the difference is the separate leaf pass (pkf's lookup
      forms its leaves inside the first tree launch) and the proof staged on the host; `separated` says whether the two spreads overlap;
  (b) w = 2, 3, 4 at c = 1: pkt_prove, and the leaf and count kernels' device time (events), their share of a proof and the GB/s of
      the bytes they move, next to tree_kernel's 4.4 TB/s for scale;
  (c) c = 4, w = 1 against four pkf_lookup_prove calls on the four columns: the batching gain.

usage: python tools/tuplelookup_bench.py [--sizes 16:8,20:16,24:20] [--reps 5] [--out profiles/r30_tuplelookup_bench.json]"""
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
from provekit_amd import fracsum as fs, tuplelookup as tl  # noqa: E402
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
    leaf_ms, count_ms, side_ms = C.c_double(), C.c_double(), (C.c_double * 2)()
    assert probes.pk_probe_tuple_profile(prover.handle, C.byref(leaf_ms), C.byref(count_ms), side_ms) == 0
    return {"leaf_ms": leaf_ms.value, "count_ms": count_ms.value, "side_f_ms": side_ms[0], "side_t_ms": side_ms[1]}


class Case:
    """a table of w random columns (rows distinct with overwhelming probability) and c groups of rows drawn from it, with their
    multiplicities from pkt_multiplicities"""

    def __init__(self, ctx, n, k, w, c):
        self.ctx, self.n, self.k, self.w, self.c = ctx, n, k, w, c
        t = [random_field(1 << k, 1 + j).reshape(-1, 4) for j in range(w)]
        rng = np.random.default_rng(2)
        self.idx = [rng.integers(0, 1 << k, size=1 << n, dtype=np.uint32) for _ in range(c)]
        self.d_t = [ctx.upload(col) for col in t]
        self.d_f = [[ctx.upload(col[i]) for col in t] for i in self.idx]
        self.d_idx = [ctx.upload(i) for i in self.idx]
        self.d_m = ctx.alloc_fe(1 << k)
        self.stmt = tl.Statement(n, k, w, c, 2)
        self.prover = tl.Prover(ctx, self.stmt)
        self.prover.multiplicities(self.d_f, self.d_t, self.d_idx, self.d_m)
        self.bind = random_field(2, 3).reshape(-1, 4)

    def prove(self):
        return self.prover.prove(self.d_f, self.d_t, self.d_m, self.bind)

    def close(self):
        self.prover.close()
        for b in self.d_t + [b for cols in self.d_f for b in cols] + self.d_idx + [self.d_m]:
            b.free()


def single_column(ctx, case, reps, measure):
    """(a) and (c): one pkt_prove of all c groups against c pkf_lookup_prove calls, one per group's column (w = 1)"""
    n, k, c = case.n, case.k, case.c
    gkr = fs.LookupProver(ctx, fs.LookupStatement(n, k, 2))
    d_ms = []
    for g in range(c):  # each single-column lookup needs its own column's multiplicities
        counts = np.bincount(case.idx[g], minlength=1 << k).astype(np.uint64)
        limbs = np.zeros((1 << k, 4), dtype=np.uint64)
        limbs[:, 0] = counts
        d = ctx.upload(limbs)
        from provekit_amd._lib import lib as product

        assert product.pk_fe_to_mont(ctx.handle, d.ptr, d.ptr, 1 << k) == 0
        d_ms.append(d)

    def separate():
        return [gkr.prove(case.d_f[g][0], case.d_t[0], d_ms[g], case.bind) for g in range(c)]

    times = {"pkt_prove": [], "pkf_lookup_prove x %d" % c: []}
    names = list(times)
    profs = []
    for rep in range(reps + 1):
        ms_t, (proof, _) = timed(case.prove)
        prof = profile(case.prover)
        ms_f, proofs = timed(separate)
        if rep == 0:  # warm-up, and the proofs are proofs
            assert tl.verify(case.stmt, proof, case.bind)[0].accepted
            assert all(fs.lookup_verify(gkr.stmt, p, case.bind)[0].accepted for p, _ in proofs)
            continue
        times[names[0]].append(ms_t), times[names[1]].append(ms_f), profs.append(prof)
    row = {"measure": measure, "n": n, "k": k, "w": 1, "c": c, "ms": {name: spread(v) for name, v in times.items()},
           "proof_bytes": {"pkt": case.prover.proof_bytes, "pkf": c * gkr.proof_bytes},
           "pkt_split": {key: spread([p[key] for p in profs]) for key in ("leaf_ms", "side_f_ms", "side_t_ms")}}
    row["pkt_over_pkf"] = row["ms"][names[0]]["median"] / row["ms"][names[1]]["median"]
    row["separated"] = separated(row["ms"][names[0]], row["ms"][names[1]])
    print(json.dumps(row), flush=True)
    gkr.close()
    for d in d_ms:
        d.free()
    return row


def widths(case, reps):
    """(b): pkt_prove and its two kernels at one width"""
    n, k, w = case.n, case.k, case.w
    total, profs = [], []
    for rep in range(reps + 1):
        case.prover.multiplicities(case.d_f, case.d_t, case.d_idx, case.d_m)
        ms, (proof, _) = timed(case.prove)
        if rep == 0:
            assert tl.verify(case.stmt, proof, case.bind)[0].accepted
            continue
        total.append(ms), profs.append(profile(case.prover))
    rows, size = 1 << n, 1 << k
    leaf_bytes = 32 * (w + 1) * (rows + size)                                 # every column read, every leaf written, both sides
    count_bytes = rows * (4 + 64 * w) + 4 * size + size * (4 + 32)            # idx, f's rows and the gathered rows of t; counts zeroed; the mont pass
    row = {"measure": "widths", "n": n, "k": k, "w": w, "c": 1, "ms": {"pkt_prove": spread(total)},
           "kernels": {key: spread([p[key] for p in profs]) for key in ("leaf_ms", "count_ms")}, "bytes": {"leaf": leaf_bytes, "count": count_bytes}}
    row["GB_per_s"] = {"leaf": leaf_bytes / (row["kernels"]["leaf_ms"]["median"] * 1e-3) / 1e9, "count": count_bytes / (row["kernels"]["count_ms"]["median"] * 1e-3) / 1e9}
    row["share_of_proof"] = {"leaf": row["kernels"]["leaf_ms"]["median"] / row["ms"]["pkt_prove"]["median"]}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16:8,20:16,24:20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in pair.split(":")) for pair in args.sizes.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/tuplelookup_bench.py", "reps": args.reps, "count_lds_max_k": tl.count_lds_max_k(), "leaf_rows_per_lane": probes.pk_probe_tuple_leaf_items(),
              "clocks": "ms of calls and side_*_ms: host clock around blocking calls; leaf_ms and count_ms: device events",
              "tree_kernel_TB_per_s_for_scale": 4.4, "single_column": [], "widths": [], "batched": []}
    for n, k in sizes:
        for measure, w, c in (("single_column", 1, 1), ("widths", 2, 1), ("widths", 3, 1), ("widths", 4, 1), ("batched", 1, 4)):
            case = Case(ctx, n, k, w, c)
            result[measure].append(widths(case, args.reps) if measure == "widths" else single_column(ctx, case, args.reps, measure))
            case.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
