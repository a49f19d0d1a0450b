#!/usr/bin/env python3
"""What a sparse-matrix evaluation proof costs on one device (libprovekit_spark.so), per (n, s, t), in runs that alternate between the
ways compared on the same tables.  Medians with the spread (min .. max) of `--reps` runs after one warm-up; the warm-up's proof is
verified.

  (a) pkx_begin + pkx_prove against the sum of the three inner calls timed by themselves in the same run -- pks_prove over
      (val, e_row, e_col), pkt_prove (n, s, w = 2) and pkt_prove (n, t, w = 2) on the very tables pkx_prove reads: the difference is
      what the two eq tables, the gather, the staging and the outer transcript cost; `separated` says whether the spreads overlap;
  (b) the gather pass by itself (device events): the TB/s of its own bytes, 8 of indices + 64 gathered + 64 stored an entry; for scale
      pkt_multiplicities (w = 2) on the same rows in the same run, whose count kernel gathers 64 bytes a row from a table of 2^s rows
      (host clock around the blocking call, 4 + 64 + 64 bytes a row);
  (c) the verifier's side, host wall time: pkx_verify + pkx_check_claims.  What it replaces -- pkv_verify's host evaluation of the
      matrices over an R1CS of the same number of non-zeros -- is not timed by this tool and is marked UNMEASURED, as is the cost of
      verifying the four openings;
  (d) pkx_matrix under full skew (every entry in column 0 and row 0) against random indices.

usage: python tools/spark_bench.py [--sizes 16:14:14,20:18:18,24:21:21] [--reps 5] [--out profiles/r33_spark_bench.json]"""
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
from provekit_amd import prodcheck as pc, spark as sp, tuplelookup as tl  # noqa: E402
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
    matrix_ms, gather_ms, eq_ms, side_ms = (C.c_double * 2)(), C.c_double(), C.c_double(), (C.c_double * 3)()
    assert probes.pk_probe_spark_profile(prover.handle, matrix_ms, C.byref(gather_ms), C.byref(eq_ms), side_ms) == 0
    return {"count_ms": matrix_ms[0], "columns_ms": matrix_ms[1], "gather_ms": gather_ms.value, "eq_ms": eq_ms.value, "side_val_ms": side_ms[0],
            "side_row_ms": side_ms[1], "side_col_ms": side_ms[2]}


def small(ctx, values):
    """a device column of small integers as Montgomery elements"""
    limbs = np.zeros((len(values), 4), dtype=np.uint64)
    limbs[:, 0] = values
    buf = ctx.upload(limbs)
    assert product.pk_fe_to_mont(ctx.handle, buf.ptr, buf.ptr, len(values)) == 0
    return buf


def run(ctx, n, s, t, reps):
    entries = 1 << n
    rng = np.random.default_rng(n)
    idx = {"random": (rng.integers(0, 1 << s, size=entries, dtype=np.uint32), rng.integers(0, 1 << t, size=entries, dtype=np.uint32)),
           "skew": (np.zeros(entries, dtype=np.uint32), np.zeros(entries, dtype=np.uint32))}
    d_idx = {kind: (ctx.upload(r), ctx.upload(c)) for kind, (r, c) in idx.items()}
    d = {"val": ctx.upload(random_field(entries, 1).reshape(-1, 4))}
    for name in ("row", "col", "e_row", "e_col"):
        d[name] = ctx.alloc_fe(entries)
    d["m_row"], d["m_col"] = ctx.alloc_fe(1 << s), ctx.alloc_fe(1 << t)
    stmt = sp.Statement(n, s, t, 2)
    prover = sp.Prover(ctx, stmt)
    bind, rx, ry = random_field(2, 3).reshape(-1, 4), random_field(s, 4).reshape(-1, 4), random_field(t, 5).reshape(-1, 4)
    d_row_idx, d_col_idx = d_idx["random"]

    def matrix(kind):
        prover.matrix(d_idx[kind][0], d_idx[kind][1], d["row"], d["col"], d["m_row"], d["m_col"])

    def begin():
        prover.begin(d_row_idx, d_col_idx, rx, ry, d["e_row"], d["e_col"])

    # the inner statements' own provers on the tables pkx_prove reads: the lookups' tables are built here once
    d_eq = [ctx.alloc_fe(1 << s), ctx.alloc_fe(1 << t)]
    assert product.pk_eq_table(ctx.handle, np.ascontiguousarray(rx).ctypes.data, s, d_eq[0].ptr) == 0
    assert product.pk_eq_table(ctx.handle, np.ascontiguousarray(ry).ctypes.data, t, d_eq[1].ptr) == 0
    d_iota = small(ctx, np.arange(1 << max(s, t), dtype=np.uint64))
    seed = random_field(1, 6).reshape(-1, 4)
    val = pc.Prover(ctx, pc.Statement(n, 3, [(1, 0b111)], False, 1))
    look = [tl.Prover(ctx, tl.Statement(n, s, 2, 1, 1)), tl.Prover(ctx, tl.Statement(n, t, 2, 1, 1))]
    d_m_scratch = ctx.alloc_fe(1 << s)
    d_bad = ctx.alloc(64)

    def inner():
        return (timed(lambda: val.prove([d["val"], d["e_row"], d["e_col"]], None, seed))[0],
                timed(lambda: look[0].prove([[d["row"], d["e_row"]]], [d_iota, d_eq[0]], d["m_row"], seed))[0],
                timed(lambda: look[1].prove([[d["col"], d["e_col"]]], [d_iota, d_eq[1]], d["m_col"], seed))[0])

    keys = ("pkx_begin", "pkx_prove", "begin_plus_prove", "inner_sum", "pks_prove_val", "pkt_prove_row", "pkt_prove_col", "pkx_matrix_random", "pkx_matrix_skew",
            "gather_ms", "pkt_multiplicities_w2", "pkx_verify", "pkx_check_claims")
    ms_of = {key: [] for key in keys}
    profs = []
    gather_ms = C.c_float()
    for rep in range(reps + 1):
        ms_skew, _ = timed(lambda: matrix("skew"))
        prof_skew = profile(prover)
        ms_random, _ = timed(lambda: matrix("random"))  # last: the columns the proof reads are the random matrix's
        prof = profile(prover)
        ms_begin, _ = timed(begin)
        ms_prove, (proof, value, claims) = timed(lambda: prover.prove(d, rx, ry, bind))
        prof.update({key: v for key, v in profile(prover).items() if key.startswith(("gather", "eq", "side"))})
        prof.update(count_skew_ms=prof_skew["count_ms"], columns_skew_ms=prof_skew["columns_ms"])
        ms_inner = inner()
        assert probes.pk_probe_spark_gather(ctx.handle, n, s, t, d_row_idx.ptr, d_col_idx.ptr, d_eq[0].ptr, d_eq[1].ptr, d["e_row"].ptr, d["e_col"].ptr, d_bad.ptr, 0,
                                            C.byref(gather_ms)) == 0
        ms_mult, _ = timed(lambda: look[0].multiplicities([[d["row"], d["e_row"]]], [d_iota, d_eq[0]], [d_row_idx], d_m_scratch))
        ms_verify, (res, _, _, seen) = timed(lambda: sp.verify(stmt, proof, rx, ry, bind, expected_value=value))
        assert res.accepted, res
        zero = np.zeros((3, 4), dtype=np.uint64)
        ms_claims, _ = timed(lambda: sp.check_claims(stmt, seen, zero, zero[:2], zero[0], zero[:2], zero[0]))
        if rep == 0:  # warm-up
            continue
        for key, v in (("pkx_begin", ms_begin), ("pkx_prove", ms_prove), ("begin_plus_prove", ms_begin + ms_prove), ("inner_sum", sum(ms_inner)),
                       ("pks_prove_val", ms_inner[0]), ("pkt_prove_row", ms_inner[1]), ("pkt_prove_col", ms_inner[2]), ("pkx_matrix_random", ms_random),
                       ("pkx_matrix_skew", ms_skew), ("gather_ms", gather_ms.value), ("pkt_multiplicities_w2", ms_mult), ("pkx_verify", ms_verify),
                       ("pkx_check_claims", ms_claims)):
            ms_of[key].append(v)
        profs.append(prof)
    ms = {key: spread(v) for key, v in ms_of.items()}
    split = {key: spread([p[key] for p in profs]) for key in profs[0]}
    bytes_moved = {"gather": entries * (8 + 64 + 64), "pkt_multiplicities_w2": entries * (4 + 64 + 64), "count": entries * 8, "columns": entries * (8 + 64)}

    def tbps(what, ms_value):
        return bytes_moved[what] / (ms_value * 1e-3) / 1e12 if ms_value else None

    row = {"n": n, "s": s, "t": t, "proof_bytes": prover.proof_bytes, "ms": ms, "split": split, "bytes": bytes_moved,
           "TB_per_s": {"gather": tbps("gather", ms["gather_ms"]["median"]), "pkt_multiplicities_w2_host_clock": tbps("pkt_multiplicities_w2", ms["pkt_multiplicities_w2"]["median"]),
                        "count_random": tbps("count", split["count_ms"]["median"]), "count_skew": tbps("count", split["count_skew_ms"]["median"]),
                        "columns": tbps("columns", split["columns_ms"]["median"])},
           "begin_plus_prove_minus_inner_ms": ms["begin_plus_prove"]["median"] - ms["inner_sum"]["median"],
           "begin_plus_prove_over_inner": ms["begin_plus_prove"]["median"] / ms["inner_sum"]["median"],
           "separated_from_inner": separated(ms["begin_plus_prove"], ms["inner_sum"]),
           "matrix_skew_over_random": ms["pkx_matrix_skew"]["median"] / ms["pkx_matrix_random"]["median"],
           "matrix_skew_separated": separated(ms["pkx_matrix_skew"], ms["pkx_matrix_random"]),
           "verifier_host_ms": ms["pkx_verify"]["median"] + ms["pkx_check_claims"]["median"], "host_matrix_evaluation_ms": "UNMEASURED", "opening_ms": "UNMEASURED"}
    print(json.dumps(row), flush=True)
    for p in [prover, val] + look:
        p.close()
    for buf in list(d.values()) + [b for pair in d_idx.values() for b in pair] + d_eq + [d_iota, d_m_scratch, d_bad]:
        buf.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16:14:14,20:18:18,24:21:21")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in triple.split(":")) for triple in args.sizes.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/spark_bench.py", "reps": args.reps, "count_lds_max": sp.count_lds_max(), "gather_entries_per_lane": probes.pk_probe_spark_gather_items(),
              "clocks": "ms: host clock around blocking calls, except gather_ms (device events); split: count/columns/gather_ms device events, eq_ms and side_*_ms "
                        "host clock", "sizes": []}
    for n, s, t in sizes:
        result["sizes"].append(run(ctx, n, s, t, args.reps))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
