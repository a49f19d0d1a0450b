#!/usr/bin/env python3
"""What a bitwise operation by digit lookups costs on one device (libprovekit_bitwise.so), per (n, d, L) and input kind ("random" words
below 2^(L d); "small" words below 2^d: every high digit row is row 0), in runs that alternate between the ways compared on the same
columns.  Medians with the spread (min .. max) of `--reps` runs after one warm-up; the warm-up's proof is verified.  The operation is
XOR; the three operations differ in one integer instruction of the pass.

  (a) the fused pass, pkb_decompose, by itself (device events through tools/probes: TB/s of its own bytes, 64 read + 32 (3 L + 1)
      written per entry) against what the libraries below offer for the same job: the host split of three columns into digits (numpy),
      the upload of the digit columns and the index lists, and pkt_multiplicities at w = 3 with the index lists given -- whole, and its
      device part alone (the blocking call, host clock).  `separated` says whether the spreads overlap, else it is a tie;
  (b) pkb_prove against pkt_prove on the same columns and table (host clock around the blocking calls);
  (c) pkb_verify + pkb_check_claims, host wall time, and the proof bytes;
  (d) small words against random words in the fused pass: what the per-group wavefront aggregation buys under device-memory atomics
      (d above the LDS bound) -- the high digit rows of small words all fall in bin 0.

usage: python tools/bitwise_bench.py [--sizes 20:8:4,24:8:4,24:6:4] [--reps 5] [--out profiles/r39_bitwise_bench.json]"""
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
from provekit_amd import bitwise as bw, tuplelookup as tl  # noqa: E402
from provekit_amd._lib import lib as product  # noqa: E402
from provekit_amd.field import random_field  # noqa: E402
from tools.pk_probes import lib as probes  # noqa: E402

OP = bw.XOR


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def separated(a, b):
    return a["max"] < b["min"] or b["max"] < a["min"]


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def canonical(values):
    limbs = np.zeros((len(values), 4), dtype=np.uint64)
    limbs[:, 0] = values
    return limbs


def to_device(ctx, values):
    """a device column of integers below 2^64 as Montgomery elements"""
    buf = ctx.upload(canonical(values))
    assert product.pk_fe_to_mont(ctx.handle, buf.ptr, buf.ptr, len(values)) == 0
    return buf


def run(ctx, n, d, L, kind, reps):
    entries, rows = 1 << n, 1 << (2 * d)
    rng = np.random.default_rng(n + d + L)
    top = d if kind == "small" else d * L
    a = rng.integers(0, 1 << top, size=entries, dtype=np.uint64)
    b = rng.integers(0, 1 << top, size=entries, dtype=np.uint64)
    stmt = bw.Statement(n, OP, d, L, 2)
    prover = bw.Prover(ctx, stmt)
    pl = prover.plan
    d_a, d_b, d_c = to_device(ctx, a), to_device(ctx, b), ctx.alloc_fe(entries)
    d_digits = [ctx.alloc_fe(entries) for _ in range(3 * L)]
    d_m, d_m_other = ctx.alloc_fe(rows), ctx.alloc_fe(rows)
    d_counts, d_bad = ctx.alloc(4 * rows), ctx.alloc(64)
    digit_ptrs = (C.c_void_p * (3 * L))(*[buf.ptr for buf in d_digits])
    bind, seed = random_field(2, 3).reshape(-1, 4), random_field(1, 6).reshape(-1, 4)
    look = tl.Prover(ctx, tl.Statement(n, 2 * d, 3, pl.c, 1))
    y = np.arange(rows, dtype=np.uint64)
    mask = np.uint64((1 << d) - 1)
    d_table = [to_device(ctx, col) for col in (y >> np.uint64(d), y & mask, (y >> np.uint64(d)) ^ (y & mask))]

    def host_way():
        """what the libraries below offer: form c and split three columns on the host, upload digit columns and index lists, count
        with the index lists given"""
        t0 = time.perf_counter()
        words = (a, b, a ^ b)
        cols = [[(w >> np.uint64(d * i)) & mask for w in words] for i in pl.digit_of]
        idx_host = [((g[0] << np.uint64(d)) | g[1]).astype(np.uint32) for g in cols]
        t1 = time.perf_counter()
        bufs = [[to_device(ctx, col) for col in g] for g in cols]
        idx = [ctx.upload(i) for i in idx_host]
        product.pk_ctx_sync(ctx.handle)
        t2 = time.perf_counter()
        look.multiplicities(bufs, d_table, idx, d_m_other)
        t3 = time.perf_counter()
        for buf in [x for g in bufs for x in g] + idx:
            buf.free()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3

    keys = ("decompose_device", "pkb_decompose", "host_split", "host_upload", "pkt_multiplicities", "host_way_whole", "pkb_prove", "pkt_prove", "pkb_verify", "pkb_check_claims")
    ms_of = {key: [] for key in keys}
    dev_ms = C.c_float()
    for rep in range(reps + 1):
        assert probes.pk_probe_bitwise_decompose(ctx.handle, n, OP, d, L, d_a.ptr, d_b.ptr, d_c.ptr, 0, digit_ptrs, d_counts.ptr, d_bad.ptr, d_m.ptr, 0, C.byref(dev_ms)) == 0
        ms_dec, _ = timed(lambda: prover.decompose(d_a, d_b, d_c, d_digits, d_m))
        split_ms, upload_ms, mult_ms = host_way()
        ms_prove, (proof, claims) = timed(lambda: prover.prove(d_digits, d_m, bind))
        groups = [[d_digits[j * L + i] for j in range(3)] for i in pl.digit_of]
        ms_inner, _ = timed(lambda: look.prove(groups, d_table, d_m, seed))
        ms_verify, (res, _, _, seen) = timed(lambda: bw.verify(stmt, proof, bind))
        assert res.accepted, res
        zero = np.zeros((3 * L, 4), dtype=np.uint64)
        ms_claims, _ = timed(lambda: bw.check_claims(stmt, seen, zero[:3], zero, zero[0]))
        if rep == 0:  # warm-up
            assert np.array_equal(ctx.download_fe(d_m, rows), ctx.download_fe(d_m_other, rows)), "the two ways count the same"
            continue
        for key, v in (("decompose_device", dev_ms.value), ("pkb_decompose", ms_dec), ("host_split", split_ms), ("host_upload", upload_ms), ("pkt_multiplicities", mult_ms),
                       ("host_way_whole", split_ms + upload_ms + mult_ms), ("pkb_prove", ms_prove), ("pkt_prove", ms_inner), ("pkb_verify", ms_verify),
                       ("pkb_check_claims", ms_claims)):
            ms_of[key].append(v)
    ms = {key: spread(v) for key, v in ms_of.items()}
    own_bytes = entries * (64 + 32 * (3 * L + 1))
    verdict = lambda x, y: "SEPARATED" if separated(ms[x], ms[y]) else "TIE"  # noqa: E731
    row = {"n": n, "op": "xor", "d": d, "L": L, "kind": kind, "groups": pl.c, "lds_histogram": d <= bw.count_lds_max_d(), "proof_bytes": prover.proof_bytes, "ms": ms,
           "decompose_bytes": own_bytes, "decompose_TB_per_s": own_bytes / (ms["decompose_device"]["median"] * 1e-3) / 1e12,
           "fused_vs_host_way_whole": verdict("pkb_decompose", "host_way_whole"),
           "pkb_decompose_over_host_way_whole": ms["pkb_decompose"]["median"] / ms["host_way_whole"]["median"],
           "fused_vs_pkt_multiplicities": verdict("pkb_decompose", "pkt_multiplicities"),
           "pkb_decompose_over_pkt_multiplicities": ms["pkb_decompose"]["median"] / ms["pkt_multiplicities"]["median"],
           "pkb_prove_vs_pkt_prove": verdict("pkb_prove", "pkt_prove"), "pkb_prove_over_pkt_prove": ms["pkb_prove"]["median"] / ms["pkt_prove"]["median"],
           "verifier_host_ms": ms["pkb_verify"]["median"] + ms["pkb_check_claims"]["median"]}
    print(json.dumps(row), flush=True)
    for p in (prover, look):
        p.close()
    for buf in [d_a, d_b, d_c, d_m, d_m_other, d_counts, d_bad] + d_table + d_digits:
        buf.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="20:8:4,24:8:4,24:6:4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in triple.split(":")) for triple in args.sizes.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/bitwise_bench.py", "reps": args.reps, "count_lds_max_d": bw.count_lds_max_d(), "decompose_entries_per_lane": probes.pk_probe_bitwise_decompose_items(),
              "clocks": "ms: host clock around blocking calls, except decompose_device (device events)",
              "unmeasured": ["AND and OR (one integer instruction of the pass differs)", "c_given = 1 (a third 32-byte load per entry, one store fewer)",
                             "the table kernel at prover creation", "device counters of the pass (no profiler run)"],
              "rows": []}
    for n, d, L in sizes:
        rows = {kind: run(ctx, n, d, L, kind, args.reps) for kind in ("random", "small")}
        small, rand = rows["small"]["ms"]["decompose_device"], rows["random"]["ms"]["decompose_device"]
        result["rows"] += list(rows.values())
        result.setdefault("small_over_random", []).append({"n": n, "d": d, "L": L, "ratio": small["median"] / rand["median"], "verdict": "SEPARATED" if separated(small, rand) else "TIE"})
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
