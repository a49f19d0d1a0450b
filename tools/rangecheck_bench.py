#!/usr/bin/env python3
"""What a limb-decomposed range check costs on one device (libprovekit_rangecheck.so), per (n, bits, k) and input kind ("random"
values below 2^bits; "small" values below 2^k: every high limb zero), in runs that alternate between the ways compared on the same
column.  Medians with the spread (min .. max) of `--reps` runs after one warm-up; the warm-up's proof is verified.

  (a) the fused pass, pkr_decompose, by itself (device events through tools/probes: TB/s of its own bytes, 32 read + 32 L written per
      entry) against what the libraries below offer for the same job: the host split of the column into limbs (numpy), the upload of
      the limb columns and the index lists, and pkt_multiplicities with the index lists given -- whole, and its device part alone
      (the blocking call, host clock).  `separated` says whether the spreads overlap, else it is a tie;
  (b) pkr_prove against pkt_prove on the same columns and table: the difference should be the scale pass (device events);
  (c) pkr_verify + pkr_check_claims, host wall time, and the proof bytes;
  (d) small values against random values in the fused pass: what the per-group wavefront aggregation buys under device-memory
      atomics (k above the LDS bound) -- the high limbs of small values all fall in bin 0.

usage: python tools/rangecheck_bench.py [--sizes 20:32:16,24:32:8,24:64:16] [--reps 5] [--out profiles/r38_rangecheck_bench.json]"""
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
from provekit_amd import rangecheck as rc, tuplelookup as tl  # noqa: E402
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


def canonical(values):
    limbs = np.zeros((len(values), 4), dtype=np.uint64)
    limbs[:, 0] = values
    return limbs


def to_device(ctx, values):
    """a device column of integers below 2^64 as Montgomery elements"""
    buf = ctx.upload(canonical(values))
    assert product.pk_fe_to_mont(ctx.handle, buf.ptr, buf.ptr, len(values)) == 0
    return buf


def run(ctx, n, bits, k, kind, reps):
    entries = 1 << n
    rng = np.random.default_rng(n + bits)
    top = min(bits, k) if kind == "small" else bits
    values = rng.integers(0, 1 << top, size=entries, dtype=np.uint64) if top < 64 else rng.integers(0, 2**64, size=entries, dtype=np.uint64)
    stmt = rc.Statement(n, bits, k, 2)
    prover = rc.Prover(ctx, stmt)
    pl = prover.plan
    d_f = to_device(ctx, values)
    d_limbs = [ctx.alloc_fe(entries) for _ in range(pl.limbs)]
    d_m, d_m_other = ctx.alloc_fe(1 << k), ctx.alloc_fe(1 << k)
    d_counts, d_bad = ctx.alloc(4 << k), ctx.alloc(64)
    limb_ptrs = (C.c_void_p * pl.limbs)(*[b.ptr for b in d_limbs])
    bind, seed = random_field(2, 3).reshape(-1, 4), random_field(1, 6).reshape(-1, 4)
    look = tl.Prover(ctx, tl.Statement(n, k, 1, pl.c, 1))
    d_table = to_device(ctx, np.arange(1 << k, dtype=np.uint64))

    def host_way():
        """what the libraries below offer: split on the host, upload limb columns and index lists, count with the index lists given"""
        t0 = time.perf_counter()
        mask = np.uint64((1 << k) - 1)
        cols = [((values >> np.uint64(k * pl.limb_of[g])) & mask) << np.uint64(pl.shift_of[g]) for g in range(pl.c)]
        t1 = time.perf_counter()
        bufs = [to_device(ctx, col) for col in cols]
        idx = [ctx.upload(col.astype(np.uint32)) for col in cols]
        product.pk_ctx_sync(ctx.handle)
        t2 = time.perf_counter()
        look.multiplicities([[b] for b in bufs], [d_table], idx, d_m_other)
        t3 = time.perf_counter()
        for b in bufs + idx:
            b.free()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3

    keys = ("decompose_device", "pkr_decompose", "host_split", "host_upload", "pkt_multiplicities", "host_way_whole", "pkr_prove", "pkt_prove", "scale_device",
            "pkr_verify", "pkr_check_claims")
    ms_of = {key: [] for key in keys}
    dev_ms = C.c_float()
    for rep in range(reps + 1):
        assert probes.pk_probe_range_decompose(ctx.handle, n, bits, k, d_f.ptr, limb_ptrs, d_counts.ptr, d_bad.ptr, d_m.ptr, 0, C.byref(dev_ms)) == 0
        ms_dec, _ = timed(lambda: prover.decompose(d_f, d_limbs, d_m))
        split_ms, upload_ms, mult_ms = host_way()
        ms_prove, (proof, claims) = timed(lambda: prover.prove(d_limbs, d_m, bind))
        scale = (C.c_double(), C.c_double(), C.c_double())
        assert probes.pk_probe_range_profile(prover.handle, *[C.byref(x) for x in scale]) == 0
        # pkt_prove on the same columns: the scaled column is the prover's own, so the top limb stands in for it (same sizes, same table)
        groups = [[d_limbs[pl.limb_of[g]]] for g in range(pl.c)]
        try:
            ms_inner, _ = timed(lambda: look.prove(groups, [d_table], d_m, seed))
        except provekit_amd._lib.ProveKitHipError:  # with a top check m counts the scaled column: the stand-in's fractions differ, after the same work
            ms_inner = None
        ms_verify, (res, _, _, seen) = timed(lambda: rc.verify(stmt, proof, bind))
        assert res.accepted, res
        zero = np.zeros((pl.limbs, 4), dtype=np.uint64)
        ms_claims, _ = timed(lambda: rc.check_claims(stmt, seen, zero[0], zero, zero[0]))
        if rep == 0:  # warm-up
            assert np.array_equal(ctx.download_fe(d_m, 1 << k), ctx.download_fe(d_m_other, 1 << k)), "the two ways count the same"
            continue
        for key, v in (("decompose_device", dev_ms.value), ("pkr_decompose", ms_dec), ("host_split", split_ms), ("host_upload", upload_ms), ("pkt_multiplicities", mult_ms),
                       ("host_way_whole", split_ms + upload_ms + mult_ms), ("pkr_prove", ms_prove), ("scale_device", scale[1].value), ("pkr_verify", ms_verify),
                       ("pkr_check_claims", ms_claims)):
            ms_of[key].append(v)
        if ms_inner is not None:
            ms_of["pkt_prove"].append(ms_inner)
    ms = {key: spread(v) if v else "UNMEASURED" for key, v in ms_of.items()}
    own_bytes = entries * (32 + 32 * pl.limbs)
    row = {"n": n, "bits": bits, "k": k, "kind": kind, "limbs": pl.limbs, "groups": pl.groups, "c": pl.c, "lds_histogram": k <= rc.count_lds_max_k(),
           "proof_bytes": prover.proof_bytes, "ms": ms, "decompose_bytes": own_bytes,
           "decompose_TB_per_s": own_bytes / (ms["decompose_device"]["median"] * 1e-3) / 1e12,
           "fused_vs_pkt_multiplicities": "separated" if separated(ms["pkr_decompose"], ms["pkt_multiplicities"]) else "tie",
           "pkr_decompose_over_pkt_multiplicities": ms["pkr_decompose"]["median"] / ms["pkt_multiplicities"]["median"],
           "pkr_decompose_over_host_way_whole": ms["pkr_decompose"]["median"] / ms["host_way_whole"]["median"],
           "verifier_host_ms": ms["pkr_verify"]["median"] + ms["pkr_check_claims"]["median"]}
    if ms["pkt_prove"] != "UNMEASURED":
        row["pkr_prove_minus_pkt_prove_ms"] = ms["pkr_prove"]["median"] - ms["pkt_prove"]["median"]
    print(json.dumps(row), flush=True)
    for p in (prover, look):
        p.close()
    for buf in [d_f, d_m, d_m_other, d_counts, d_bad, d_table] + d_limbs:
        buf.free()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="20:32:16,24:32:8,24:64:16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in triple.split(":")) for triple in args.sizes.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/rangecheck_bench.py", "reps": args.reps, "count_lds_max_k": rc.count_lds_max_k(), "decompose_entries_per_lane": probes.pk_probe_range_decompose_items(),
              "clocks": "ms: host clock around blocking calls, except decompose_device and scale_device (device events)", "rows": []}
    for n, bits, k in sizes:
        rows = {kind: run(ctx, n, bits, k, kind, args.reps) for kind in ("random", "small")}
        a, b = rows["small"]["ms"]["decompose_device"], rows["random"]["ms"]["decompose_device"]
        result["rows"] += list(rows.values())
        result.setdefault("small_over_random", []).append({"n": n, "bits": bits, "k": k, "ratio": a["median"] / b["median"], "verdict": "separated" if separated(a, b) else "tie"})
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
