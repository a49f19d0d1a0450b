#!/usr/bin/env python3
"""The two kernels of a linear statement against the routes the product's public API offers for the same values:

  sums         pkw_weighted_sums            against  batch * l calls of pk_dot
  combination  linear.hip's combine kernel  against  l calls of pk_fe_axpy   (through tools/probes: it has no C ABI)

and what ships for the weighted sums (a 2 x 2 register tile; 1 x 4 for a single polynomial) against 1 x 4, 2 x 1 and 2 x 2 throughout.  Writes
profiles/r13_whir_pcs_linear.json.

    python tools/whir_pcs_linear_bench.py [--out profiles/r13_whir_pcs_linear.json] [--reps 9] [--sizes 20,22]

A/B on one box in one process: per shape both sides are warmed, then timed ALTERNATING for --reps rounds.  Every figure is host wall
time of the blocking call(s), which is what a caller sees; each side's run-to-run spread is (max - min) / median of its rounds.
"not slower" is judged as: fused median <= public median * (1 + the larger of the two spreads).  Achieved bandwidth counts the bytes
the shipped tile T_b x T_w must read, 32 * 2^n * (batch * ceil(l / T_w) + l * ceil(batch / T_b)); the bound is the larger of those bytes over the
achievable HBM bandwidth and 81 * 2^n * batch * l multiply-adds over the measured v_mad_u64_u32 rate
(profiles/r03_ubench_valu_rates.txt).  Without a GPU the result's shape is printed with null figures and no file is written."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
ACHIEVABLE_GBPS = 6300.0  # what the project takes as achievable HBM bandwidth on MI355X
MAD_PER_S = 27.9e12       # v_mad_u64_u32 lane-operations per second, 4 waves per SIMD (profiles/r03_ubench_valu_rates.txt)
SHAPES = [(batch, l) for batch in (1, 2) for l in (1, 4, 16)]

from whir_pcs_helpers import ab, ptrs  # noqa: E402


def not_slower(fused, public):
    return fused["median_ms"] <= public["median_ms"] * (1 + max(fused["spread"], public["spread"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_whir_pcs_linear.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="20,22")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    result = {"tool": "tools/whir_pcs_linear_bench.py", "achievable_gbps": ACHIEVABLE_GBPS, "mad_per_s": MAD_PER_S, "reps": args.reps, "sums": [],
              "combination": []}
    try:
        import torch

        torch.cuda.is_available()
        import pk_probes
        import provekit_amd
        from provekit_amd import whir_pcs
        from provekit_amd._lib import lib
        from provekit_amd.field import random_field

        ctx = provekit_amd.Context(0)
    except Exception as e:  # no device: the shape of the file without figures
        result["measured_on_mi355x"] = False
        result["note"] = f"not run on a GPU ({type(e).__name__}: {e}); every figure is null"
        for n in sizes:
            for batch, l in SHAPES:
                result["sums"].append({"n_vars": n, "batch": batch, "l": l, "fused": None, "public": None, "not_slower": None})
            for l in (1, 4, 16):
                result["combination"].append({"n_vars": n, "l": l, "fused": None, "public": None, "not_slower": None})
        print(json.dumps(result))  # no file: profiles/ holds measurements only
        return
    result["measured_on_mi355x"] = True
    probes = pk_probes.lib
    for n in sizes:
        N = 1 << n
        polys = [ctx.upload(random_field(N, 10 + b)) for b in range(2)]
        weights = [ctx.upload(random_field(N, 30 + i)) for i in range(16)]
        scales = random_field(16, 5)
        table = ctx.alloc_fe(N)
        out4 = np.zeros(4, dtype=np.uint64)
        for batch, l in SHAPES:
            f, w = polys[:batch], weights[:l]

            def fused():
                return whir_pcs.weighted_sums(ctx, f, n, w)

            def public():
                vals = np.zeros((batch, l, 4), dtype=np.uint64)
                for b in range(batch):
                    for i in range(l):
                        ctx._check(lib.pk_dot(ctx.handle, w[i].ptr, f[b].ptr, N, out4.ctypes.data))
                        vals[b, i] = out4
                return vals

            def tiled(tile):
                def run():
                    out = np.zeros((batch, l, 4), dtype=np.uint64)
                    ctx._check(probes.pk_probe_whir_weighted_sums(ctx.handle, ptrs(f), batch, n, ptrs(w), l, 0, tile, out.ctypes.data))
                    return out

                return run

            ref = public()
            assert np.array_equal(fused(), ref) and all(np.array_equal(tiled(t)(), ref) for t in (1, 2, 3)), "the routes disagree"
            t = ab({"fused": fused, "public": public, "tile_1x4": tiled(1), "tile_2x1": tiled(2), "tile_2x2": tiled(3)}, args.reps)
            tb, tw = (1, 4) if batch == 1 else (2, 2)  # the tile that ships for this batch
            nbytes = 32 * N * (batch * ((l + tw - 1) // tw) + l * ((batch + tb - 1) // tb))
            t_mem, t_alu = nbytes / (ACHIEVABLE_GBPS * 1e9), 81 * N * batch * l / MAD_PER_S
            row = {"n_vars": n, "batch": batch, "l": l, **t, "ratio": round(t["fused"]["median_ms"] / t["public"]["median_ms"], 4),
                   "not_slower": not_slower(t["fused"], t["public"]), "algorithmic_bytes": nbytes,
                   "gbps": round(nbytes / (t["fused"]["median_ms"] * 1e-3) / 1e9, 1), "bound": "memory" if t_mem >= t_alu else "multiply-add issue",
                   "fraction_of_bound": round(max(t_mem, t_alu) / (t["fused"]["median_ms"] * 1e-3), 3)}
            result["sums"].append(row)
            print(json.dumps(row), flush=True)
        for l in (1, 4, 16):
            w = weights[:l]

            def fused_c():
                ctx._check(probes.pk_probe_whir_combine(ctx.handle, table.ptr, N, ptrs(w), scales.ctypes.data, l, 1))

            def public_c():
                for i in range(l):
                    ctx._check(lib.pk_fe_axpy(ctx.handle, table.ptr, scales[i].ctypes.data, w[i].ptr, N))
                ctx.sync()

            ctx.zero(table.ptr, 32 * N)
            fused_c()
            a = ctx.download_fe(table.ptr, N)
            ctx.zero(table.ptr, 32 * N)
            public_c()
            assert np.array_equal(a, ctx.download_fe(table.ptr, N)), "the two combinations disagree"
            t = ab({"fused": fused_c, "public": public_c}, args.reps)
            nbytes = 32 * N * (l + 2)
            row = {"n_vars": n, "l": l, **t, "ratio": round(t["fused"]["median_ms"] / t["public"]["median_ms"], 4),
                   "not_slower": not_slower(t["fused"], t["public"]), "algorithmic_bytes": nbytes, "public_bytes": 96 * N * l,
                   "gbps": round(nbytes / (t["fused"]["median_ms"] * 1e-3) / 1e9, 1)}
            result["combination"].append(row)
            print(json.dumps(row), flush=True)
        for x in polys + weights + [table]:
            x.free()
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
