#!/usr/bin/env python3
"""What a hiding commitment costs next to a plain one (include/provekit_whir_hiding.h).  At n + 1 = 21 and 23, B = 1 and 3:
the stage kernel alone (the masks and g in one launch, through the probe); pkw_commit_hiding against plain pkw_commit on the same
extended config, in the same process and alternating; pkw_open_hiding against pkw_open on the same extended config.  The expected
shape is commit_hiding = commit + stage (+ the copies of the extended tables).  Writes profiles/r18_whir_pcs_hiding.json.

    python tools/whir_pcs_hiding_bench.py [--out profiles/r18_whir_pcs_hiding.json] [--reps 7] [--sizes 21,23]

Every figure is host wall time of the blocking call (median of --reps after one warm-up).  The configs are pk_whir_config_derive's
with the grinding flattened to 4 bits, so that the proof-of-work search, whose length depends on the transcript, does not decide
the comparison.  A hiding commitment is opened once, so every timed pkw_open_hiding has a fresh commitment made outside the timed
region.  `plain_guard` repeats tools/whir_pcs_bench.py's commit/open row (n_vars = 20, batch 2, q = 8, the derived config as it is)
for comparison with that tool on another commit.  Without a GPU the file is written with null figures and says so."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from whir_pcs_helpers import ab, ptrs, timed  # noqa: E402

KEY = bytes(range(32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_whir_pcs_hiding.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="21,23")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    result = {"tool": "tools/whir_pcs_hiding_bench.py", "reps": args.reps, "rows": [], "plain_guard": None}
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
        result["note"] = f"not run on a GPU ({type(e).__name__}: {e}); figures are null"
        for n1 in sizes:
            for B in (1, 3):
                result["rows"].append({"n_vars": n1, "polys": B, "stage_ms": None, "commit_ms": None, "commit_hiding_ms": None, "open_ms": None, "open_hiding_ms": None})
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result))
        return
    result["measured_on_mi355x"] = True
    for n1 in sizes:
        n, N = n1 - 1, 1 << (n1 - 1)
        for B in (1, 3):
            cfg = WhirConfig.derive(n1, batch_size=B + 1)
            cfg.pow_bits, cfg.final_pow_bits = [4.0] * cfg.n_rounds, 4.0
            f = [ctx.upload(random_field(N, 10 + b)) for b in range(B)]
            ext = [ctx.alloc_fe(2 * N) for _ in range(B + 1)]
            for b in range(B):
                ctx.zero(ext[b], 64 * N)
            table_ptrs = ptrs(ext)

            def stage():
                assert pk_probes.lib.pk_probe_whir_hiding_fill(ctx.handle, table_ptrs, B, n, KEY, 0) == 0

            t_stage, min_stage = timed(stage, args.reps)
            hiding, plain = whir_pcs.Scheme(ctx, cfg, hiding=True), whir_pcs.Scheme(ctx, cfg)
            holder = {}

            def commit_hiding():
                if "h" in holder:
                    holder["h"].close()
                holder["h"] = hiding.commit_hiding(f)

            def commit_plain():
                if "p" in holder:
                    holder["p"].close()
                holder["p"] = plain.commit(ext)

            commits = ab({"commit": commit_plain, "commit_hiding": commit_hiding}, args.reps)
            q = 8
            pts = random_field(q * n, 5).reshape(q, n, 4)
            ext_pts = random_field(q * n1, 6).reshape(q, n1, 4)
            ext_pts[:, 0] = 0  # the plain opening at points of the same form, (0, z)
            ext_pts[:, 1:] = pts
            t_open, t_open_hiding = [], []
            for rep in range(args.reps + 1):  # the first round warms both sides
                commit_hiding()
                t0 = time.perf_counter()
                evals, proof = hiding.open_hiding(holder["h"], pts)
                t1 = time.perf_counter()
                plain.open(holder["p"], ext_pts)
                t2 = time.perf_counter()
                if rep:
                    t_open_hiding.append(t1 - t0)
                    t_open.append(t2 - t1)
            ok = whir_pcs.verify_hiding(cfg, pts, proof, expected_root=holder["h"].root())[0].accepted
            written = (B + 2) * N * 32
            row = {"n_vars": n1, "polys": B, "q": q, "stage_ms": round(1e3 * t_stage, 4), "stage_min_ms": round(1e3 * min_stage, 4),
                   "stage_grid": int(pk_probes.lib.pk_probe_whir_hiding_grid(B, n)), "stage_bytes_written": written,
                   "stage_gbps": round(written / t_stage / 1e9, 1), "stage_gblocks_per_s_lower_bound": round(written / 64 / t_stage / 1e9, 3),
                   "commit": commits["commit"], "commit_hiding": commits["commit_hiding"],
                   "commit_hiding_minus_commit_ms": round(commits["commit_hiding"]["median_ms"] - commits["commit"]["median_ms"], 4),
                   "open_ms": round(1e3 * statistics.median(t_open), 3), "open_hiding_ms": round(1e3 * statistics.median(t_open_hiding), 3),
                   "open_spread": round((max(t_open) - min(t_open)) / statistics.median(t_open), 3),
                   "open_hiding_spread": round((max(t_open_hiding) - min(t_open_hiding)) / statistics.median(t_open_hiding), 3),
                   "proof_bytes": len(proof), "verified": bool(ok)}
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            for x in (holder["h"], holder["p"], hiding, plain):
                x.close()
            for x in (*f, *ext):
                x.free()
    # tools/whir_pcs_bench.py's commit/open row, as that tool measures it
    n = 20
    cfg = WhirConfig.derive(n, batch_size=2)
    polys = [ctx.upload(random_field(1 << n, 10 + b)) for b in range(2)]
    scheme = whir_pcs.Scheme(ctx, cfg)
    pts = random_field(8 * n, 5).reshape(8, n, 4)
    holder = {}

    def commit():
        if "c" in holder:
            holder["c"].close()
        holder["c"] = scheme.commit(polys)

    runs = []
    for _ in range(3):  # the tool's own run-to-run spread, in one process
        t_commit, _ = timed(commit, args.reps)
        t_open, _ = timed(lambda: scheme.open(holder["c"], pts), args.reps)
        runs.append({"commit_ms": round(1e3 * t_commit, 3), "open_ms": round(1e3 * t_open, 3)})
    result["plain_guard"] = {"n_vars": n, "batch": 2, "q": 8, "runs": runs}
    print(json.dumps(result["plain_guard"]), flush=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
