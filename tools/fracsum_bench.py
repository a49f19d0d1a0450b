#!/usr/bin/env python3
"""What a lookup costs with and without helper columns on one device (libprovekit_fracsum.so against libprovekit_lookup.so), per
(n, k), in runs that alternate between the two ways on the same tables.  Medians with the spread (min .. max) of `--reps` runs after one
warm-up; every proof and opening of the warm-up is verified.

  (a) the argument alone: pkf_lookup_prove against pkl_begin + pkl_finish (the multiplicities are made once, outside both);
  (b) end to end with WHIR commitments and openings: LogUp-GKR commits f and {t, m} in one phase and opens at two points; helper-column
      LogUp commits f and {t, m}, then h_f and h_t in a second phase, and opens f, {t, m}, h_f (two points) and h_t (two points);
  (c) where pkf_lookup_prove's time goes per side: the leaf-and-tree phase and the combine passes (device events), the layers'
      pks_prove (host clock), and the layers up to the tail's limit by themselves.

One yardstick rides along: the tree kernels by themselves (tools/probes/fracsum.hip) at 1, 2 and 3 layers per launch, alternating on the
same tables, with and without numerators, with the bytes each variant moves and its GB/s.

usage: python tools/fracsum_bench.py [--sizes 16:8,20:16,24:20] [--reps 5] [--no-end-to-end] [--out profiles/r28_fracsum_bench.json]"""
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
from provekit_amd import fracsum as fs, lookup, whir_pcs  # noqa: E402
from provekit_amd.field import random_field  # noqa: E402
from provekit_amd.scheme import WhirConfig  # noqa: E402
from tools.pk_probes import lib as probes  # noqa: E402

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HALF = np.frombuffer(((P + 1) // 2 * (1 << 256) % P).to_bytes(32, "little"), dtype="<u8").copy()  # (p + 1) / 2, Montgomery


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def tree_bytes(n, s, unit):
    """what the tree kernels move at s layers per launch: every launch reads the layer it starts from (both arrays, or the denominators
    alone over unit leaves) and writes both arrays of the layers it makes"""
    t, d, total, first = fs.tail_max_n(), n, 0, True
    while d > 0:
        step = min(s, d - t) if d > t else d  # the tail takes everything that is left
        total += 32 * (1 if first and unit else 2) * (1 << d)
        total += 64 * sum(1 << (d - k) for k in range(1, step + 1))
        d -= step
        first = False
    return total


def side_profile(handle, side, size):
    inner = probes.pk_probe_fracsum_lookup_side(handle, side)
    tree_ms, combine_ms, layer_ms = C.c_double(), (C.c_double * 28)(), (C.c_double * 28)()
    assert probes.pk_probe_fracsum_profile(inner, C.byref(tree_ms), combine_ms, layer_ms) == 0
    t = fs.tail_max_n()
    return {"tree_ms": tree_ms.value, "combine_ms": sum(combine_ms[d] for d in range(1, size)), "layers_ms": sum(layer_ms[d] for d in range(1, size)),
            "layers_up_to_tail_ms": sum(layer_ms[d] + combine_ms[d] for d in range(1, min(size, t + 1)))}


class Case:
    """t random (distinct with overwhelming probability), f drawn from it, m made by pkl_multiplicities"""

    def __init__(self, ctx, n, k):
        self.ctx, self.n, self.k = ctx, n, k
        t = random_field(1 << k, 1).reshape(-1, 4)
        idx = np.random.default_rng(2).integers(0, 1 << k, size=1 << n, dtype=np.uint32)
        self.d_t, self.d_f, self.d_idx, self.d_m = ctx.upload(t), ctx.upload(t[idx]), ctx.upload(idx), ctx.alloc_fe(1 << k)
        self.helper = lookup.LookupProver(ctx, lookup.Statement(n, k, 2, 2))
        self.helper.multiplicities(self.d_f, self.d_t, self.d_idx, self.d_m)
        self.gkr = fs.LookupProver(ctx, fs.LookupStatement(n, k, 2))
        self.bind = random_field(2, 3).reshape(-1, 4)

    def close(self):
        self.helper.close()
        self.gkr.close()
        for b in (self.d_t, self.d_f, self.d_idx, self.d_m):
            b.free()


def bench_argument(case, reps):
    """(a) and (c)"""
    n, k = case.n, case.k
    times = {"pkf_lookup_prove": [], "pkl_begin+pkl_finish": []}
    sides = {"F": [], "T": []}
    for rep in range(reps + 1):
        ms_gkr, (proof, _) = timed(lambda: case.gkr.prove(case.d_f, case.d_t, case.d_m, case.bind))
        prof = {"F": side_profile(case.gkr.handle, 0, n), "T": side_profile(case.gkr.handle, 1, k)}

        def helper():
            case.helper.begin(case.d_t, case.d_idx, case.bind)
            return case.helper.finish(case.bind)

        case.helper.multiplicities(case.d_f, case.d_t, case.d_idx, case.d_m)  # outside both: each way needs m
        ms_helper, (helper_proof, _) = timed(helper)
        if rep == 0:  # warm-up, and the proofs are proofs
            assert fs.lookup_verify(case.gkr.stmt, proof, case.bind)[0].accepted
            assert lookup.verify(case.helper.stmt, helper_proof, case.bind, case.bind)[0].accepted
            continue
        times["pkf_lookup_prove"].append(ms_gkr), times["pkl_begin+pkl_finish"].append(ms_helper)
        for side in sides:
            sides[side].append(prof[side])
    row = {"measure": "argument", "n": n, "k": k, "ms": {name: spread(v) for name, v in times.items()},
           "proof_bytes": {"pkf": case.gkr.proof_bytes, "pkl": lookup.proof_bytes(case.helper.stmt)},
           "arena_bytes": {"pkf": fs.arena_bytes(case.gkr.stmt), "pkl": lookup.arena_bytes(case.helper.stmt)},
           "sumcheck_round_trips": n * (n - 1) // 2 + k * (k - 1) // 2,
           "pkf_split": {side: {key: spread([p[key] for p in v]) for key in v[0]} for side, v in sides.items()}}
    row["pkf_over_pkl"] = row["ms"]["pkf_lookup_prove"]["median"] / row["ms"]["pkl_begin+pkl_finish"]["median"]
    print(json.dumps(row), flush=True)
    return row


def bench_end_to_end(case, reps):
    """(b): commitments, the argument and openings, both ways"""
    ctx, n, k = case.ctx, case.n, case.k
    cfg_n1, cfg_k2, cfg_k1 = WhirConfig.derive(n, batch_size=1), WhirConfig.derive(k, batch_size=2), WhirConfig.derive(k, batch_size=1)
    s_n1, s_k2, s_k1 = whir_pcs.Scheme(ctx, cfg_n1), whir_pcs.Scheme(ctx, cfg_k2), whir_pcs.Scheme(ctx, cfg_k1)
    half_n, half_k = np.tile(HALF, (n, 1)), np.tile(HALF, (k, 1))

    def roots(*coms):
        limbs = np.zeros((len(coms), 4), dtype=np.uint64)
        for i, com in enumerate(coms):
            limbs[i, :3] = np.frombuffer(com.root(), dtype="<u8")[:3]  # 192 bits of the digest: an element below p
        return limbs

    def gkr():
        com_f, com_tm = s_n1.commit([case.d_f]), s_k2.commit([case.d_t, case.d_m])
        proof, claims = case.gkr.prove(case.d_f, case.d_t, case.d_m, roots(com_f, com_tm))
        opened = [(cfg_n1, claims.z_f[None], com_f, s_n1.open(com_f, claims.z_f[None])), (cfg_k2, claims.z_t[None], com_tm, s_k2.open(com_tm, claims.z_t[None]))]
        return proof, claims, opened

    def helper():
        com_f, com_tm = s_n1.commit([case.d_f]), s_k2.commit([case.d_t, case.d_m])
        _, h_f, h_t = case.helper.begin(case.d_t, case.d_idx, roots(com_f, com_tm))
        com_hf, com_ht = s_n1.commit([h_f]), s_k1.commit([h_t])  # the second phase: the helper columns exist only after alpha
        proof, c = case.helper.finish(roots(com_hf, com_ht))
        at_f, at_t = np.stack([c.r_f, half_n]), np.stack([c.r_t, half_k])
        opened = [(cfg_n1, c.r_f[None], com_f, s_n1.open(com_f, c.r_f[None])), (cfg_k2, c.r_t[None], com_tm, s_k2.open(com_tm, c.r_t[None])),
                  (cfg_n1, at_f, com_hf, s_n1.open(com_hf, at_f)), (cfg_k1, at_t, com_ht, s_k1.open(com_ht, at_t))]
        return proof, c, opened

    def check(opened):
        total = 0
        for cfg, points, com, (evals, opening) in opened:
            res, bound = whir_pcs.verify(cfg, points, opening, expected_root=com.root())
            assert res.accepted and np.array_equal(bound, evals), res
            total += len(opening)
        return total

    def close(opened):
        for com in {id(o[2]): o[2] for o in opened}.values():
            com.close()

    times, sizes = {"logup_gkr": [], "logup_helper_columns": []}, {}
    for rep in range(reps + 1):
        for name, run in (("logup_gkr", gkr), ("logup_helper_columns", helper)):  # alternating
            case.helper.multiplicities(case.d_f, case.d_t, case.d_idx, case.d_m)  # outside both: each way needs m
            ms, (proof, claims, opened) = timed(run)
            if rep == 0:
                sizes[name] = {"proof_bytes": len(proof), "opening_bytes": check(opened), "commitments": len({id(o[2]) for o in opened}), "openings": len(opened)}
                if name == "logup_gkr":
                    assert np.array_equal(opened[0][3][0][0, 0], claims.f_value) and np.array_equal(opened[1][3][0][1, 0], claims.m_value)
            else:
                times[name].append(ms)
            close(opened)
    row = {"measure": "end_to_end", "n": n, "k": k, "ms": {name: spread(v) for name, v in times.items()}, "sizes": sizes,
           "commitment_phases": {"logup_gkr": 1, "logup_helper_columns": 2}}
    row["gkr_over_helper"] = row["ms"]["logup_gkr"]["median"] / row["ms"]["logup_helper_columns"]["median"]
    print(json.dumps(row), flush=True)
    for s in (s_n1, s_k2, s_k1):
        s.close()
    return row


def tree_ab(ctx, n, reps):
    """1, 2 and 3 layers per launch, alternating, with numerators and over unit leaves"""
    rows = []
    d_p, d_q = ctx.upload(random_field(1 << n, 20).reshape(-1, 4)), ctx.upload(random_field(1 << n, 21).reshape(-1, 4))
    d_pt, d_qt = ctx.alloc_fe(1 << n), ctx.alloc_fe(1 << n)
    ms = C.c_float()
    for unit in (0, 1):
        ts = {s: [] for s in (1, 2, 3)}
        for rep in range(reps + 1):
            for s in ts:  # alternating
                ctx._check(probes.pk_probe_fracsum_tree(ctx.handle, n, None if unit else d_p.ptr, d_q.ptr, d_pt.ptr, d_qt.ptr, s, 0, C.byref(ms)))
                if rep:
                    ts[s].append(ms.value)
        row = {"measure": "tree_ab", "n": n, "unit": unit, "layers_per_launch": {}}
        for s, v in ts.items():
            nbytes = tree_bytes(n, s, unit)
            row["layers_per_launch"][str(s)] = {"ms": spread(v), "bytes": nbytes, "GB_per_s": nbytes / (statistics.median(v) * 1e-3) / 1e9}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for b in (d_p, d_q, d_pt, d_qt):
        b.free()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16:8,20:16,24:20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in pair.split(":")) for pair in args.sizes.split(",")]
    ctx = provekit_amd.Context(0)
    result = {"tool": "tools/fracsum_bench.py", "reps": args.reps, "tail_max_n": fs.tail_max_n(), "default_layers_per_launch": probes.pk_probe_fracsum_default_layers(),
              "clocks": "ms of calls and layers_ms: host clock around blocking calls; tree_ms, combine_ms and tree_ab: device events", "argument": [],
              "end_to_end": [], "tree_ab": []}
    for n, k in sizes:
        case = Case(ctx, n, k)
        result["argument"].append(bench_argument(case, args.reps))
        if not args.no_end_to_end:
            result["end_to_end"].append(bench_end_to_end(case, args.reps))
        case.close()
        result["tree_ab"] += tree_ab(ctx, n, args.reps)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
