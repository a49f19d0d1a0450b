#!/usr/bin/env python3
"""What a rank of a device set still does in full in pkw_commit and pkw_open, on ONE GPU: the kernel time of one rank of G against
the lone scheme's, and from the two the share that is not divided by G.  No scaling curve: G ranks on one GPU time-slice it, so
nothing here is a speed; the ranks take turns between collectives (whir_pcs_helpers.HostSet over the library's host transport), so
that pk_profile_* times each rank's kernels as if it had the chip to itself.  The library's own evaluation kernel runs on the
scheme's stream, outside pk_profile_*: its full grid and a rank's slice are timed by the slice probe on an idle context and added.

    python tools/whir_pcs_sharded_profile.py [--n 22] [--batch 2] [--ranks 8] [--points 8] [--out profiles/r20_whir_pcs_sharded_profile.json]

Model, as tools/sharded_profile.py: T_rank = R + (T_lone - R) / G, so R = (T_rank - T_lone / G) / (1 - 1 / G); reported as a share of
the lone time and of the rank's own time."""
import argparse
import ctypes as C
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from whir_pcs_helpers import HostSet, ptrs  # noqa: E402


def kernel_ms(prof):
    return sum(v[1] for k, v in prof.items() if not k.startswith("comm_"))


def profiled(c, cfg, polys, pts):
    """commit and open on context c after one warm-up of both -> ({kernel: ms} of the commit, of the opening, root, proof)"""
    from provekit_amd import whir_pcs

    scheme = whir_pcs.Scheme(c, cfg)
    d_polys = [c.upload(p) for p in polys]
    scheme.open(scheme.commit(d_polys), pts)  # twiddle tables, workspaces, the pattern
    c.sync()
    c.profile(True)
    c.profile_reset()
    com = scheme.commit(d_polys)
    c.sync()
    commit = c.profile_read()
    c.profile_reset()
    _, proof = scheme.open(com, pts)
    c.sync()
    opening = c.profile_read()
    c.profile(False)
    root = com.root()
    for x in (com, scheme, *d_polys):
        (x.close if hasattr(x, "close") else x.free)()
    return commit, opening, root, proof


def share(t_lone, t_rank, G):
    R = (t_rank - t_lone / G) / (1.0 - 1.0 / G)
    return {"lone_kernel_ms": round(t_lone, 3), "rank_kernel_ms": round(t_rank, 3), "rank_over_lone": round(t_rank / t_lone, 4), "ideal": round(1.0 / G, 4),
            "not_divided_ms": round(R, 3), "not_divided_share_of_lone": round(R / t_lone, 4), "not_divided_share_of_rank": round(R / t_rank, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=22)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_whir_pcs_sharded_profile.json"))
    args = ap.parse_args()
    import torch  # torch's HIP runtime first, as tests/conftest.py does

    torch.cuda.is_available()
    import pk_probes
    import provekit_amd
    from provekit_amd import whir_pcs
    from provekit_amd.field import random_field
    from provekit_amd.scheme import WhirConfig

    n, batch, G, q = args.n, args.batch, args.ranks, args.points
    cfg = WhirConfig.derive(n, batch_size=batch)
    polys = [random_field(1 << n, 10 + b) for b in range(batch)]
    pts = random_field(q * n, 5).reshape(q, n, 4)
    ctx = provekit_amd.Context(0)
    lone_commit, lone_open, root, proof = profiled(ctx, cfg, polys, pts)
    assert whir_pcs.verify(cfg, pts, proof, expected_root=root)[0].accepted

    # the evaluation kernel, a pass of up to 8 points at a time: the full grid against the slice of one rank of G
    n_wg = pk_probes.lib.pk_probe_whir_eval_grid(n)
    sliced = n_wg >= G and n_wg % G == 0
    d_polys = [ctx.upload(p) for p in polys]
    part = (C.c_uint64 * (4 * batch * 8 * n_wg))()

    def eval_ms(count):
        total = 0.0
        for q0 in range(0, q, 8):
            runs = []
            for _ in range(4):  # the first call warms; the least of the rest
                ms = C.c_float()
                rc = pk_probes.lib.pk_probe_whir_eval_slice(ctx.handle, ptrs(d_polys), batch, n, pts[q0:].ctypes.data, min(8, q - q0), 0, count, part, C.byref(ms))
                assert rc == 0
                runs.append(ms.value)
            total += min(runs[1:])
        return total

    eval_full, eval_rank = eval_ms(n_wg), eval_ms(n_wg // G if sliced else n_wg)
    for b in d_polys:
        b.free()

    hs = HostSet(G, take_turns=True)
    out, err = [None] * G, []

    def go(r):
        try:
            hs.begin(r)
            out[r] = profiled(hs.ctxs[r], cfg, polys, pts)
            hs.end(r)
        except BaseException as e:  # noqa: BLE001
            err.append(e)

    ths = [threading.Thread(target=go, args=(r,), daemon=True) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=600)
    if err:
        raise err[0]
    assert not any(t.is_alive() for t in ths), "a rank did not come back"
    assert all(o[2] == root and o[3] == proof for o in out), "a rank's root or proof differs from the lone scheme's"
    worst = max(range(G), key=lambda r: kernel_ms(out[r][0]) + kernel_ms(out[r][1]))
    rank_commit, rank_open = out[worst][0], out[worst][1]
    by_kernel = lambda prof: {k: round(v[1], 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
    report = {
        "tool": "tools/whir_pcs_sharded_profile.py", "measured_on_mi355x": True,
        "setting": f"ONE GPU: {G} ranks over the host transport taking turns between collectives; kernel time per rank, no wall time, no scaling curve",
        "n_vars": n, "batch": batch, "ranks": G, "points": q, "proof_bytes": len(proof), "roots_and_proofs_identical": True,
        "evaluation_kernel": {"workgroups": n_wg, "sliced": sliced, "full_grid_ms": round(eval_full, 4), "rank_slice_ms": round(eval_rank, 4)},
        "pkw_commit": share(kernel_ms(lone_commit), kernel_ms(rank_commit), G),
        "pkw_open": share(kernel_ms(lone_open) + eval_full, kernel_ms(rank_open) + eval_rank, G),
        "collectives_per_rank": {"count": len(hs.log[0]), "bytes_per_rank": sorted(set(hs.log[0]))},
        "lone_commit_ms_by_kernel": by_kernel(lone_commit), "rank_commit_ms_by_kernel": by_kernel(rank_commit),
        "lone_open_ms_by_kernel": by_kernel(lone_open), "rank_open_ms_by_kernel": by_kernel(rank_open),
    }
    both_lone = kernel_ms(lone_commit) + kernel_ms(lone_open) + eval_full
    both_rank = kernel_ms(rank_commit) + kernel_ms(rank_open) + eval_rank
    report["commit_and_open"] = share(both_lone, both_rank, G)
    hs.close()
    ctx.close()
    json.dump(report, open(args.out, "w"), indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
