"""GPU: libprovekit_whir.so on the contexts of a device set (include/provekit_whir.h, "Device sets").  G ranks on ONE GPU over the
library's in-process transport, one host thread per rank, every rank making the same calls with the same inputs: each rank's root,
evaluations, sums and proof bytes against a lone scheme's on the fixture context, for the four statement forms, at sizes on both
sides of the product's thresholds (2^11 local rows: the scaled leaf encoding; 2^13 rows per rank: the subtree-sharded heap) and of
the slice rule (fewer evaluation workgroups than ranks: the replicated pass).  Then the hiding key of rank 0, the ranks' refusal of
a statement they disagree on, and the slice kernels with the finish kernel over gathered blocks on one context."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_config_cases as CC  # noqa: E402
import whir_pcs_linear_cases as L  # noqa: E402

P_LIMBS = np.array([(K.P - 1) >> (64 * i) & (2**64 - 1) for i in range(4)], dtype=np.uint64)  # p - 1: the largest memory image
# (n_vars, G) at folding factor 2 and rate 1/2: rows = 2^(n - 1).  n = 10: the whole heap on every rank, and at G = 8 four evaluation
# workgroups for eight ranks; n = 14: 2^12 local rows, scaled leaves, whole heap; n = 16: the sharded heap (exactly 2^13 rows per rank
# at G = 4), with round commits below the thresholds again
SHAPES = [(10, 2), (10, 4), (10, 8), (14, 2), (16, 2), (16, 4)]
POINT_COUNTS = (1, 9, 64)  # one pass, a second pass, the most
WEIGHT_COUNTS = (1, 5)
LINEAR_POINTS = 2
KEY = bytes(range(7, 39))
JOIN_SECONDS = 120


def run_ranks(ctxs, fn):
    """fn(rank, ctx) on one thread per rank -> the ranks' results; re-raises the first failure; a rank that is not back after
    JOIN_SECONDS is a failure (nothing is retried)"""
    out, err = [None] * len(ctxs), []

    def go(r):
        try:
            out[r] = fn(r, ctxs[r])
        except BaseException as e:  # noqa: BLE001
            err.append(e)

    ths = [threading.Thread(target=go, args=(r,), daemon=True) for r in range(len(ctxs))]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=JOIN_SECONDS)
    if err:
        raise err[0]
    assert not any(t.is_alive() for t in ths), "a rank did not come back"
    return out


@pytest.fixture()
def rank_sets():
    import torch

    torch.cuda.is_available()
    import provekit_amd

    made = []

    def make(G):
        cs = provekit_amd.Context.create_set([0] * G)
        made.append(cs)
        return cs

    yield make
    for cs in made:
        for c in cs:
            c.close()


def config(n, batch):
    return CC.config(n, 2, 1, batch)


# ---- the inputs: Montgomery memory images, the same on every rank ------------------------------------------------------------------
def tables(n, count, seed):
    from provekit_amd.field import random_field

    out = [random_field(1 << n, seed + 11 * b) for b in range(count)]
    for t in out:
        t[0], t[-1] = 0, P_LIMBS
    return out


def point_set(n, q, seed=5):
    from provekit_amd.field import random_field

    p = random_field(q * n, seed + q).reshape(q, n, 4)
    p[0, 0] = P_LIMBS
    if q >= 3:
        p[1, n // 2], p[-1] = 0, p[0]
    return p


def sparse_lists(n, l, seed=41):
    """l index/value lists: a random eighth of the positions; no entry; index 0; index 2^n - 1; a random third"""
    from provekit_amd.field import random_field

    N, rng = 1 << n, np.random.default_rng(seed)
    picks = [np.sort(rng.choice(N, size=N // 8, replace=False)), np.zeros(0, dtype=np.int64), np.array([0]), np.array([N - 1]),
             np.sort(rng.choice(N, size=N // 3, replace=False))]
    out = []
    for i in range(l):
        vals = random_field(max(len(picks[i]), 1), seed + i)[: len(picks[i])]
        if len(vals):
            vals[-1] = P_LIMBS
        out.append((picks[i].astype(np.uint32), vals))
    return out


def statement_inputs(oracle, n, batch):
    return {"polys": tables(n, batch, 3), "points": {q: point_set(n, q) for q in POINT_COUNTS + (LINEAR_POINTS,)},
            "weights": tables(n, max(WEIGHT_COUNTS), 23), "tags": L.mont(oracle, L.tags(max(WEIGHT_COUNTS))), "lists": sparse_lists(n, max(WEIGHT_COUNTS))}


def commit_and_open_everything(c, cfg, inp):
    """on context c: commit, then every opening of this file -> {name: (root | (evaluations, sums, proof))}"""
    from provekit_amd import whir_pcs

    scheme = whir_pcs.Scheme(c, cfg)
    d_polys, d_weights = [c.upload(t) for t in inp["polys"]], [c.upload(t) for t in inp["weights"]]
    com = scheme.commit(d_polys)
    out = {"root": com.root()}
    for q in POINT_COUNTS:
        evals, proof = scheme.open(com, inp["points"][q])
        out[f"open q={q}"] = (evals.tobytes(), b"", proof)
    pts = inp["points"][LINEAR_POINTS]
    for l in WEIGHT_COUNTS:
        evals, sums, proof = scheme.open_linear(com, pts, d_weights[:l], inp["tags"][:l])
        out[f"open_linear l={l}"] = (evals.tobytes(), sums.tobytes(), proof)
        lists = whir_pcs.SparseWeights(inp["lists"][:l]).upload(c)
        evals, sums, proof = scheme.open_sparse(com, pts, lists, inp["tags"][:l])
        out[f"open_sparse l={l}"] = (evals.tobytes(), sums.tobytes(), proof)
        lists.free()
    for x in (com, scheme, *d_polys, *d_weights):
        (x.close if hasattr(x, "close") else x.free)()
    return out


_lone = {}


def lone_reference(ctx, oracle, n, batch):
    """the lone scheme's results on the fixture context, computed once per (n, batch), each proof accepted by its verifier"""
    from provekit_amd import whir_pcs

    if (n, batch) in _lone:
        return _lone[n, batch]
    cfg, inp = config(n, batch), statement_inputs(oracle, n, batch)
    ref = commit_and_open_everything(ctx, cfg, inp)
    for q in POINT_COUNTS:
        res, evals = whir_pcs.verify(cfg, inp["points"][q], ref[f"open q={q}"][2], expected_root=ref["root"])
        assert res.accepted and evals.tobytes() == ref[f"open q={q}"][0], (q, res)
    pts = inp["points"][LINEAR_POINTS]
    for l in WEIGHT_COUNTS:
        v = whir_pcs.verify_linear(cfg, pts, inp["tags"][:l], inp["weights"][:l], ref[f"open_linear l={l}"][2], expected_root=ref["root"])
        assert v.result.accepted and v.unchecked == 0 and v.sums.tobytes() == ref[f"open_linear l={l}"][1], (l, v.result)
        v = whir_pcs.verify_sparse(cfg, pts, inp["tags"][:l], whir_pcs.SparseWeights(inp["lists"][:l]), ref[f"open_sparse l={l}"][2],
                                   expected_root=ref["root"])
        assert v.result.accepted and v.sums.tobytes() == ref[f"open_sparse l={l}"][1], (l, v.result)
    _lone[n, batch] = (cfg, inp, ref)
    return _lone[n, batch]


def test_the_shapes_straddle_the_thresholds_they_were_chosen_for(ctx):
    import pk_probes

    grid = pk_probes.lib.pk_probe_whir_eval_grid
    assert [grid(n) for n in (8, 9, 10, 14, 16)] == [1, 2, 4, 64, 256]
    assert grid(10) < 8 and grid(10) % 4 == 0  # G = 8 at n = 10: the replicated pass; G = 2, 4: slices
    rows = {n: 1 << (n - 1) for n, _ in SHAPES}  # folding factor 2, rate 1/2
    assert rows[10] // 2 < 1 << 11 <= rows[14] // 2 < 1 << 13  # the scaled leaf encoding starts between n = 10 and n = 14 ...
    assert rows[16] // 2 >= 1 << 13 and rows[16] // 4 == 1 << 13  # ... the sharded heap at n = 16, exactly at G = 4
    assert all(rows[n] >= 64 * G for n, G in SHAPES)  # every committed codeword is sharded by leaf index


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("n,G", SHAPES)
def test_every_rank_gets_the_lone_schemes_root_and_proof_bytes(ctx, oracle, rank_sets, n, G, batch):
    cfg, inp, ref = lone_reference(ctx, oracle, n, batch)
    got = run_ranks(rank_sets(G), lambda r, c: commit_and_open_everything(c, cfg, inp))
    for r in range(G):
        assert got[r].keys() == ref.keys()
        for name in ref:
            assert got[r][name] == ref[name], (r, name)


def hiding_inputs(n):
    return tables(n - 1, 1, 61), point_set(n - 1, 3, seed=71)


def commit_and_open_hiding(c, cfg, polys, pts, seed):
    from provekit_amd import whir_pcs

    scheme = whir_pcs.Scheme(c, cfg, hiding=True)
    d_polys = [c.upload(t) for t in polys]
    com = scheme.commit_hiding(d_polys, seed=seed)
    root = com.root()
    evals, proof = scheme.open_hiding(com, pts)
    with pytest.raises(Exception, match="already opened"):  # per-rank state, the same on every rank: refused before any collective
        scheme.open_hiding(com, pts)
    for x in (com, scheme, *d_polys):
        (x.close if hasattr(x, "close") else x.free)()
    return root, evals.tobytes(), proof


@pytest.mark.parametrize("n,G", SHAPES)
def test_hiding_commitments_under_a_given_seed_are_the_lone_schemes(ctx, rank_sets, n, G):
    from provekit_amd import whir_pcs

    cfg = config(n, 2)  # one polynomial of n - 1 variables and g
    polys, pts = hiding_inputs(n)
    ref = commit_and_open_hiding(ctx, cfg, polys, pts, KEY)
    res, evals = whir_pcs.verify_hiding(cfg, pts, ref[2], expected_root=ref[0])
    assert res.accepted and evals.tobytes() == ref[1], res
    got = run_ranks(rank_sets(G), lambda r, c: commit_and_open_hiding(c, cfg, polys, pts, KEY))
    assert all(g == ref for g in got)


def test_without_a_seed_the_set_commits_under_rank_0s_key(ctx, rank_sets):
    from provekit_amd import whir_pcs

    n, G = 10, 2
    cfg = config(n, 2)
    polys, pts = hiding_inputs(n)
    got = run_ranks(rank_sets(G), lambda r, c: commit_and_open_hiding(c, cfg, polys, pts, None))
    assert got[0] == got[1]  # one batch: the same root, evaluations and bytes
    res, evals = whir_pcs.verify_hiding(cfg, pts, got[0][2], expected_root=got[0][0])
    assert res.accepted and evals.tobytes() == got[0][1], res
    again = run_ranks(rank_sets(G), lambda r, c: commit_and_open_hiding(c, cfg, polys, pts, None))
    assert again[0][0] != got[0][0]  # a fresh key per commitment


def test_ranks_that_disagree_on_the_points_all_refuse_and_the_set_stays_usable(ctx, oracle, rank_sets):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    n, G, q = 10, 2, 9
    cfg, inp, ref = lone_reference(ctx, oracle, n, 1)
    other = inp["points"][q].copy()
    other[4, 3] = P_LIMBS  # one coordinate of one point, on rank 1 alone

    def fn(r, c):
        scheme = whir_pcs.Scheme(c, cfg)
        d_polys = [c.upload(t) for t in inp["polys"]]
        com = scheme.commit(d_polys)
        with pytest.raises(ProveKitHipError, match="ranks disagree on the statement") as e:
            scheme.open(com, other if r == 1 else inp["points"][q])
        evals, proof = scheme.open(com, inp["points"][q])
        for x in (com, scheme, *d_polys):
            (x.close if hasattr(x, "close") else x.free)()
        return e.value.code, evals.tobytes(), proof

    for code, evals, proof in run_ranks(rank_sets(G), fn):
        assert code == -1  # PK_ERR_BAD_ARG
        assert (evals, b"", proof) == ref[f"open q={q}"]


def test_one_gather_per_pass_carries_a_slices_partials_and_its_status(ctx, oracle):
    """Over the host transport, whose callback sees every collective: an opening starts with one all-gather per pass of a sliced
    reduction (a rank's partials and one status element), then the 64-byte comparison of the sponges; the deferred values of dense
    weights end it, four tables a pass.  With fewer workgroups than ranks no pass gathers.  The bytes are the lone scheme's here too"""
    import pk_probes
    from provekit_amd import whir_pcs
    from whir_pcs_helpers import HostSet

    n, batch, q, l = 10, 2, 9, 5
    cfg, inp, ref = lone_reference(ctx, oracle, n, batch)
    assert pk_probes.lib.pk_probe_whir_eval_grid(n) == 4 == pk_probes.lib.pk_probe_whir_wsum_grid(n)
    for G, per in ((2, 2), (8, 0)):
        hs = HostSet(G)

        def fn(r, c):
            scheme = whir_pcs.Scheme(c, cfg)
            d_polys, d_weights = [c.upload(t) for t in inp["polys"]], [c.upload(t) for t in inp["weights"][:l]]
            com = scheme.commit(d_polys)
            at = len(hs.log[r])
            _, proof = scheme.open(com, inp["points"][q])
            mid = len(hs.log[r])
            _, _, linear = scheme.open_linear(com, inp["points"][LINEAR_POINTS], d_weights, inp["tags"][:l])
            seen = hs.log[r][at:mid], hs.log[r][mid:]
            for x in (com, scheme, *d_polys, *d_weights):
                (x.close if hasattr(x, "close") else x.free)()
            return proof, linear, seen

        try:
            got = run_ranks(hs.ctxs, fn)
        finally:
            hs.close()
        block = lambda outputs: 32 * (outputs * per + 1)
        for proof, linear, (points_log, linear_log) in got:
            assert proof == ref[f"open q={q}"][2] and linear == ref[f"open_linear l={l}"][2]
            if per:
                assert points_log[:3] == [block(batch * 8), block(batch * 8), 64]  # two passes of 8 and 1 points, then the sponges
                assert linear_log[:3] == [block(batch * 8), block(batch * l), 64]  # the points, the sums, the sponges
                assert linear_log[-2:] == [block(4 * 8), block(1 * 8)]  # the deferred values of 4 + 1 tables
            else:
                assert points_log[0] == 64 and linear_log[0] == 64  # nothing before the sponges


# ---- the slices on one context --------------------------------------------------------------------------------------------------------
def slice_cut(n_wg, G):
    """(workgroups per slice, slices): the library's rule -- G slices when G divides n_wg, else the whole grid as one"""
    return (n_wg // G, G) if n_wg >= G and n_wg % G == 0 else (n_wg, 1)


def finished_union(ctx, launch_slice, n_wg, G, rows, count, row_stride):
    """the finish kernel over the blocks of all slices, one element apart as the exchange leaves them (its status word)"""
    import pk_probes

    per, slices = slice_cut(n_wg, G)
    block = rows * row_stride * per
    gathered = np.full((slices, block + 1, 4), 0xDEADBEEF, dtype=np.uint64)  # the gaps are never read
    for g in range(slices):
        part = np.zeros((block, 4), dtype=np.uint64)
        assert launch_slice(g * per, per, part.ctypes.data) == 0
        gathered[g, :block] = part
    out = np.zeros((rows, count, 4), dtype=np.uint64)
    assert pk_probes.lib.pk_probe_whir_finish(ctx.handle, gathered.ctypes.data, gathered.shape[0] * gathered.shape[1], n_wg, per, block + 1, rows, count,
                                              row_stride, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("n,n_wg", [(8, 1), (9, 2), (10, 4), (16, 256)])
def test_the_finished_union_of_the_slices_is_the_full_grids_output(ctx, n, n_wg, G):
    import pk_probes
    from provekit_amd import whir_pcs

    lib = pk_probes.lib
    assert lib.pk_probe_whir_eval_grid(n) == n_wg == lib.pk_probe_whir_wsum_grid(n)
    assert slice_cut(n_wg, G)[1] == (G if n_wg >= G else 1)
    batch, Q, Lw = 2, 3, 3
    polys, weights, pts = tables(n, batch, 3), tables(n, Lw, 23), point_set(n, Q)
    d_polys, d_weights = [ctx.upload(t) for t in polys], [ctx.upload(t) for t in weights]
    full = whir_pcs.evaluate(ctx, d_polys, n, pts)
    got = finished_union(ctx, lambda first, count, out: lib.pk_probe_whir_eval_slice(ctx.handle, K.ptrs(d_polys), batch, n, pts.ctypes.data, Q, first, count, out, None),
                         n_wg, G, batch, Q, 8)
    assert np.array_equal(got, full)
    full = whir_pcs.weighted_sums(ctx, d_polys, n, d_weights)
    got = finished_union(ctx, lambda first, count, out: lib.pk_probe_whir_wsum_slice(ctx.handle, K.ptrs(d_polys), batch, n, K.ptrs(d_weights), Lw, 0, first,
                                                                                    count, 0, out, None), n_wg, G, batch, Lw, Lw)
    assert np.array_equal(got, full)
    for b in d_polys + d_weights:
        b.free()


def test_cpp_host_drives_four_ranks_to_one_root_and_one_accepted_proof():
    import subprocess

    demo = os.path.join(ROOT, "examples", "pcs_sharded_demo")
    assert os.path.exists(demo), "examples/pcs_sharded_demo is built by __graft_entry__.build()"
    out = subprocess.run([demo, "12", "4", "7"], capture_output=True, text=True, timeout=JOIN_SECONDS)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("ok n_vars=12 ranks=4 points=2 proof_bytes=") and "one root, one proof, accepted" in out.stdout
