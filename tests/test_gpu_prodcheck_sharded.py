"""GPU: the sharded product sumcheck (include/provekit_sumcheck_sharded.h).  G ranks on ONE GPU over the in-process transport, one
host thread per rank, every rank making the same calls: each rank's proof bytes, point, finals and sum against the Python reference
(tests/prodcheck_refs.py) for every shape, at the sizes where the number of sharded rounds S changes what the prover does (S = 0:
all replicated; 1: nothing stored; 2: the first hand-over; 3: the first in-place sharded round; more).  Then one rank's slice of a
round against the lone round, edge values, the caller's tables, reuse, refusals that every rank must make, and the composition with
the sharded commitment scheme."""
import functools
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prodcheck_refs as K  # noqa: E402
import prodcheck_shard_refs as R  # noqa: E402
from test_gpu_prodcheck import reference  # noqa: E402  (computed once per (shape, size), shared with the lone suite)

P = K.P
JOIN_SECONDS = 120
# (G, n) -> S with c = 8
SIZES = {(2, 9): 0, (2, 10): 1, (2, 11): 2, (2, 12): 3, (2, 14): 5, (4, 10): 0, (4, 11): 1, (4, 12): 2, (4, 13): 3, (4, 16): 6, (8, 11): 0, (8, 13): 2}


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


def refusal(call):
    """the ProveKitHipError `call` raises, as (code, message), or None.  A rank's thread asserts nothing while its peers may still be
    in a collective: it reports, and the test asserts once every rank is back"""
    from provekit_amd._lib import ProveKitHipError

    try:
        call()
    except ProveKitHipError as e:
        return e.code, str(e)
    return None


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch bundles its own HIP runtime: it must initialise it before the library is loaded, also for the tests that need no context"""
    import torch

    torch.cuda.is_available()


@pytest.fixture()
def rank_sets():
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


def smallest_n(G, S, m=3):
    """the smallest n with S sharded rounds on G ranks, from the library's plan"""
    from provekit_amd import prodcheck, prodcheck_sharded

    return next(n for n in range(1, 29) if prodcheck_sharded.plan(prodcheck.Statement(n, m, [(1, (1 << m) - 1)]), G).S == S)


@functools.lru_cache(maxsize=None)
def images(name, n):
    """the reference's tables, tau and bind as Montgomery memory images"""
    shape, tables, tau, bind = reference(name, n)[:4]
    return [K.mont(t) for t in tables], K.mont(tau) if tau is not None else None, K.mont(bind)


def prove_on_ranks(ctxs, stmt, tabs, tau, bind, repeat=1, per_rank=None):
    """every rank: upload, create, prove `repeat` times -> per rank [Proof, ...]; per_rank(r) may replace (tau, bind) on a rank"""
    from provekit_amd import prodcheck_sharded

    def fn(r, c):
        d = [c.upload(t) for t in tabs]
        prover = prodcheck_sharded.Prover(c, stmt)
        try:
            t, b = per_rank(r) if per_rank else (tau, bind)
            return [prover.prove(d, t, b) for _ in range(repeat)]
        finally:
            prover.close()
            for x in d:
                x.free()

    return run_ranks(ctxs, fn)


def test_the_sizes_have_the_sharded_rounds_they_were_chosen_for():
    from provekit_amd import prodcheck_sharded

    for (G, n), S in SIZES.items():
        p = prodcheck_sharded.plan(K.Shape("r1cs", n).statement(), G)
        assert p.S == S == max(0, n - p.c - p.g) and p.handover_len == 1 << (p.c + p.g + 1)
    for G in (2, 4, 8):  # S = 0 .. 3 are each met at their first size
        assert all((G, smallest_n(G, S)) in SIZES for S in ((1, 2, 3) if G < 8 else (2,)))


@pytest.mark.parametrize("G,n", list(SIZES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_every_ranks_bytes_are_the_references_and_are_accepted(rank_sets, name, G, n):
    from provekit_amd import prodcheck

    shape, tables, tau, bind, want, point, finals, s = reference(name, n)
    tabs, tau_m, bind_m = images(name, n)
    got = prove_on_ranks(rank_sets(G), shape.statement(), tabs, tau_m, bind_m)
    for r in range(G):
        (proof,) = got[r]
        assert len(proof.bytes) == shape.proof_bytes() and proof.sum_canonical == s, r
        assert proof.bytes == want, r
        assert K.unmont(proof.point) == point and K.unmont(proof.finals) == finals, r
    res, vpoint, vfinals = prodcheck.verify(shape.statement(), got[0][0].bytes, tau_m, bind_m, K.mont([s]))
    assert res.accepted and res.check == "NONE" and res.offset == len(want), res
    assert np.array_equal(vpoint, got[0][0].point) and np.array_equal(vfinals, got[0][0].finals)


def field_sum(parts):
    """[ranks][D + 1, 4] Montgomery -> the D + 1 field sums, canonical"""
    return [sum(col) % P for col in zip(*(K.unmont(h) for h in parts))]


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("name", ["r1cs", "triple", "four"])
def test_the_ranks_slices_add_up_to_the_lone_round_and_store_its_fold_compacted(ctx, name, G):
    """pkss_round_shard on one lone context at a round length of 2^(c+g+1) -- the shortest sharded round: one chunk pair per rank --
    and twice that, without and with a fold, with tau where the shape has one: over the ranks the slices' field sum is pks_round's
    values on the same tables, on grids 1, 2, 7, 300 and the library's, and each rank's output tables are the compaction of the lone
    fold's output"""
    from provekit_amd import prodcheck, prodcheck_sharded
    from provekit_amd.field import random_field

    base = K.Shape(name, 28)
    hand = prodcheck_sharded.plan(base.statement(), G).handover_len
    g = R.log2(G)
    for round_len in (hand, 2 * hand):
        for fold in (False, True):
            N = 2 * round_len if fold else round_len
            n = N.bit_length() - 1
            shape = K.Shape(name, n)
            stmt = shape.statement()
            full = [random_field(N, 7 * j + n) for j in range(shape.m)]
            d = [ctx.upload(t) for t in full]
            coords = (round_len // 2).bit_length() - 1  # the coordinates after the round's own
            tau_rest = random_field(coords, 5) if shape.has_tau else None
            alpha = random_field(1, 9) if fold else None
            lone_out = [ctx.alloc_fe(N // 2) for _ in range(shape.m)] if fold else None
            want = prodcheck.round(ctx, stmt, d, N, tau_rest, alpha, lone_out)
            folded = [ctx.download_fe(o.ptr, N // 2) for o in lone_out] if fold else None
            local = [ctx.alloc_fe(N // 2 // G) for _ in range(shape.m)] if fold else None
            for grid in (0, 1, 2, 7, 300):
                parts = []
                for r in range(G):
                    parts.append(prodcheck_sharded.round_shard(ctx, stmt, d, N, G, r, tau_rest, alpha, local, grid))
                    if fold:
                        for j in range(shape.m):
                            got = ctx.download_fe(local[j].ptr, N // 2 // G)
                            idx = np.array([R.expand(y, g, r) for y in range(N // 2 // G)])
                            assert np.array_equal(got, folded[j][idx]), (round_len, grid, r, j)
                            ctx.zero(local[j].ptr, 32 * (N // 2 // G))
                assert field_sum(parts) == K.unmont(want), (round_len, fold, grid)
            for b in d + (lone_out or []) + (local or []):
                b.free()


def test_a_round_too_short_to_be_sharded_and_a_rank_outside_the_world_are_refused(ctx):
    from provekit_amd import prodcheck_sharded
    from provekit_amd._lib import ProveKitHipError

    shape = K.Shape("inner", 12)
    hand = prodcheck_sharded.plan(shape.statement(), 2).handover_len
    d = [ctx.alloc_fe(1 << 12) for _ in range(2)]
    with pytest.raises(ProveKitHipError, match="not sharded"):
        prodcheck_sharded.round_shard(ctx, shape.statement(), d, hand // 2, 2, 0)
    with pytest.raises(ProveKitHipError, match="not sharded"):  # with a fold the round is half the tables
        prodcheck_sharded.round_shard(ctx, shape.statement(), d, hand, 2, 0, fold=K.mont([5]), d_out_local=d)
    with pytest.raises(ProveKitHipError, match="rank must be below world"):
        prodcheck_sharded.round_shard(ctx, shape.statement(), d, hand, 2, 2)
    with pytest.raises(ProveKitHipError, match="power of two"):
        prodcheck_sharded.round_shard(ctx, shape.statement(), d, hand, 3, 0)
    for b in d:
        b.free()


def check_against(ctxs, shape, tables, tau, bind=()):
    want, point, finals, s = K.prove(shape, tables, tau, bind)
    got = prove_on_ranks(ctxs, shape.statement(), [K.mont(t) for t in tables], K.mont(tau) if tau is not None else None, None)
    for (proof,) in got:
        assert proof.bytes == want and K.unmont(proof.point) == point and K.unmont(proof.finals) == finals and proof.sum_canonical == s
    return s


@pytest.mark.parametrize("name", ["inner", "r1cs", "four"])
def test_edge_values_all_zero_and_all_p_minus_one(rank_sets, name):
    n = smallest_n(2, 3)  # a hand-over and an in-place sharded round
    shape = K.Shape(name, n)
    ctxs = rank_sets(2)
    tau = K.random_elements(n, seed=1) if shape.has_tau else None
    assert check_against(ctxs, shape, [[0] * (1 << n)] * shape.m, tau) == 0
    check_against(ctxs, shape, [[P - 1] * (1 << n)] * shape.m, [P - 1] * n if shape.has_tau else None)


@pytest.mark.parametrize("name", ["r1cs", "mixed"])
def test_edge_values_tau_with_coordinates_0_1_and_p_minus_one(rank_sets, name):
    n = smallest_n(4, 3)
    shape = K.Shape(name, n)
    tables = K.random_tables(shape.m, n, seed=5)
    ctxs = rank_sets(4)
    for tau in (([0, 1, P - 1] * n)[:n], [1] * n, [0] * n, ([P - 1, 0, 0, 1, 1, P - 1, 5, 0, 1] * 2)[:n]):
        check_against(ctxs, shape, tables, tau)


def test_the_callers_tables_are_unchanged_and_a_prover_proves_again_the_same(rank_sets):
    from provekit_amd import prodcheck_sharded

    G = 4
    n = smallest_n(G, 3)
    shape, tables, tau, bind, want, _, _, _ = reference("r1cs", n)
    tabs, tau_m, bind_m = images("r1cs", n)

    def fn(r, c):
        d = [c.upload(t) for t in tabs]
        prover = prodcheck_sharded.Prover(c, shape.statement())
        first = prover.prove(d, tau_m, bind_m)
        same = all(np.array_equal(c.download_fe(b.ptr, 1 << n).reshape(-1, 4), t) for t, b in zip(tabs, d))
        second = prover.prove(d, tau_m, bind_m)
        profile = prover.plan, prover.last_profile()
        prover.close()
        for b in d:
            b.free()
        return first, second, same, profile

    for first, second, same, (plan, profile) in run_ranks(rank_sets(G), fn):
        assert same and first.bytes == second.bytes == want
        assert np.array_equal(first.point, second.point) and np.array_equal(first.finals, second.finals)
        # what each round's launch covered on this rank: 1 / G of the round's pairs while it is sharded, all of them after
        assert [(r["sharded"], r["pairs"]) for r in profile["rounds"]] == [(i < plan.S, (1 << (n - 1 - i)) >> (plan.g if i < plan.S else 0)) for i in range(n)]
        assert profile["total_s"] > 0 and profile["handover_s"] > 0 and all(r["exchange_s"] > 0 for r in profile["rounds"][: plan.S])


def test_a_short_proof_buffer_is_refused_on_every_rank_and_the_prover_stays_usable(rank_sets):
    from provekit_amd import prodcheck_sharded
    from provekit_amd._lib import ProveKitHipError

    G = 2
    n = smallest_n(G, 2)
    shape, tables, tau, bind, want, _, _, _ = reference("mixed", n)
    tabs, tau_m, bind_m = images("mixed", n)

    def fn(r, c):
        d = [c.upload(t) for t in tabs]
        prover = prodcheck_sharded.Prover(c, shape.statement())
        short = [(refusal(lambda: prover.prove(d, tau_m, bind_m, capacity=cap)), prover.last_len) for cap in (0, len(want) - 1)]
        out = short, prover.prove(d, tau_m, bind_m).bytes, prover.prove(d, tau_m, bind_m, capacity=len(want) + 100).bytes
        prover.close()
        for b in d:
            b.free()
        return out

    for short, exact, roomy in run_ranks(rank_sets(G), fn):
        for (code, message), last_len in short:  # every rank with its own reason, not with "rank 0 failed"
            assert code == -1 and "proof buffer" in message and last_len == len(want)
        assert exact == roomy == want


@pytest.mark.parametrize("what", ["tau", "bind"])
def test_ranks_that_disagree_on_tau_or_bind_all_refuse_and_then_prove(rank_sets, what):
    from provekit_amd import prodcheck_sharded
    from provekit_amd._lib import ProveKitHipError

    G = 2
    n = smallest_n(G, 2)
    shape, tables, tau, bind, want, _, _, _ = reference("r1cs", n)
    tabs, tau_m, bind_m = images("r1cs", n)
    other_tau, other_bind = tau_m.copy(), bind_m.copy()
    other_tau[n - 1, 0] ^= 1  # the last coordinate, on rank 1 alone: it enters the weights of the last round only
    other_bind[0, 0] ^= 1

    def fn(r, c):
        d = [c.upload(t) for t in tabs]
        prover = prodcheck_sharded.Prover(c, shape.statement())
        no = refusal(lambda: prover.prove(d, other_tau if r == 1 and what == "tau" else tau_m, other_bind if r == 1 and what == "bind" else bind_m))
        out = no, prover.prove(d, tau_m, bind_m).bytes
        prover.close()
        for b in d:
            b.free()
        return out

    for (code, message), proof in run_ranks(rank_sets(G), fn):
        assert code == -1 and "ranks disagree on bind, tau or the coefficients: rank 1" in message
        assert proof == want


def test_creation_is_refused_outside_a_set_and_when_the_ranks_statements_differ(ctx, rank_sets):
    from provekit_amd import prodcheck, prodcheck_sharded
    from provekit_amd._lib import ProveKitHipError

    stmt = K.Shape("r1cs", 11, n_bind=1).statement()
    with pytest.raises(ProveKitHipError, match="not in a device set") as e:
        prodcheck_sharded.Prover(ctx, stmt)
    assert e.value.code == -1

    def differ(r, c):
        other = refusal(lambda: prodcheck_sharded.Prover(c, K.Shape("r1cs", 11, n_bind=2 if r == 1 else 1).statement()))
        # one rank's statement is refused: every rank leaves with its status
        bad = refusal(lambda: prodcheck_sharded.Prover(c, prodcheck.Statement(11, 3, [(1, 0b011)]) if r == 1 else stmt))
        # each kind of prover proves through its own call
        sharded, lone = prodcheck_sharded.Prover(c, stmt), prodcheck.Prover(c, stmt)
        d = [c.alloc_fe(1 << 11) for _ in range(3)]
        tau, bind = K.mont([1] * 11), K.mont([1])
        wrong = refusal(lambda: prodcheck.Prover.prove(sharded, d, tau, bind))
        lone.handle, sharded.handle = sharded.handle, lone.handle
        wrong_too = refusal(lambda: prodcheck_sharded.Prover.prove(sharded, d, tau, bind))
        lone.handle, sharded.handle = sharded.handle, lone.handle
        sharded.close()
        lone.close()
        for b in d:
            b.free()
        return other, bad, wrong, wrong_too

    for r, (other, bad, wrong, wrong_too) in enumerate(run_ranks(rank_sets(2), differ)):
        assert other[0] == -1 and "ranks disagree on the statement: rank 1" in other[1]
        assert bad[0] == -1 and ("used by no term" if r == 1 else "rank 1 of the device set failed") in bad[1]
        assert wrong[0] == -1 and "proves with pkss_prove" in wrong[1]
        assert wrong_too[0] == -1 and "proves with pks_prove" in wrong_too[1]


def test_composition_on_a_set_sharded_commit_sumcheck_and_opening(rank_sets):
    """every rank: commit a, b, c with the set's sharded scheme, prove eq (a b - c) = s with the root bound, open the commitment at the
    sumcheck's point.  All ranks' root, proof and opening are equal, and both host verifiers accept"""
    import whir_pcs_config_cases as CC
    from provekit_amd import prodcheck, prodcheck_sharded, whir_pcs
    from provekit_amd.field import random_field

    G = 2
    n = smallest_n(G, 3)
    shape = K.Shape("r1cs", n, n_bind=1)
    tabs = [random_field(1 << n, seed) for seed in (21, 22, 23)]
    tau = random_field(n, 24)
    cfg = CC.config(n, 2, 1, 3)

    def fn(r, c):
        d = [c.upload(t) for t in tabs]
        scheme = whir_pcs.Scheme(c, cfg)
        com = scheme.commit(d)
        root = com.root()
        bind = K.mont([int.from_bytes(root, "little")])
        prover = prodcheck_sharded.Prover(c, shape.statement())
        proof = prover.prove(d, tau, bind)
        evals, opening = scheme.open(com, proof.point[None])
        assert np.array_equal(evals.reshape(-1, 4), proof.finals)
        for x in (prover, com, scheme):
            x.close()
        for b in d:
            b.free()
        return root, proof.bytes, opening

    got = run_ranks(rank_sets(G), fn)
    assert all(g == got[0] for g in got)
    root, proof, opening = got[0]
    bind = K.mont([int.from_bytes(root, "little")])
    res, point, finals = prodcheck.verify(shape.statement(), proof, tau, bind)
    assert res.accepted and res.check == "NONE", res
    wres, wevals = whir_pcs.verify(cfg, point[None], opening, expected_root=root)
    assert wres.accepted, wres
    assert np.array_equal(wevals.reshape(-1, 4), finals)


def test_the_cpp_demo_commits_proves_and_opens_on_a_set_and_verifies_once():
    import subprocess

    demo = os.path.join(ROOT, "examples", "sumcheck_sharded_demo")
    assert os.path.exists(demo), "examples/sumcheck_sharded_demo is built by __graft_entry__.build()"
    n, G = smallest_n(2, 3), 2
    out = subprocess.run(["timeout", "-k", "10", "120", demo, str(n), str(G), "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("ok n_vars=%d ranks=%d sharded_rounds=3 " % (n, G)) and "sumcheck_bytes=%d " % (32 * (1 + n * 3 + 3)) in out.stdout
    assert out.stdout.rstrip().endswith("one root, one sumcheck, one opening, accepted")
