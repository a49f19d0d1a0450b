"""GPU: the round kernel of libprovekit_sumcheck.so (csrc/sumcheck/round.hip) in every form its launch() dispatches -- nine (D, m)
pairs, each with and without a fold, lone and as one rank's slice: 36 kernels -- and with every coefficient kind weighted and not.
The twelve statements of tests/prodcheck_refs.py (SHAPES and FORMS; tests/test_prodcheck_host.py holds them to the dispatch list)
through the public entry points against Python ints, bit for bit: pks_round and pkss_round_shard against K.round_values at the round
lengths where the lanes, the workgroups and the library's grid change, on grids up to PKS_MAX_GRID, at the value edges; whole proofs of
the forms, lone and sharded, against K.prove."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prodcheck_refs as K  # noqa: E402
import prodcheck_shard_refs as R  # noqa: E402
from test_gpu_prodcheck import reference  # noqa: E402  (computed once per (shape, size), shared with the other suites)
from test_gpu_prodcheck_sharded import field_sum, images, prove_on_ranks, rank_sets, torch_first  # noqa: E402, F401  (fixtures too)

pytestmark = pytest.mark.gpu
P = K.P
ONE_PER_PAIR = ["eval", "lin2", "lin3", "lin4", "inner", "r1cs", "mixed", "triple", "four"]  # (1,1) (1,2) (1,3) (1,4) (2,2) (2,3) (2,4) (3,3) (3,4)
# fewer pairs than lanes; one full workgroup of lanes; the library's grid 1 at its largest (two pairs per lane); its grid 2
PAIRS = [1, 2, 4, 256, 512, 1024]
MAX_GRID = 1024


def test_one_shape_per_dispatched_pair():
    assert sorted((K.Shape(name, 1).D, K.Shape(name, 1).m) for name in ONE_PER_PAIR) == [(1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4)]


@functools.lru_cache(maxsize=None)
def tables_of(m, length, seed=0):
    """random canonical tables and their Montgomery images"""
    rng = K.random.Random(1000 * length + 10 * m + seed)
    tables = [[rng.randrange(P) for _ in range(length)] for _ in range(m)]
    return tables, [K.mont(t) for t in tables]


def mont_or_none(values):
    return K.mont(values) if values is not None else None


def check_round(ctx, shape, tables, imgs, tau_rest, alpha, grids):
    """pks_round on `tables` on every grid against K.round_values: without a fold the sums, the tables as they were; with one the sums
    and the folded tables, into separate output tables (the input as it was) and in place on a fresh copy (the upper half as it was)"""
    from provekit_amd import prodcheck

    stmt, m, N = shape.statement(), shape.m, len(tables[0])
    tau_m, alpha_m = mont_or_none(tau_rest), mont_or_none([alpha] if alpha is not None else None)
    d = [ctx.upload(im) for im in imgs]
    try:
        if alpha is None:
            want = K.round_values(shape, tables, tau_rest)
            for grid in grids:
                assert K.unmont(prodcheck.round(ctx, stmt, d, N, tau_m, None, None, grid)) == want, (N, grid)
        else:
            want, folded = K.round_values(shape, tables, tau_rest, alpha)
            folded_m = [K.mont(t) for t in folded]
            outs = [ctx.alloc_fe(N // 2) for _ in range(m)]
            inplace = [ctx.alloc_fe(N) for _ in range(m)]
            try:
                for grid in grids:
                    for o in outs:
                        ctx.zero(o.ptr, 32 * (N // 2))
                    assert K.unmont(prodcheck.round(ctx, stmt, d, N, tau_m, alpha_m, outs, grid)) == want, (N, grid)
                    for j in range(m):
                        assert np.array_equal(ctx.download_fe(outs[j].ptr, N // 2), folded_m[j]), (N, grid, j)
                    for j in range(m):
                        ctx.upload_into(inplace[j].ptr, imgs[j])
                    assert K.unmont(prodcheck.round(ctx, stmt, inplace, N, tau_m, alpha_m, inplace, grid)) == want, (N, grid, "in place")
                    for j in range(m):
                        got = ctx.download_fe(inplace[j].ptr, N)
                        assert np.array_equal(got[: N // 2], folded_m[j]) and np.array_equal(got[N // 2 :], imgs[j][N // 2 :]), (N, grid, j, "in place")
            finally:
                for b in outs + inplace:
                    b.free()
        for j in range(m):  # the input is only ever read
            assert np.array_equal(ctx.download_fe(d[j].ptr, N), imgs[j]), (N, j)
    finally:
        for b in d:
            b.free()
    return want


# ---- a. every lone instantiation through pks_round ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True], ids=["asis", "fold"])
@pytest.mark.parametrize("name", ONE_PER_PAIR + ["lin2rep", "deg3low", "pair2"])
def test_the_lone_round_of_every_form_is_the_references_at_every_length_and_grid(ctx, name, fold):
    """round_kernel<D, m, fold> of the shape's (D, m): pairs 1 .. 1024, tau_rest given and NULL whatever the shape's has_tau, the
    library's grid, 1 and 3, and at 1024 pairs PKS_MAX_GRID = 1024 workgroups: all but four idle, their partials zero, and the finish
    kernel's lanes take four partials each"""
    for pairs in PAIRS:
        N = (4 if fold else 2) * pairs
        shape = K.Shape(name, N.bit_length() - 1)
        tables, imgs = tables_of(shape.m, N)
        coords = pairs.bit_length() - 1
        alpha = K.random_elements(1, seed=pairs)[0] if fold else None
        grids = (0, 1, 3) + ((MAX_GRID,) if pairs == 1024 else ())
        for tau_rest in (K.random_elements(coords, seed=60 + coords), None):
            check_round(ctx, shape, tables, imgs, tau_rest, alpha, grids)


# ---- b. values at the edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_PER_PAIR)
def test_the_lone_round_at_the_value_edges(ctx, name):
    """256 pairs: all tables p - 1; 0 and p - 1 by halves (and, under a fold, by quarters: the halves of the folded tables), the other
    way round in every second table, so every hi - lo is +-(p - 1); all zero, whose sums are zero; fold challenges 0, 1, p - 1; tau_rest
    with coordinates of {0, 1, p - 1}"""
    pairs = 256
    for alpha in (None, 0, 1, P - 1):
        N = (2 if alpha is None else 4) * pairs
        shape = K.Shape(name, N.bit_length() - 1)
        m = shape.m

        def by(parts):  # table j: `parts` runs of 0 and p - 1 in turn, beginning with p - 1 in the odd tables
            run = N // parts
            return [[(P - 1) * ((x // run + j) % 2) for x in range(N)] for j in range(m)]

        sets = {"p-1": [[P - 1] * N] * m, "halves": by(2), "zero": [[0] * N] * m}
        if alpha is not None:
            sets["quarters"] = by(4)
        for what, tables in sets.items():
            imgs = [K.mont(t) for t in tables]
            for tau_rest in (None, [0, 1, P - 1, 1, P - 1, 0, P - 1, 1], [P - 1] * 8, [1, 0, 0, 1, 1, 0, 1, 0]):
                h = check_round(ctx, shape, tables, imgs, tau_rest, alpha, (0,))  # the reference's sums, which the device's equal
                assert what != "zero" or h == [0] * (shape.D + 1)


# ---- c. grid bounds ---------------------------------------------------------------------------------------------------------------------
def test_grid_1024_is_taken_and_1025_refused_with_its_reason_and_the_context_stays_usable(ctx):
    from provekit_amd import prodcheck, prodcheck_sharded
    from provekit_amd._lib import ProveKitHipError

    shape = K.Shape("lin2", 11)
    tables, imgs = tables_of(2, 1 << 11)
    tau_rest = K.random_elements(10, seed=3)
    want = K.round_values(shape, tables, tau_rest)
    d = [ctx.upload(im) for im in imgs]
    stmt = shape.statement()
    assert prodcheck.MAX_GRID == MAX_GRID
    assert K.unmont(prodcheck.round(ctx, stmt, d, 1 << 11, K.mont(tau_rest), grid=MAX_GRID)) == want
    for call in (lambda: prodcheck.round(ctx, stmt, d, 1 << 11, K.mont(tau_rest), grid=MAX_GRID + 1),
                 lambda: prodcheck_sharded.round_shard(ctx, stmt, d, 1 << 11, 2, 0, K.mont(tau_rest), grid=MAX_GRID + 1)):
        with pytest.raises(ProveKitHipError, match=r"grid must be 0\.\.1024") as e:
            call()
        assert e.value.code == -1  # PK_ERR_BAD_ARG
    assert K.unmont(prodcheck.round(ctx, stmt, d, 1 << 11, K.mont(tau_rest))) == want
    parts = [prodcheck_sharded.round_shard(ctx, stmt, d, 1 << 11, 2, r, K.mont(tau_rest), grid=MAX_GRID) for r in range(2)]
    assert field_sum(parts) == want
    for b in d:
        b.free()


# ---- d. every sharded instantiation through pkss_round_shard on one lone context -----------------------------------------------------
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", ["lin2", "lin3", "lin4", "deg3low", "pair2"])
def test_the_ranks_slices_of_every_form_add_up_to_the_references_round_and_store_its_fold_compacted(ctx, name, G):
    """round_kernel_sharded<D, m, fold> at the shortest sharded round length 2^(c+g+1) and twice that, without and with a fold, tau_rest
    as the shape says (lin3, lin4: the other way too), grids 0, 1, 7: the field sum of the ranks' slices is K.round_values' on the same
    tables, and each rank's output tables are the expand()-compaction of its folded tables"""
    from provekit_amd import prodcheck_sharded

    g = R.log2(G)
    hand = prodcheck_sharded.plan(K.Shape(name, 28).statement(), G).handover_len
    assert hand == 1 << (R.C + g + 1)
    for round_len in (hand, 2 * hand):
        for fold in (False, True):
            N = 2 * round_len if fold else round_len
            shape = K.Shape(name, N.bit_length() - 1)
            stmt, m = shape.statement(), shape.m
            tables, imgs = tables_of(m, N)
            d = [ctx.upload(im) for im in imgs]
            coords = (round_len // 2).bit_length() - 1
            alpha = K.random_elements(1, seed=9)[0] if fold else None
            local_len = N // 2 // G
            local = [ctx.alloc_fe(local_len) for _ in range(m)] if fold else None
            idx = [np.array([R.expand(y, g, r) for y in range(local_len)]) for r in range(G)]
            for weighted in ((shape.has_tau, not shape.has_tau) if name in ("lin3", "lin4") else (shape.has_tau,)):
                tau_rest = K.random_elements(coords, seed=5) if weighted else None
                want = K.round_values(shape, tables, tau_rest, alpha)
                if fold:
                    want, folded = want
                    folded_m = [K.mont(t) for t in folded]
                for grid in (0, 1, 7):
                    parts = []
                    for r in range(G):
                        parts.append(prodcheck_sharded.round_shard(ctx, stmt, d, N, G, r, mont_or_none(tau_rest), mont_or_none([alpha] if fold else None), local, grid))
                        if fold:
                            for j in range(m):
                                assert np.array_equal(ctx.download_fe(local[j].ptr, local_len), folded_m[j][idx[r]]), (round_len, grid, r, j)
                                ctx.zero(local[j].ptr, 32 * local_len)
                    assert field_sum(parts) == want, (round_len, fold, weighted, grid)
            for j in range(m):
                assert np.array_equal(ctx.download_fe(d[j].ptr, N), imgs[j])
            for b in d + (local or []):
                b.free()


# ---- e. whole proofs, lone -------------------------------------------------------------------------------------------------------------
# n = 1: the finals come from the caller's tables; 2: the first fold, one pair; 3: the first split eq weights with H = L = 1; 9 .. 11: the
# pair count straddles one workgroup
@pytest.mark.parametrize("n", [1, 2, 3, 9, 10, 11])
@pytest.mark.parametrize("name", list(K.FORMS))
def test_the_provers_bytes_of_the_forms_are_the_references_twice_in_a_row_and_are_accepted(ctx, name, n):
    from provekit_amd import prodcheck

    shape, tables, tau, bind, want, point, finals, s = reference(name, n)
    other = K.random_tables(shape.m, n, seed=77 + n)
    stmt = shape.statement()
    tau_m, bind_m = mont_or_none(tau), K.mont(bind)
    prover = prodcheck.Prover(ctx, stmt)
    try:
        for tabs, ref in ((tables, (want, point, finals, s)), (other, K.prove(shape, other, tau, bind)), (tables, (want, point, finals, s))):
            imgs = [K.mont(t) for t in tabs]
            d = [ctx.upload(im) for im in imgs]
            got = prover.prove(d, tau_m, bind_m)
            assert len(got.bytes) == shape.proof_bytes() and got.bytes == ref[0]
            assert K.unmont(got.point) == ref[1] and K.unmont(got.finals) == ref[2] and got.sum_canonical == ref[3]
            res, vpoint, vfinals = prodcheck.verify(stmt, got.bytes, tau_m, bind_m, K.mont([ref[3]]))
            assert res.accepted and res.check == "NONE" and res.offset == len(ref[0]), res
            assert np.array_equal(vpoint, got.point) and np.array_equal(vfinals, got.finals)
            for im, b in zip(imgs, d):
                assert np.array_equal(ctx.download_fe(b.ptr, 1 << n), im)
                b.free()
    finally:
        prover.close()


# ---- f. whole proofs, sharded ----------------------------------------------------------------------------------------------------------
SHARDED = {(2, 10): 1, (2, 11): 2, (2, 12): 3, (4, 13): 3}  # (G, n) -> S: nothing stored; the first hand-over; the first in-place sharded round


@pytest.mark.parametrize("G,n", list(SHARDED))
@pytest.mark.parametrize("name", ["lin3", "lin4", "deg3low"])
def test_every_ranks_bytes_of_the_forms_are_the_references(rank_sets, name, G, n):
    from provekit_amd import prodcheck, prodcheck_sharded

    shape, tables, tau, bind, want, point, finals, s = reference(name, n)
    assert prodcheck_sharded.plan(shape.statement(), G).S == SHARDED[(G, n)]
    tabs, tau_m, bind_m = images(name, n)
    got = prove_on_ranks(rank_sets(G), shape.statement(), tabs, tau_m, bind_m)
    for r in range(G):
        (proof,) = got[r]
        assert len(proof.bytes) == shape.proof_bytes() and proof.sum_canonical == s, r
        assert proof.bytes == want, r
        assert K.unmont(proof.point) == point and K.unmont(proof.finals) == finals, r
    res, _, _ = prodcheck.verify(shape.statement(), got[0][0].bytes, tau_m, bind_m, K.mont([s]))
    assert res.accepted and res.check == "NONE", res
