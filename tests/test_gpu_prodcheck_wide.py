"""GPU: the wide product sumcheck on the device (include/provekit_sumcheck_wide.h, csrc/sumcheck/wide.hip).  pksw_round against the
Python reference's round (tests/prodcheck_wide_refs.py) for every catalogue entry over pair counts, grids, folds in and out of place,
weights and edge tables; the cross-check against the existing kernel -- pksw_round's values equal pks_round's bit for bit on the twelve
statements both interfaces state; pksw_prove's bytes against the reference prover's; point and finals returned, the caller's tables
untouched, a prover reused; a false Plonk gate; the C++ demo.  All comparisons are exact.

A weighted round's length is a power of two (the split eq weights are tables over the bits of the pair index), so the weighted
rounds run at 1, 2, 256 and 1024 pairs; the unweighted ones run at 3, 255 and 257 pairs too -- a pair count that is no power of two,
a last workgroup one lane short, and one lane into the next -- which pksw_round takes where it has no weight to index."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prodcheck_refs as K  # noqa: E402
import prodcheck_wide_refs as W  # noqa: E402

pytestmark = pytest.mark.gpu
P = W.P
EVERY = list(W.CATALOGUE)
MAX_GRID = 1024
PAIRS = [1, 2, 3, 255, 256, 257, 1024]
GRIDS = [1, 2, 3, 7, MAX_GRID, 0]
PROOF_SIZES = [1, 2, 8, 9, 10, 12]
WHOLE_PROOFS = ["plonk", "pow5", "wide16"] + W.ONE_PER_DEGREE


def upload(ctx, tables):
    return [ctx.upload(W.mont(t)) for t in tables]


def free(bufs):
    for b in bufs:
        b.free()


def fe_bytes(values):
    return W.mont(values).tobytes()


def check_rounds(ctx, shape, tables, pairs, tau_rest, r, grids):
    """pksw_round of `pairs` pairs against round_values on every grid: without a fold on the first 2 * pairs entries of `tables`, with
    the fold by r on all 4 * pairs of them, out of place and in place"""
    from provekit_amd import prodcheck_wide

    stmt = shape.statement()
    short = [t[: 2 * pairs] for t in tables]
    want = fe_bytes(W.round_values(shape, short, tau_rest))
    want_folded, folded = W.round_values(shape, tables, tau_rest, fold=r)
    want_folded, folded = fe_bytes(want_folded), b"".join(fe_bytes(t) for t in folded)
    tau_a = W.mont(tau_rest) if tau_rest is not None else None
    d_short, d_long = upload(ctx, short), upload(ctx, tables)
    outs = [ctx.alloc_fe(2 * pairs) for _ in range(shape.m)]
    try:
        for grid in grids:
            assert prodcheck_wide.round(ctx, stmt, d_short, 2 * pairs, tau_a, grid=grid).tobytes() == want, ("no fold", grid)
            h = prodcheck_wide.round(ctx, stmt, d_long, 4 * pairs, tau_a, W.mont([r]), outs, grid)
            assert h.tobytes() == want_folded, ("fold", grid)
            assert b"".join(ctx.download_fe(o.ptr, 2 * pairs).tobytes() for o in outs) == folded, ("folded tables", grid)
            for o in outs:
                ctx.zero(o.ptr, 32 * 2 * pairs)
        # the caller's tables were inputs only
        assert b"".join(ctx.download_fe(b.ptr, 4 * pairs).tobytes() for b in d_long) == b"".join(fe_bytes(t) for t in tables)
        # in place: the output tables are the input tables, as the prover folds its arena
        for grid in grids:
            scratch = upload(ctx, tables)
            h = prodcheck_wide.round(ctx, stmt, scratch, 4 * pairs, tau_a, W.mont([r]), scratch, grid)
            assert h.tobytes() == want_folded, ("fold in place", grid)
            assert b"".join(ctx.download_fe(b.ptr, 2 * pairs).tobytes() for b in scratch) == folded, ("tables folded in place", grid)
            free(scratch)
    finally:
        free(d_short + d_long + outs)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("name", EVERY)
def test_the_round_of_every_entry_is_the_references_at_every_pair_count_grid_and_fold(ctx, name, weighted):
    shape = W.Shape(name, 12)
    for pairs in PAIRS:
        if weighted and pairs & (pairs - 1):
            continue  # no weight without a power of two; test_a_weighted_round_of_a_length_that_is_no_power_of_two_is_refused
        k = pairs.bit_length() - 1  # coordinates of tau after the round's own variable
        rng = random.Random(1000 * pairs + len(name))
        tables = [[rng.randrange(P) for _ in range(4 * pairs)] for _ in range(shape.m)]
        tau_rest = W.random_elements(k, seed=k + 5) if weighted else None
        r = W.random_elements(1, seed=k + 77)[0]
        check_rounds(ctx, shape, tables, pairs, tau_rest, r, GRIDS)


def test_a_weighted_round_of_a_length_that_is_no_power_of_two_is_refused_and_so_is_an_odd_length(ctx):
    from provekit_amd import prodcheck_wide
    from provekit_amd._lib import ProveKitHipError

    shape = W.Shape("d2t", 12)
    d = upload(ctx, W.random_tables(shape.m, 10, seed=1))
    outs = [ctx.alloc_fe(512) for _ in range(shape.m)]
    tau = W.mont(W.random_elements(8, seed=2))
    with pytest.raises(ProveKitHipError, match="power of two"):
        prodcheck_wide.round(ctx, shape.statement(), d, 6, tau)
    for length, fold in ((7, None), (0, None), (6, W.mont([5])), (1 << 13, None)):
        with pytest.raises(ProveKitHipError, match="len must be"):
            prodcheck_wide.round(ctx, shape.statement(), d, length, None, fold, outs if fold is not None else None)
    free(d + outs)


@pytest.mark.parametrize("name", EVERY)
def test_the_round_of_every_entry_on_tables_of_all_p_minus_one_and_all_zero(ctx, name):
    """every entry of every table p - 1, with every coordinate of tau and the fold challenge p - 1 too; then all 0, whose sums are 0"""
    shape = W.Shape(name, 12)
    for pairs in (2, 256):
        k = pairs.bit_length() - 1
        for v in (P - 1, 0):
            tables = [[v] * (4 * pairs)] * shape.m
            check_rounds(ctx, shape, tables, pairs, [P - 1] * k, P - 1, GRIDS)
            check_rounds(ctx, shape, tables, pairs, None, P - 1, GRIDS)
    for pairs in (3, 257):
        check_rounds(ctx, shape, [[P - 1] * (4 * pairs)] * shape.m, pairs, None, P - 1, GRIDS)
    from provekit_amd import prodcheck_wide

    d = upload(ctx, [[0] * 512] * shape.m)
    assert not prodcheck_wide.round(ctx, shape.statement(), d, 512, W.mont(W.random_elements(8, seed=1))).any()
    free(d)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("wide", list(W.TRANSLATED))
def test_the_wide_round_is_the_product_sumchecks_round_bit_for_bit(ctx, wide, fold):
    """the cross-check against the existing kernel: the twelve statements both interfaces state, the same device tables, with and
    without a fold, weighted as the statement is: pksw_round's D + 1 values are pks_round's, and so are the folded tables"""
    from provekit_amd import prodcheck, prodcheck_wide

    a, b = W.Shape(wide, 12), K.Shape(W.TRANSLATED[wide], 12)
    for length in (4, 1 << 9, 1 << 12):
        pairs = length // 4 if fold else length // 2
        k = pairs.bit_length() - 1
        tables = W.random_tables(a.m, length.bit_length() - 1, seed=length + len(wide))
        tau_rest = W.mont(W.random_elements(k, seed=3)) if a.has_tau else None
        r = W.mont(W.random_elements(1, seed=4)) if fold else None
        d = upload(ctx, tables)
        outs_a = [ctx.alloc_fe(length // 2) for _ in range(a.m)] if fold else None
        outs_b = [ctx.alloc_fe(length // 2) for _ in range(a.m)] if fold else None
        got = prodcheck_wide.round(ctx, a.statement(), d, length, tau_rest, r, outs_a)
        want = prodcheck.round(ctx, b.statement(), d, length, tau_rest, r, outs_b)
        assert got.tobytes() == want.tobytes(), (wide, length)
        if fold:
            for x, y in zip(outs_a, outs_b):
                assert ctx.download_fe(x.ptr, length // 2).tobytes() == ctx.download_fe(y.ptr, length // 2).tobytes()
        free(d + (outs_a or []) + (outs_b or []))


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """computed once per (entry, size) and shared: (shape, tables, tau, bind, proof, point, finals, s)"""
    shape = W.Shape(name, n, n_bind=1)
    tables = W.random_tables(shape.m, n, seed=100 * n + len(name))
    tau = W.random_elements(n, seed=n) if shape.has_tau else None
    bind = W.random_elements(1, seed=3)
    return (shape, tables, tau, bind) + W.prove(shape, tables, tau, bind)


@pytest.mark.parametrize("n", PROOF_SIZES)
@pytest.mark.parametrize("name", WHOLE_PROOFS)
def test_the_provers_bytes_are_the_references_with_point_and_finals_and_are_accepted(ctx, name, n):
    from provekit_amd import prodcheck_wide

    shape, tables, tau, bind, want, point, finals, s = reference(name, n)
    d = upload(ctx, tables)
    prover = prodcheck_wide.Prover(ctx, shape.statement())
    try:
        got = prover.prove(d, W.mont(tau) if tau is not None else None, W.mont(bind))
    finally:
        prover.close()
        free(d)
    assert len(got.bytes) == shape.proof_bytes() and got.sum_canonical == s
    assert got.bytes == want
    assert W.unmont(got.point) == point and W.unmont(got.finals) == finals
    res, vpoint, vfinals = prodcheck_wide.verify(shape.statement(), got.bytes, W.mont(tau) if tau is not None else None, W.mont(bind), W.mont([s]))
    assert res.accepted and res.check == "NONE" and res.offset == len(want), res
    assert np.array_equal(vpoint, got.point) and np.array_equal(vfinals, got.finals)


def test_the_callers_tables_are_unchanged_and_one_prover_proves_twice(ctx):
    """the same prover, two proofs over different tables and then the first again: each the reference's, the tables as uploaded"""
    from provekit_amd import prodcheck_wide

    shape, tables, tau, bind, want, point, finals, _ = reference("plonk", 10)
    other = W.random_tables(shape.m, 10, seed=5)
    want_other = W.prove(shape, other, tau, bind)[0]
    images = [W.mont(t) for t in tables]
    d, d_other = [ctx.upload(im) for im in images], upload(ctx, other)
    prover = prodcheck_wide.Prover(ctx, shape.statement())
    first = prover.prove(d, W.mont(tau), W.mont(bind))
    for im, b in zip(images, d):
        assert np.array_equal(ctx.download_fe(b.ptr, 1 << 10).reshape(-1, 4), im)
    second = prover.prove(d_other, W.mont(tau), W.mont(bind))
    third = prover.prove(d, W.mont(tau), W.mont(bind))
    assert first.bytes == third.bytes == want and second.bytes == want_other and want != want_other
    assert W.unmont(first.point) == point and W.unmont(first.finals) == finals
    assert np.array_equal(first.point, third.point) and np.array_equal(first.finals, third.finals)
    for im, b in zip(images, d):
        assert np.array_equal(ctx.download_fe(b.ptr, 1 << 10).reshape(-1, 4), im)
    prover.close()
    free(d + d_other)


def test_a_short_proof_buffer_is_refused_with_the_length_and_the_prover_stays_usable(ctx):
    from provekit_amd import prodcheck_wide
    from provekit_amd._lib import ProveKitHipError

    shape, tables, tau, bind, want, _, _, _ = reference("d5t", 8)
    d = upload(ctx, tables)
    prover = prodcheck_wide.Prover(ctx, shape.statement())
    for cap in (0, len(want) - 1):
        with pytest.raises(ProveKitHipError, match="proof buffer") as e:
            prover.prove(d, W.mont(tau), W.mont(bind), capacity=cap)
        assert e.value.code == -1 and prover.last_len == len(want)
    assert prover.prove(d, W.mont(tau), W.mont(bind)).bytes == want
    prover.close()
    free(d)


def test_a_false_plonk_gate_is_proved_and_the_expected_sum_0_answers_sum(ctx):
    """a satisfied gate sums to 0 under any tau and is accepted with expected sum 0; with one wire changed the prover proves the sum
    the tables have, pksw_verify accepts that sum and answers PKS_CHECK_SUM to the expected sum 0"""
    from provekit_amd import prodcheck_wide

    n = 8
    shape = W.Shape("plonk", n)
    qL, qR, qM, qO, a, b, c = W.random_tables(7, n, seed=9)
    qC = [-(l * x + r * y + m * x * y + o * z) % P for l, r, m, o, x, y, z in zip(qL, qR, qM, qO, a, b, c)]
    tau = W.random_elements(n, seed=10)
    stmt = shape.statement()
    prover = prodcheck_wide.Prover(ctx, stmt)
    d = upload(ctx, [qL, qR, qM, qO, qC, a, b, c])
    true_gate = prover.prove(d, W.mont(tau))
    assert true_gate.sum_canonical == 0
    res, _, _ = prodcheck_wide.verify(stmt, true_gate.bytes, W.mont(tau), expected_sum=W.mont([0]))
    assert res.accepted, res
    c_bad = list(c)
    c_bad[5] = (c_bad[5] + 1) % P
    d_bad = ctx.upload(W.mont(c_bad))
    false_gate = prover.prove(d[:7] + [d_bad], W.mont(tau))
    want = W.prove(shape, [qL, qR, qM, qO, qC, a, b, c_bad], tau)
    assert false_gate.bytes == want[0] and false_gate.sum_canonical == want[3] != 0
    res, _, _ = prodcheck_wide.verify(stmt, false_gate.bytes, W.mont(tau), expected_sum=W.mont([0]))
    assert not res.accepted and res.check == "SUM" and res.offset == 32, res
    res, _, _ = prodcheck_wide.verify(stmt, false_gate.bytes, W.mont(tau))
    assert res.accepted, res  # for the sum it states, which is not 0
    prover.close()
    free(d + [d_bad])


def test_gate_pcs_demo_exits_0():
    """the C++ face end to end: two WHIR batches of four committed, the gate proved with both roots bound, all eight columns opened at
    the sumcheck's point, both verified, and the error paths"""
    demo = os.path.join(ROOT, "examples", "gate_pcs_demo")
    assert os.path.exists(demo), "examples/gate_pcs_demo is built by __graft_entry__.build()"
    p = subprocess.run([demo, "10", "7"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert lines[0].startswith("ok n_vars=10 sumcheck_bytes=%d " % (32 * (1 + 10 * 4 + 8)))
    assert "check=ROUND" in lines[1] and "check=SUM" in lines[3] and "refused" in lines[4]
