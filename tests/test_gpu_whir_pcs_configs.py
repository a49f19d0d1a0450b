"""GPU: pkw_commit / pkw_open / pkw_open_linear / pkw_open_sparse over the grid of whir_pcs_config_cases.py -- every fold, rate, batch,
round count, final polynomial size, OOD count and grinding position the library accepts, and more than 32 weights in one
combination -- byte for byte against the transcript the oracle prover's parts write (the proofs test_whir_pcs_configs_host.py
verifies on the CPU).  Every comparison is of bytes or of field elements.  A mismatch is reported with its first differing offset
and the region of the proof it lies in."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_config_cases as G  # noqa: E402
import whir_pcs_linear_cases as L  # noqa: E402
import whir_pcs_sparse_cases as S  # noqa: E402

PK_ERR_OOM = -2
ids = lambda e: e.id if isinstance(e, G.Entry) else None  # noqa: E731


def ints(oracle, limbs):
    return oracle.limbs_to_ints(oracle.from_mont(np.ascontiguousarray(limbs).reshape(-1, 4)))


def opened(call, what):
    """call(), with PK_ERR_OOM named for what it is: plan() (csrc/whir_pcs/pcs.hpp) sized the arena below what the opening takes"""
    from provekit_amd._lib import ProveKitHipError

    try:
        return call()
    except ProveKitHipError as e:
        if e.code == PK_ERR_OOM:
            pytest.fail(f"{what}: plan() and the opening's buffers disagree ({e})")
        raise


class Device:
    """a scheme, the polynomials on the device and their commitment"""

    def __init__(self, ctx, oracle, cfg, polys):
        from provekit_amd import whir_pcs

        self.scheme = whir_pcs.Scheme(ctx, cfg)
        self.bufs = [ctx.upload(L.mont(oracle, p)) for p in polys]
        self.com = self.scheme.commit(self.bufs)

    def close(self):
        for x in self.bufs:
            x.free()
        self.com.close()
        self.scheme.close()


def check_opening(ctx, oracle, o):
    """the assertions of test_open_writes_the_oracles_transcript_byte_for_byte on one oracle opening `o`"""
    from provekit_amd import whir_pcs

    ctx.set_hash_version(o.hash_version)
    try:
        d = Device(ctx, oracle, o.cfg, o.polys)
        assert d.com.root() == o.root
        evals, proof = opened(lambda: d.scheme.open(d.com, o.mpts), o.entry.id)
        again = opened(lambda: d.scheme.open(d.com, o.mpts), o.entry.id)[1]
    finally:
        ctx.set_hash_version(2)
    assert ints(oracle, evals) == [v for row in o.vals for v in row]
    assert len(proof) == len(o.proof) and proof == o.proof, G.first_difference(proof, o.proof, o.cfg, o.q)
    r, bound = whir_pcs.verify(o.cfg, o.mpts, proof, expected_root=o.root, hash_version=o.hash_version)
    assert r.accepted and r.offset == len(proof) and np.array_equal(bound, evals), r
    assert again == proof, G.first_difference(again, proof, o.cfg, o.q)
    d.close()


@pytest.mark.parametrize("entry", G.FOLD_EDGES + G.MIXED + G.SINGLE_GRIND, ids=ids)
def test_open_writes_the_oracles_transcript_at_every_config(ctx, oracle, entry):
    check_opening(ctx, oracle, G.opening(oracle, entry))


@pytest.mark.parametrize("entry", G.HASH_V1, ids=ids)
def test_open_writes_the_oracles_transcript_under_hash_version_1(ctx, oracle, entry):
    o = G.opening(oracle, entry, hash_version=1)
    assert o.root != G.opening(oracle, entry).root
    check_opening(ctx, oracle, o)


@pytest.mark.parametrize("entry,weights", G.INITIAL_WEIGHTS, ids=ids)
def test_open_with_an_initial_combination_of_32_33_and_68_weights(ctx, oracle, entry, weights):
    """the points and the commitment's OOD samples go to pk_eq_accumulate 32 at a time: one full chunk, a second chunk of one, and
    (64 points, 4 samples) a third"""
    o = G.opening(oracle, entry)
    assert o.cfg.commitment_ood_samples + o.q == weights  # the count the name promises, before anything is compared
    check_opening(ctx, oracle, o)


@pytest.mark.parametrize("entry,distinct", G.ROUND_WEIGHTS, ids=ids)
def test_open_with_a_rounds_combination_of_31_to_34_weights(ctx, oracle, entry, distinct):
    """one OOD sample and 30..33 distinct STIR indexes in round 0, as the oracle's transcript draws them"""
    o = G.opening(oracle, entry)
    assert o.counts[0] == (o.cfg.num_queries[0], distinct, 64) and o.cfg.ood_samples[0] == 1
    check_opening(ctx, oracle, o)


def test_open_with_every_row_of_the_initial_tree_opened(ctx, oracle):
    o = G.opening(oracle, G.ALL_ROWS)
    assert o.counts[0] == (400, 32, 32)
    check_opening(ctx, oracle, o)


@pytest.mark.parametrize("q,l", G.LINEAR_COUNTS)
@pytest.mark.parametrize("entry", G.LINEAR, ids=ids)
def test_open_linear_and_open_sparse_write_the_oracles_transcript(ctx, oracle, entry, q, l):
    """pkw_open_linear against the oracle's opening of the dense statement; pkw_open_sparse against pkw_open_linear's bytes on the
    densified tables"""
    from provekit_amd import whir_pcs

    o = G.linear_opening(oracle, entry, q, l)
    d = Device(ctx, oracle, o.cfg, o.polys)
    assert d.com.root() == o.root
    d_w = [ctx.upload(w) for w in o.mdense]
    sw = S.pack(oracle, o.ws).upload(ctx)
    evals, sums, proof = opened(lambda: d.scheme.open_linear(d.com, o.mpts, d_w, o.mtags), entry.id)
    assert sums.shape == (o.batch, l, 4) and ints(oracle, sums) == [s for row in o.sums for s in row]
    assert evals.shape == (o.batch, q, 4) and (not q or ints(oracle, evals) == [v for row in o.vals for v in row])
    assert len(proof) == len(o.proof) and proof == o.proof, G.first_difference(proof, o.proof, o.cfg, q, l)
    v = whir_pcs.verify_linear(o.cfg, o.mpts, o.mtags, o.mdense, proof, expected_root=o.root)
    assert v.result.accepted and v.unchecked == 0 and v.result.offset == len(proof), v.result
    s_evals, s_sums, s_proof = opened(lambda: d.scheme.open_sparse(d.com, o.mpts, sw, o.mtags), entry.id)
    assert np.array_equal(s_evals, evals) and np.array_equal(s_sums, sums)
    assert len(s_proof) == len(proof) and s_proof == proof, G.first_difference(s_proof, proof, o.cfg, q, l)
    v = whir_pcs.verify_sparse(o.cfg, o.mpts, o.mtags, sw, s_proof, expected_root=o.root)
    assert v.result.accepted and v.result.offset == len(s_proof), v.result
    assert d.scheme.open_linear(d.com, o.mpts, d_w, o.mtags)[2] == proof  # either order over the same arena
    for x in d_w + [sw]:
        x.free()
    d.close()


def test_one_scheme_opens_two_commitments_alternately(ctx, oracle):
    """the arena is reused from the front: an opening gives the bytes it gave alone, whatever the previous one left there"""
    from provekit_amd import whir_pcs

    entry = G.Entry(9, 4, 2, 3, ood=4, commitment_ood=4)
    first = G.opening(oracle, entry)
    cfg, pts = first.cfg, first.mpts
    other_polys = K.polynomials(entry.n, entry.batch, seed=41)
    assert other_polys != first.polys
    other, other_root, _ = K.oracle_opening(oracle, cfg, other_polys, first.pts, first.pattern)
    d = Device(ctx, oracle, cfg, first.polys)
    bufs = [ctx.upload(L.mont(oracle, p)) for p in other_polys]
    com2 = d.scheme.commit(bufs)
    assert d.com.root() == first.root and com2.root() == other_root != first.root
    alone = [d.scheme.open(d.com, pts)[1], d.scheme.open(d.com, pts)[1]]
    assert alone[0] == alone[1] == first.proof, G.first_difference(alone[0], first.proof, cfg, first.q)
    for _ in range(2):
        got2 = opened(lambda: d.scheme.open(com2, pts), entry.id)[1]
        assert got2 == other, G.first_difference(got2, other, cfg, first.q)
        got1 = opened(lambda: d.scheme.open(d.com, pts), entry.id)[1]
        assert got1 == first.proof, G.first_difference(got1, first.proof, cfg, first.q)
    assert whir_pcs.verify(cfg, pts, got2, expected_root=other_root)[0].accepted
    r, _ = whir_pcs.verify(cfg, pts, got2, expected_root=first.root)
    assert not r.accepted and r.check == "ROOT"
    for x in bufs:
        x.free()
    com2.close()
    d.close()


RUNNABLE = [(what, accepted) for what, _, accepted, runnable in G.BOUNDS if runnable]


@pytest.mark.parametrize("what,accepted", RUNNABLE, ids=[w for w, _ in RUNNABLE])
def test_the_accepted_neighbours_of_the_bounds_open_and_verify(ctx, oracle, what, accepted):
    check_opening(ctx, oracle, G.opening(oracle, G.Entry(*accepted[0], **accepted[1])))
