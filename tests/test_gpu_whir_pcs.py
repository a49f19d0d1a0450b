"""GPU: libprovekit_whir.so on the device.  pkw_evaluate bit-exact against oracle/verifier.py's mle_eval_table at every size at
which the kernel takes another path; pkw_open's bytes against the transcript the oracle prover's parts write; round trips through
pkw_verify; the refusals; examples/pcs_demo."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
DEMO = os.path.join(ROOT, "examples", "pcs_demo")

import whir_pcs_cases as K  # noqa: E402
from whir_pcs_cases import resolve_n  # noqa: E402

MAX_Q = 9  # 9 points force the second pass over the polynomial


@functools.lru_cache(maxsize=None)
def eval_case(n):
    """two polynomials and nine points per size, and the oracle's evaluations, computed once.  Point 2 repeats point 0."""
    polys = K.polynomials(n, 2, seed=11 + n)
    pts = [K.random_ints(n, 1000 * n + i) for i in range(MAX_Q)]
    for i, special in enumerate((0, 1, K.P - 1)):
        pts[i + 3][(5 * i) % n] = special
        pts[i + 6][n - 1 - (5 * i) % n] = special
    pts[2] = list(pts[0])
    return polys, pts, K.expected_evals(polys, pts)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("q", [1, 3, 8, 9])
@pytest.mark.parametrize("label", ["1", "4", "b-1", "b", "b+1", "13"])
def test_evaluate_is_bit_exact_against_the_oracle(ctx, oracle, label, q, batch):
    from provekit_amd import whir_pcs

    n = resolve_n(label)
    polys, pts, want = eval_case(n)
    bufs = [ctx.upload(oracle.to_mont(oracle.ints_to_limbs(p))) for p in polys[:batch]]
    got = whir_pcs.evaluate(ctx, bufs, n, K.mont_points(oracle, pts[:q]))
    assert got.shape == (batch, q, 4)
    expect = oracle.to_mont(oracle.ints_to_limbs([want[b][i] for b in range(batch) for i in range(q)])).reshape(batch, q, 4)
    assert np.array_equal(got, expect)
    if q >= 3:
        assert np.array_equal(got[:, 0], got[:, 2])  # two equal points
    for b in bufs:
        b.free()


WIDE_BATCH, WIDE_Q = 4, 17  # EVAL_MAX_BATCH polynomials; 17 points are two full passes of eight and a third pass of one


@functools.lru_cache(maxsize=None)
def wide_case(n):
    """eval_case's two polynomials and nine points, two more polynomials and eight more points, and the oracle's evaluations"""
    polys = K.polynomials(n, WIDE_BATCH, seed=11 + n)
    pts = list(eval_case(n)[1]) + [K.random_ints(n, 1000 * n + i) for i in range(MAX_Q, WIDE_Q)]
    pts[16] = list(pts[8])  # the third pass's point repeats the second pass's first
    assert polys[:2] == eval_case(n)[0]
    return polys, pts, K.expected_evals(polys, pts)


def check_wide(ctx, oracle, n, batch, q):
    from provekit_amd import whir_pcs

    polys, pts, want = wide_case(n)
    bufs = [ctx.upload(oracle.to_mont(oracle.ints_to_limbs(p))) for p in polys[:batch]]
    got = whir_pcs.evaluate(ctx, bufs, n, K.mont_points(oracle, pts[:q]))
    assert got.shape == (batch, q, 4)
    expect = oracle.to_mont(oracle.ints_to_limbs([want[b][i] for b in range(batch) for i in range(q)])).reshape(batch, q, 4)
    assert np.array_equal(got, expect)
    assert len({got[b].tobytes() for b in range(batch)}) == batch  # every polynomial its own row
    if q == WIDE_Q:
        assert np.array_equal(got[:, 8], got[:, 16])
    for b in bufs:
        b.free()


@pytest.mark.parametrize("batch", [3, 4])
@pytest.mark.parametrize("q", [3, 9])
@pytest.mark.parametrize("label", ["b-1", "b", "b+1"])
def test_evaluate_with_three_and_four_polynomials(ctx, oracle, label, q, batch):
    check_wide(ctx, oracle, resolve_n(label), batch, q)


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("q", [16, 17])
def test_evaluate_with_a_full_second_and_a_third_pass_over_the_points(ctx, oracle, q, batch):
    check_wide(ctx, oracle, resolve_n("b-1"), batch, q)


@pytest.mark.parametrize("n,tiles", [(17, 1), (18, 2), (20, 8)])
def test_evaluate_with_several_tiles_per_workgroup(ctx, oracle, n, tiles):
    """from 2^18 a workgroup streams more than one tile, four at a time: 2 tiles leave a group half empty, 8 make two groups.
    2^17 is the smallest size with 512 workgroups (one tile each): the nine points are a pass of eight and a pass of ONE, whose
    single output the finish kernel sums from rows of EVAL_PASS = 8 with every lane making a second trip.
    Reference: the C oracle's eq table and dot product (mle_eval_table would take minutes here)."""
    from provekit_amd import whir_pcs
    from provekit_amd.field import random_field

    assert tiles == 1 << (n - whir_pcs.low_vars() - 9)
    polys = [random_field(1 << n, 60 + b) for b in range(2)]
    pts = random_field(MAX_Q * n, n).reshape(MAX_Q, n, 4)
    bufs = [ctx.upload(p) for p in polys]
    got = whir_pcs.evaluate(ctx, bufs, n, pts)
    for i in range(MAX_Q):
        eq = oracle.eq_table(pts[i])
        for b in range(2):
            assert np.array_equal(got[b, i], oracle.dot(eq, polys[b]).reshape(4)), (b, i)
    for b in bufs:
        b.free()


@pytest.mark.parametrize("hash_version", [2, 1])
@pytest.mark.parametrize("shape", K.SHAPES)
def test_open_writes_the_oracles_transcript_byte_for_byte(ctx, oracle, shape, hash_version):
    from provekit_amd import whir_pcs

    n, batch, q = shape
    cfg = K.small_config(n, batch)
    polys, pts = K.polynomials(n, batch), K.points(n, q)
    want, root, vals = K.oracle_opening(oracle, cfg, polys, pts, whir_pcs.io_pattern(cfg, q), hash_version=hash_version)
    ctx.set_hash_version(hash_version)
    try:
        scheme = whir_pcs.Scheme(ctx, cfg)
        com = scheme.commit([ctx.upload(oracle.to_mont(oracle.ints_to_limbs(p))) for p in polys])
        assert com.root() == root
        evals, proof = scheme.open(com, K.mont_points(oracle, pts))
    finally:
        ctx.set_hash_version(2)
    assert oracle.limbs_to_ints(oracle.from_mont(evals.reshape(-1, 4))) == [v for row in vals for v in row]
    assert len(proof) == len(want) and proof == want
    r, _ = whir_pcs.verify(cfg, K.mont_points(oracle, pts), proof, expected_root=root, hash_version=hash_version)
    assert r.accepted, r
    com.close()
    scheme.close()


@pytest.mark.parametrize("n", [12, 16])
def test_round_trip_and_two_openings_of_one_commitment(ctx, oracle, n):
    from provekit_amd import whir_pcs
    from provekit_amd.field import random_field

    cfg = K.small_config(n, 2)
    bufs = [ctx.upload(random_field(1 << n, 40 + b)) for b in range(2)]
    scheme = whir_pcs.Scheme(ctx, cfg)
    com = scheme.commit(bufs)
    root = com.root()
    proofs = []
    for seed in (1, 2):  # the same commitment, two point sets
        pts = random_field(3 * n, 90 + seed).reshape(3, n, 4)
        evals, proof = scheme.open(com, pts)
        r, bound = whir_pcs.verify(cfg, pts, proof, expected_root=root)
        assert r.accepted and r.offset == len(proof), r
        assert np.array_equal(bound, evals) and np.array_equal(evals, whir_pcs.evaluate(ctx, bufs, n, pts))
        assert proof[:32] == root
        again = scheme.open(com, pts)[1]
        assert again == proof  # no randomness: the same inputs give the same bytes
        proofs.append(proof)
    assert proofs[0] != proofs[1]
    com.close()
    scheme.close()


def test_refusals_leave_the_context_usable(ctx, oracle):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError
    from provekit_amd.field import random_field

    n = 8
    cfg = K.small_config(n, 1)
    scheme, other = whir_pcs.Scheme(ctx, cfg), whir_pcs.Scheme(ctx, cfg)
    buf = ctx.upload(random_field(1 << n, 3))
    com, foreign = scheme.commit([buf]), other.commit([buf])
    pts = random_field(65 * n, 4).reshape(65, n, 4)
    n_out, evals = whir_pcs.sz(), np.zeros((65, 4), dtype=np.uint64)
    big = (whir_pcs.C.c_uint8 * (1 << 20))()
    for q in (0, 65):
        rc = whir_pcs.lib.pkw_open(scheme.handle, com.handle, pts.ctypes.data, q, evals.ctypes.data, big, len(big), whir_pcs.C.byref(n_out))
        assert rc == -1 and b"1..64" in whir_pcs.lib.pkw_last_error(scheme.handle)
    with pytest.raises(ProveKitHipError, match="too small") as e:
        scheme.open(com, pts[:2], cap=100)
    assert e.value.code == -1  # PK_ERR_BAD_ARG
    with pytest.raises(ProveKitHipError, match="another scheme") as e:
        scheme.open(foreign, pts[:2])
    assert e.value.code == -1
    bad = K.small_config(n, 1)
    bad.batch_size = 7
    with pytest.raises(ProveKitHipError):
        whir_pcs.Scheme(ctx, bad)
    # the scheme, the commitment and the context still work
    ev, proof = scheme.open(com, pts[:2])
    assert whir_pcs.verify(cfg, pts[:2], proof, expected_root=com.root())[0].accepted
    assert np.array_equal(ev, whir_pcs.evaluate(ctx, [buf], n, pts[:2]))
    for x in (com, foreign, scheme, other):
        x.close()


def test_cpp_host_commits_opens_verifies_and_sees_a_rejection():
    assert os.path.exists(DEMO), "examples/pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run([DEMO, "12", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n_vars=12 points=2 proof_bytes=")
    assert "rejected, check=WHIR_SUMCHECK" in lines[1]
