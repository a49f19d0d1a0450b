"""GPU: hiding commitments on the device (include/provekit_whir_hiding.h).  The stage kernel against oracle/prover_ref.py's random_fe
segment by segment, at every size at which its grid rule or a lane's walk changes, on grids 1, 2 and the default; pkw_commit_hiding's
root against plain pkw_commit on host-built extended tables; pkw_open_hiding's bytes against the transcript the oracle prover's
parts write; seeds; the refusals, each with its message; examples/pcs_hiding_demo."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
DEMO = os.path.join(ROOT, "examples", "pcs_hiding_demo")

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_hiding_cases as H  # noqa: E402

OTHER_KEY = bytes(range(1, 33))
# n = 1: a mask segment is ONE pair.  For B = 1 the 3 * 2^(n-1) pairs fit one pair per lane of the single workgroup up to n = 7 (192)
# and a lane takes a second pair from n = 8 (384); the grid rule gives a second workgroup from n = 11 (3072 > 2048 pairs).  For
# B = 3 (5 * 2^(n-1) pairs) those sizes are n = 6 | 7 and n = 9 | 10.  n = 9 | 10 is also where the pairs of one MASK segment fill one
# 256-lane workgroup exactly, and then two
STAGE_SIZES = [1, 6, 7, 8, 9, 10, 11]


def test_the_grid_rule_is_what_the_stage_sizes_straddle(ctx):  # ctx: the fixture initialises the HIP runtime before a library of ours loads
    import pk_probes

    lib = pk_probes.lib
    threads, per_lane = lib.pk_probe_whir_hiding_threads(), lib.pk_probe_whir_hiding_pairs_per_lane()
    assert (threads, per_lane) == (256, 8)  # STAGE_SIZES were chosen for these; another shape needs another look at them
    for B in (1, 2, 3):
        for n in range(1, 16):
            pairs = (B + 2) << (n - 1)
            assert lib.pk_probe_whir_hiding_grid(B, n) == max(1, -(-pairs // (threads * per_lane)))
    pairs = {B: {n: (B + 2) << (n - 1) for n in STAGE_SIZES} for B in (1, 3)}
    assert pairs[1][7] <= threads < pairs[1][8] and pairs[3][6] <= threads < pairs[3][7]  # a lane's second pair
    assert pairs[1][10] <= threads * per_lane < pairs[1][11] and pairs[3][9] <= threads * per_lane < pairs[3][10]  # the second workgroup
    assert [lib.pk_probe_whir_hiding_grid(1, n) for n in (10, 11)] == [1, 2] and [lib.pk_probe_whir_hiding_grid(3, n) for n in (9, 10)] == [1, 2]
    assert 1 << (9 - 1) == threads  # the mask pairs at n = 9 fill one workgroup


def test_rejected_candidates_occur_in_every_segment_of_512_elements(ctx):
    """the oracle's side of the retry path: at 2^9 elements per segment about a quarter of the candidates are rejected, so the stage
    test below cannot pass without the (pair, attempt) walk taking its retry branch; the C oracle and the Python cipher agree"""
    import prover_ref as PR
    from rng_pow_refs import draw_ref

    mask0, g, _ = H.streams()
    for stream in (mask0, mask0 + 2, g):
        vals, attempts = draw_ref(H.KEY, stream, 512)
        retried = sum(a > 1 for a in attempts)
        assert 64 <= retried <= 192 and max(attempts) >= 3, (stream, retried)
        limbs = PR.random_fe(H.KEY, stream, 512)
        assert [int.from_bytes(limbs[i].tobytes(), "little") for i in range(512)] == vals


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", STAGE_SIZES)
def test_the_stage_kernel_draws_every_segment_as_the_oracle_does_on_any_grid(ctx, oracle, n, B):
    import pk_probes
    import prover_ref as PR

    mask0, g, _ = H.streams()
    N = 1 << n
    want = [PR.random_fe(H.KEY, mask0 + b, N) for b in range(B)] + [PR.random_fe(H.KEY, g, 2 * N)]
    lower = [np.full((N, 4), 0xA5A5A5A5A5A5A5A5 + b, dtype=np.uint64) for b in range(B)]  # what the launch must not touch
    first = None
    for grid in (0, 1, 2):
        bufs = [ctx.upload(np.concatenate([lower[b], np.zeros((N, 4), dtype=np.uint64)])) for b in range(B)] + [ctx.upload(np.zeros((2 * N, 4), dtype=np.uint64))]
        rc = pk_probes.lib.pk_probe_whir_hiding_fill(ctx.handle, K.ptrs(bufs), B, n, H.KEY, grid)
        assert rc == 0
        got = [ctx.download_fe(b, 2 * N) for b in bufs]
        for b in range(B):
            assert np.array_equal(got[b][:N], lower[b]), (grid, b)
            assert np.array_equal(got[b][N:], want[b]), (grid, b)
        assert np.array_equal(got[B], want[B]), grid
        if first is None:
            first = got
        assert all(np.array_equal(x, y) for x, y in zip(first, got))  # the bits do not depend on the launch shape
        for b in bufs:
            b.free()
    assert len({w[:2].tobytes() for w in want}) == B + 1  # every segment its own stream


def upload_tables(ctx, oracle, tables):
    return [ctx.upload(oracle.to_mont(oracle.ints_to_limbs(t))) for t in tables]


@pytest.mark.parametrize("hash_version", [2, 1])
@pytest.mark.parametrize("n1,B", [(8, 1), (12, 3)])
def test_commit_hiding_is_the_plain_commitment_of_the_host_built_extended_tables(ctx, oracle, n1, B, hash_version):
    from provekit_amd import whir_pcs

    cfg = H.hiding_config(n1, B)
    f, ext, draws = H.extended_tables(n1 - 1, B)
    ctx.set_hash_version(hash_version)
    try:
        hiding, plain = whir_pcs.Scheme(ctx, cfg, hiding=True), whir_pcs.Scheme(ctx, cfg)
        d_f, d_ext = upload_tables(ctx, oracle, f), upload_tables(ctx, oracle, ext)
        for b in range(B):  # the host-built table holds the drawn words as they are
            assert np.array_equal(ctx.download_fe(d_ext[b], 1 << n1)[1 << (n1 - 1) :], draws[b])
        com, ref = hiding.commit_hiding(d_f, seed=H.KEY), plain.commit(d_ext)
        assert com.root() == ref.root()
    finally:
        ctx.set_hash_version(2)
    for x in (com, ref, hiding, plain, *d_f, *d_ext):
        (x.close if hasattr(x, "close") else x.free)()


@pytest.mark.parametrize("shape", H.SHAPES + [(12, 1, 9)])  # 9 points: the evaluation kernel's second pass
def test_open_hiding_writes_the_oracles_transcript_byte_for_byte(ctx, oracle, shape):
    from provekit_amd import whir_pcs

    c = H.case(oracle, shape)
    scheme = whir_pcs.Scheme(ctx, c.cfg, hiding=True)
    d_f = upload_tables(ctx, oracle, c.f)
    com = scheme.commit_hiding(d_f, seed=H.KEY)
    assert com.root() == c.root
    evals, proof = scheme.open_hiding(com, c.mpts)
    assert evals.shape == (c.B, c.q, 4)
    assert oracle.limbs_to_ints(oracle.from_mont(evals.reshape(-1, 4))) == [v for row in c.expected for v in row]
    assert len(proof) == len(c.proof) and proof == c.proof
    r, bound = whir_pcs.verify_hiding(c.cfg, c.mpts, proof, expected_root=com.root())
    assert r.accepted and r.offset == len(proof), r
    assert np.array_equal(bound, evals)
    for x in (com, scheme):
        x.close()
    for b in d_f:
        b.free()


def test_seeds_change_the_root_the_proof_and_g_but_not_the_evaluations(ctx, oracle):
    from provekit_amd import whir_pcs

    c = H.case(oracle, (8, 3, 3))
    scheme = whir_pcs.Scheme(ctx, c.cfg, hiding=True)
    d_f = upload_tables(ctx, oracle, c.f)
    seen = {}
    for key in (H.KEY, OTHER_KEY):
        com = scheme.commit_hiding(d_f, seed=key)
        evals, proof = scheme.open_hiding(com, c.mpts)
        assert whir_pcs.verify_hiding(c.cfg, c.mpts, proof, expected_root=com.root())[0].accepted
        g_at = proof[c.eval_offset + 32 * c.q * c.B : c.eval_offset + 32 * c.q * (c.B + 1)]  # g(0, z_i) on the transcript
        seen[key] = (com.root(), proof, g_at, evals)
        com.close()
    a, b = seen[H.KEY], seen[OTHER_KEY]
    assert a[0] != b[0] and a[1] != b[1] and a[2] != b[2] and np.array_equal(a[3], b[3])
    assert a[1][c.eval_offset : c.eval_offset + 32 * c.q * c.B] == b[1][c.eval_offset : c.eval_offset + 32 * c.q * c.B]  # f's rows on the transcript
    fresh = [scheme.commit_hiding(d_f) for _ in range(2)]  # no seed: the key comes from the OS
    assert len({x.root() for x in fresh} | {a[0], b[0]}) == 4
    for x in (*fresh, scheme):
        x.close()
    for x in d_f:
        x.free()


def test_refusals_each_with_its_message_leave_everything_usable(ctx, oracle):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    c = H.case(oracle, (8, 1, 1))
    scheme, other = whir_pcs.Scheme(ctx, c.cfg, hiding=True), whir_pcs.Scheme(ctx, c.cfg, hiding=True)
    d_f = upload_tables(ctx, oracle, c.f)
    com, foreign = scheme.commit_hiding(d_f, seed=H.KEY), other.commit_hiding(d_f, seed=H.KEY)
    pts = np.concatenate([c.mpts] * 65)
    n_out, evals = whir_pcs.sz(), np.zeros((65, 4), dtype=np.uint64)
    big = (C.c_uint8 * (1 << 20))()
    open_raw = whir_pcs.lib.pkw_open_hiding
    for q in (0, 65):
        assert open_raw(scheme.handle, com.handle, pts.ctypes.data, q, evals.ctypes.data, big, len(big), C.byref(n_out)) == -1
        assert b"1..64" in whir_pcs.lib.pkw_last_error(scheme.handle)
    assert open_raw(scheme.handle, com.handle, pts.ctypes.data, 1, evals.ctypes.data, big, 100, C.byref(n_out)) == -1  # cap too small: *len is set
    assert b"too small" in whir_pcs.lib.pkw_last_error(scheme.handle) and n_out.value == len(c.proof)
    with pytest.raises(ProveKitHipError, match="another scheme") as e:
        scheme.open_hiding(foreign, c.mpts)
    assert e.value.code == -1
    # a plain scheme whose config breaks a hiding rule, and the hiding scheme that cannot be made of it
    loose = K.small_config(8, 2)
    assert H.budget(loose)[0] > H.budget(loose)[1]
    plain = whir_pcs.Scheme(ctx, loose)
    with pytest.raises(ProveKitHipError, match="not a hiding scheme: mask budget: 321 values") as e:
        plain.commit_hiding(d_f, seed=H.KEY)
    assert e.value.code == -1
    with pytest.raises(ProveKitHipError, match="mask budget: 321 values") as e:
        whir_pcs.Scheme(ctx, loose, hiding=True)
    assert e.value.code == -1
    with pytest.raises(ProveKitHipError, match="batch_size must be 2..4"):
        whir_pcs.Scheme(ctx, K.small_config(8, 1), hiding=True)
    # none of the refused calls counted as the opening: the first one that hands out a proof does, and the next is refused
    ev, proof = scheme.open_hiding(com, c.mpts)
    assert proof == c.proof and whir_pcs.verify_hiding(c.cfg, c.mpts, proof, expected_root=com.root())[0].accepted
    with pytest.raises(ProveKitHipError, match="already opened") as e:
        scheme.open_hiding(com, c.mpts)
    assert e.value.code == -1
    assert other.open_hiding(foreign, c.mpts)[1] == c.proof  # its own scheme opens the other commitment
    for x in (com, foreign, scheme, other, plain):
        x.close()
    for x in d_f:
        x.free()


def test_cpp_host_commits_opens_verifies_is_refused_a_second_opening_and_sees_a_rejection():
    assert os.path.exists(DEMO), "examples/pcs_hiding_demo is built by __graft_entry__.build()"
    out = subprocess.run([DEMO, "12", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert any("a second opening: refused" in ln and "already opened" in ln for ln in lines)
    assert lines[-2].startswith("ok n=12 points=2 proof_bytes=") and "rejected, check=" in lines[-1]
