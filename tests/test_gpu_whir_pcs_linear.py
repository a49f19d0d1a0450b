"""GPU: the linear statements of libprovekit_whir.so on the device.  pkw_weighted_sums bit-exact against Python ints at every size
at which the kernel takes another path, on every grid and register tile; the combination kernel through its probe; pkw_open_linear's
bytes against the transcript the oracle prover's parts write; round trips; the refusals; examples/pcs_linear_demo."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
DEMO = os.path.join(ROOT, "examples", "pcs_linear_demo")

import whir_pcs_cases as K  # noqa: E402
from whir_pcs_cases import low_vars, ptrs, resolve_n  # noqa: E402
import whir_pcs_linear_cases as L  # noqa: E402

T_WS = (2, 4)  # the weight extents of the kernel's register tiles: 2 x 2, and 1 x 4 for a single polynomial (csrc/whir_pcs/linear.hpp)
MAX_L = 17  # two full passes of eight weights and a third pass of one


@functools.lru_cache(maxsize=None)
def sums_case(n):
    """four polynomials and seventeen weights per size and their Python-int inner products, computed once.  Weight 1 is all zero;
    weight 3 repeats weight 0"""
    polys = K.polynomials(n, 4, seed=13 + n)
    weights = [K.random_ints(1 << n, 500 * n + i) for i in range(MAX_L)]
    for w in weights:
        w[0] = K.P - 1
    weights[1] = [0] * (1 << n)
    weights[3] = list(weights[0])
    return polys, weights, L.expected_sums(polys, weights)


@pytest.mark.parametrize("batch", [1, 2, 3, 4])
@pytest.mark.parametrize("label", ["0", "1", "4", "b-1", "b", "b+1", "13"])
def test_weighted_sums_are_bit_exact_against_python_ints(ctx, oracle, label, batch):
    from provekit_amd import whir_pcs

    n = resolve_n(label)
    polys, weights, want = sums_case(n)
    f = [ctx.upload(L.mont(oracle, p)) for p in polys[:batch]]
    w = [ctx.upload(L.mont(oracle, x)) for x in weights]
    for l in sorted({1, 16, 17} | {t + d for t in T_WS for d in (-1, 0, 1)}):  # 1, T_w - 1, T_w, T_w + 1 of either tile, 16, 17
        got = whir_pcs.weighted_sums(ctx, f, n, w[:l])
        assert got.shape == (batch, l, 4)
        assert oracle.limbs_to_ints(oracle.from_mont(got.reshape(-1, 4))) == [want[b][i] for b in range(batch) for i in range(l)], (n, batch, l)
        if l >= 4:
            assert not got[:, 1].any() and np.array_equal(got[:, 0], got[:, 3])  # the zero weight; two equal weights
    again = whir_pcs.weighted_sums(ctx, f, n, w[:3])  # a second call on the same buffers
    assert np.array_equal(again, whir_pcs.weighted_sums(ctx, f, n, w[:3]))
    # a weight that IS a polynomial: <f_0, f_b>
    got = whir_pcs.weighted_sums(ctx, f, n, [f[0]])
    assert oracle.limbs_to_ints(oracle.from_mont(got.reshape(-1, 4))) == [sum(a * c for a, c in zip(polys[0], polys[b])) % K.P for b in range(batch)]
    for x in f + w:
        x.free()


@pytest.mark.parametrize("n,grid,per_lane", [(12, 16, "1"), (12, 6, "3 and 2"), (12, 4, "4"), (12, 3, "6 and 5"), (4, 1, "1"), (9, 2, "1"), (10, 1, "4")])
def test_weighted_sums_of_all_p_minus_1_at_every_phase_of_a_reduction_group(ctx, oracle, n, grid, per_lane):
    """every operand p - 1: the column accumulators at their bound.  A lane makes one product per element it sees, and reduces once
    per DOT29_GROUP = 4: grids on which the lanes see 1, 3, 4 and 5 elements end in every phase.  The public entry's grid is a power
    of two, so the odd counts come through the probe, which takes the grid; the result must not depend on it, nor on the tile."""
    import pk_probes

    top = oracle.ints_to_limbs([K.P - 1] * (1 << n))  # the LIMBS are p - 1: the largest operand the kernel's contract allows
    f = [ctx.upload(top) for _ in range(3)]
    w = [ctx.upload(top) for _ in range(3)]
    want = oracle.ints_to_limbs([(K.P - 1) ** 2 * (1 << n) * pow(1 << 256, -1, K.P) % K.P])[0]  # a sum of Montgomery products
    for tile in (0, 1, 2, 3):
        out = np.zeros((3, 3, 4), dtype=np.uint64)
        ctx._check(pk_probes.lib.pk_probe_whir_weighted_sums(ctx.handle, ptrs(f), 3, n, ptrs(w), 3, grid, tile, out.ctypes.data))
        assert (out == want).all(), (tile, per_lane)
    for x in f + w:
        x.free()


@functools.lru_cache(maxsize=None)
def finish_case(n):
    """n_vars = 17, the smallest size whose grid reaches 512 workgroups: three polynomials and eight weights (one full pass) with
    their Python-int inner products, computed once"""
    polys = [K.many_ints(1 << n, 20 + b) for b in range(3)]
    weights = [K.many_ints(1 << n, 30 + i) for i in range(8)]
    return polys, weights, L.expected_sums(polys, weights)


GRIDS_13 = ((1, 0), (5, 0), (31, 0), (32, 1), (7, 1), (32, 2), (3, 2), (32, 3), (9, 3))
# the finish kernel sums 1, 2, 256 (one partial per lane), 257 (one lane makes a second trip) and 512 (all do) partials per output
GRIDS_17 = ((1, 0), (2, 0), (256, 0), (257, 0), (512, 0), (257, 1), (257, 3))


# l = 5: rows of five partial sums, fewer than a pass; l = 8: a full pass
@pytest.mark.parametrize("n,l,full,grids", [(13, 5, 32, GRIDS_13), (17, 5, 512, GRIDS_17), (17, 8, 512, GRIDS_17)],
                         ids=["13-l5", "17-l5", "17-l8"])
def test_weighted_sums_do_not_depend_on_the_grid_or_the_tile(ctx, oracle, n, l, full, grids):
    import pk_probes
    from provekit_amd import whir_pcs

    polys, weights, want = sums_case(n) if n == 13 else finish_case(n)
    f = [ctx.upload(L.mont(oracle, p)) for p in polys[:3]]
    w = [ctx.upload(L.mont(oracle, x)) for x in weights[:l]]
    ref = whir_pcs.weighted_sums(ctx, f, n, w)
    assert oracle.limbs_to_ints(oracle.from_mont(ref.reshape(-1, 4))) == [want[b][i] for b in range(3) for i in range(l)]
    assert pk_probes.lib.pk_probe_whir_wsum_grid(n) == full
    for grid, tile in grids:
        out = np.zeros_like(ref)
        ctx._check(pk_probes.lib.pk_probe_whir_weighted_sums(ctx.handle, ptrs(f), 3, n, ptrs(w), l, grid, tile, out.ctypes.data))
        assert np.array_equal(out, ref), (grid, tile)
    out = np.zeros_like(ref)
    assert pk_probes.lib.pk_probe_whir_weighted_sums(ctx.handle, ptrs(f), 3, n, ptrs(w), l, full + 1, 0, out.ctypes.data) == -1  # beyond the scratch
    assert whir_pcs.lib.pkw_weighted_sums(ctx.handle, ptrs(f), 3, n, ptrs(w), 0, out.ctypes.data) == -1  # l = 0
    assert np.array_equal(whir_pcs.weighted_sums(ctx, f, n, w), ref)
    for x in f + w:
        x.free()


def test_weighted_sums_with_several_steps_per_workgroup(ctx, oracle):
    """from 2^18 the grid stays at 512 workgroups and a lane takes more than one element: 2^18 is the smallest such size (two).
    Reference: the C oracle's dot product."""
    import pk_probes
    from provekit_amd import whir_pcs
    from provekit_amd.field import random_field

    n = low_vars() + 10
    assert pk_probes.lib.pk_probe_whir_wsum_grid(n - 1) == pk_probes.lib.pk_probe_whir_wsum_grid(n) == 512
    polys = [random_field(1 << n, 70 + b) for b in range(2)]
    weights = [random_field(1 << n, 80 + i) for i in range(3)]
    f, w = [ctx.upload(p) for p in polys], [ctx.upload(x) for x in weights]
    got = whir_pcs.weighted_sums(ctx, f, n, w)
    for b in range(2):
        for i in range(3):
            assert np.array_equal(got[b, i], oracle.dot(weights[i], polys[b]).reshape(4)), (b, i)
    for x in f + w:
        x.free()


@pytest.mark.parametrize("n", [4, 9, 13])
def test_the_sums_against_eq_tables_are_the_evaluations(ctx, oracle, n):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import lib

    polys = K.polynomials(n, 2, seed=11 + n)
    pts = K.mont_points(oracle, K.points(n, 3))
    f = [ctx.upload(L.mont(oracle, p)) for p in polys]
    tables = [ctx.alloc_fe(1 << n) for _ in range(3)]
    for i, t in enumerate(tables):
        ctx._check(lib.pk_eq_table(ctx.handle, pts[i].ctypes.data, n, t.ptr))
    assert np.array_equal(whir_pcs.weighted_sums(ctx, f, n, tables), whir_pcs.evaluate(ctx, f, n, pts))
    for x in f + tables:
        x.free()


@pytest.mark.parametrize("l", [1, 15, 16, 17, 33])
def test_the_combination_kernel_against_python_ints(ctx, oracle, l):
    """W (+)= sum_i s_i w_i through the probe: a length that is no multiple of the workgroup, l across the 16-weight pass, scales 0, 1
    and p - 1, overwriting a non-zero table and accumulating onto it"""
    import pk_probes

    length = 1000
    weights = [K.random_ints(length, 300 + i) for i in range(l)]
    weights[0][0], weights[0][1], weights[0][2] = 0, 1, K.P - 1
    scales = K.random_ints(l, 17)
    for i, special in enumerate((K.P - 1, 0, 1)):
        if i < l:
            scales[-1 - i] = special
    before = K.random_ints(length, 5)
    before[0] = K.P - 1
    combo = [sum(s * w[x] for s, w in zip(scales, weights)) % K.P for x in range(length)]
    w = [ctx.upload(L.mont(oracle, x)) for x in weights]
    sc = L.mont(oracle, scales)
    for accumulate in (0, 1):
        d = ctx.upload(L.mont(oracle, before))
        ctx._check(pk_probes.lib.pk_probe_whir_combine(ctx.handle, d.ptr, length, ptrs(w), sc.ctypes.data, l, accumulate))
        got = oracle.limbs_to_ints(oracle.from_mont(ctx.download_fe(d.ptr, length)))
        assert got == ([(a + c) % K.P for a, c in zip(before, combo)] if accumulate else combo), accumulate
        d.free()
    for x in w:
        x.free()


@pytest.mark.parametrize("hash_version", [2, 1])
@pytest.mark.parametrize("shape", L.SHAPES)
def test_open_linear_writes_the_oracles_transcript_byte_for_byte(ctx, oracle, shape, hash_version):
    from provekit_amd import whir_pcs

    n, batch, q, l = shape
    cfg = K.small_config(n, batch)
    polys, pts = K.polynomials(n, batch), (K.points(n, q) if q else [])
    weights, tags = L.weight_tables(oracle, n, l), L.tags(l)
    want, root, vals, sums = L.oracle_linear_opening(oracle, cfg, polys, pts, weights, tags, whir_pcs.io_pattern_linear(cfg, q, l), hash_version=hash_version)
    mpts = K.mont_points(oracle, pts) if q else None
    mweights, mtags = [L.mont(oracle, w) for w in weights], L.mont(oracle, tags)
    ctx.set_hash_version(hash_version)
    try:
        scheme = whir_pcs.Scheme(ctx, cfg)
        com = scheme.commit([ctx.upload(L.mont(oracle, p)) for p in polys])
        assert com.root() == root
        d_w = [ctx.upload(w) for w in mweights]
        evals, got_sums, proof = scheme.open_linear(com, mpts, d_w, mtags)
    finally:
        ctx.set_hash_version(2)
    assert oracle.limbs_to_ints(oracle.from_mont(got_sums.reshape(-1, 4))) == [s for row in sums for s in row]
    if q:
        assert oracle.limbs_to_ints(oracle.from_mont(evals.reshape(-1, 4))) == [v for row in vals for v in row]
    assert len(proof) == len(want) and proof == want
    v = whir_pcs.verify_linear(cfg, mpts, mtags, mweights, proof, expected_root=root, hash_version=hash_version)
    assert v.result.accepted and v.unchecked == 0, v.result
    for x in d_w:
        x.free()
    com.close()
    scheme.close()


@pytest.mark.parametrize("n", [12, 16])
def test_round_trip_of_both_statements_over_one_commitment(ctx, oracle, n):
    from provekit_amd import whir_pcs
    from provekit_amd.field import random_field

    cfg = K.small_config(n, 2)
    polys = [random_field(1 << n, 40 + b) for b in range(2)]
    bufs = [ctx.upload(p) for p in polys]
    scheme = whir_pcs.Scheme(ctx, cfg)
    com = scheme.commit(bufs)
    root = com.root()
    pts = random_field(3 * n, 91).reshape(3, n, 4)
    evals, proof = scheme.open(com, pts)
    # pkw_open's bytes are what they were: the oracle's transcript of the evaluation statement
    ints = [oracle.limbs_to_ints(oracle.from_mont(p)) for p in polys]
    ipts = [oracle.limbs_to_ints(oracle.from_mont(p)) for p in pts]
    want, want_root, _ = K.oracle_opening(oracle, cfg, ints, ipts, whir_pcs.io_pattern(cfg, 3))
    assert want_root == root and proof == want
    r, bound = whir_pcs.verify(cfg, pts, proof, expected_root=root)
    assert r.accepted and np.array_equal(bound, evals), r
    weights = [random_field(1 << n, 50 + i) for i in range(2)]
    d_w = [ctx.upload(w) for w in weights]
    tags = random_field(2, 8)
    ev2, sums, lproof = scheme.open_linear(com, pts[:1], d_w, tags)
    assert np.array_equal(ev2, evals[:, :1]) and np.array_equal(sums, whir_pcs.weighted_sums(ctx, bufs, n, d_w))
    v = whir_pcs.verify_linear(cfg, pts[:1], tags, weights, lproof, expected_root=root)
    assert v.result.accepted and v.result.offset == len(lproof) and v.unchecked == 0, v.result
    assert np.array_equal(v.sums, sums) and np.array_equal(v.evals, ev2)
    # the tables withheld: the caller closes the condition with pkw_evaluate at the folding point
    v = whir_pcs.verify_linear(cfg, pts[:1], tags, None, lproof, expected_root=root)
    assert v.result.accepted and v.unchecked == 2
    assert np.array_equal(whir_pcs.evaluate(ctx, d_w, n, v.fold_point.reshape(1, n, 4))[:, 0], v.deferred)
    assert scheme.open(com, pts)[1] == proof and scheme.open_linear(com, pts[:1], d_w, tags)[2] == lproof  # either order, the same bytes
    for x in d_w:
        x.free()
    com.close()
    scheme.close()


def test_refusals_of_a_linear_opening_leave_the_context_usable(ctx, oracle):
    from provekit_amd import whir_pcs
    from provekit_amd.field import random_field

    n = 8
    cfg = K.small_config(n, 1)
    scheme = whir_pcs.Scheme(ctx, cfg)
    buf = ctx.upload(random_field(1 << n, 3))
    com = scheme.commit([buf])
    weights = [random_field(1 << n, 20 + i) for i in range(2)]
    d_w = [ctx.upload(w) for w in weights]
    tags = random_field(17, 6)
    pts = random_field(65 * n, 4).reshape(65, n, 4)
    first = scheme.open_linear(com, pts[:1], d_w, tags[:2])
    big, n_out = (C.c_uint8 * (1 << 20))(), whir_pcs.sz()
    many = (C.c_void_p * 17)(*([d_w[0].ptr] * 17))
    holed = (C.c_void_p * 2)(d_w[0].ptr, None)

    def call(q, weights_arr, l):
        return whir_pcs.lib.pkw_open_linear(scheme.handle, com.handle, pts.ctypes.data, q, C.cast(weights_arr, C.c_void_p), tags.ctypes.data, l, None, None,
                                            big, len(big), C.byref(n_out))

    for q, arr, l, why in ((1, many, 0, b"1..16"), (1, many, 17, b"1..16"), (65, many, 1, b"0..64"), (1, holed, 2, b"weight 1 is a null pointer")):
        assert call(q, arr, l) == -1 and why in whir_pcs.lib.pkw_last_error(scheme.handle), (q, l)
    again = scheme.open_linear(com, pts[:1], d_w, tags[:2])
    assert again[2] == first[2] and np.array_equal(again[1], first[1])
    assert whir_pcs.verify_linear(cfg, pts[:1], tags[:2], weights, again[2], expected_root=com.root()).result.accepted
    for x in d_w + [com, scheme]:
        (x.free if hasattr(x, "free") else x.close)()


def test_cpp_host_opens_a_linear_statement_verifies_both_ways_and_sees_a_rejection():
    assert os.path.exists(DEMO), "examples/pcs_linear_demo is built by __graft_entry__.build()"
    out = subprocess.run([DEMO, "12", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n_vars=12 points=1 weights=2 proof_bytes=")
    assert "unchecked=2" in lines[1] and "closed with pkw_evaluate" in lines[1]
    assert "rejected, check=WHIR_SUMCHECK" in lines[2]
