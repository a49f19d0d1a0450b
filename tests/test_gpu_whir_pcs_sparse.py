"""GPU: sparse weights (index/value lists) on the device.  pkw_sparse_sums, pkw_sparse_accumulate and pkw_sparse_evaluate bit-exact
against their dense twins on the densified tables and against Python ints, at the sizes at which the kernels take another path;
the validation pass's refusals from every entry point (nothing is gathered or scattered through a bad index: no fault is provoked);
pkw_open_sparse's bytes against pkw_open_linear's on the densified tables and against the oracle's transcript; examples/pcs_sparse_demo."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
DEMO = os.path.join(ROOT, "examples", "pcs_sparse_demo")

import whir_pcs_cases as K  # noqa: E402
from whir_pcs_cases import ptrs  # noqa: E402
import whir_pcs_linear_cases as L  # noqa: E402
import whir_pcs_sparse_cases as S  # noqa: E402

NAMES_BOTH = re.compile(r"weight \d+.*entry \d+", re.S)


def step():
    """entries a workgroup takes per step"""
    import pk_probes

    w = pk_probes.lib.pk_probe_whir_sparse_threads()
    assert w == 256  # the lengths below straddle it
    return w


def ints(oracle, limbs):
    return oracle.limbs_to_ints(oracle.from_mont(np.ascontiguousarray(limbs).reshape(-1, 4)))


@functools.lru_cache(maxsize=None)
def sums_case(n):
    """four polynomials and sixteen weights whose lengths are 0, 1, W - 1, W, W + 1 and 2^n (as far as 2^n allows), in turns --
    very different lengths side by side -- with their Python-int sums, computed once"""
    N, W = 1 << n, step()
    lengths = [x for x in (0, 1, W - 1, W, W + 1, N, 2, N // 2 + 1) if x <= N]
    polys = K.polynomials(n, 4, seed=17 + n)
    ws = []
    for i in range(16):
        nnz = lengths[i % len(lengths)]
        ws.append((list(range(N)), K.random_ints(N, 900 + i)) if nnz == N else S.random_weight(n, nnz, 700 * n + i))
    for idx, val in ws:
        if val:
            val[0] = K.P - 1
    return polys, ws, S.sums(polys, ws)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 13])
def test_sparse_sums_equal_the_dense_sums_and_python_ints(ctx, oracle, n):
    from provekit_amd import whir_pcs

    polys, ws, want = sums_case(n)
    f = [ctx.upload(L.mont(oracle, p)) for p in polys]
    dense = [ctx.upload(L.mont(oracle, S.densify(n, w))) for w in ws]
    packed = {l: S.pack(oracle, ws[:l]).upload(ctx) for l in (1, 2, 16)}
    for batch in (1, 2, 3, 4):
        for l in (16, 1, 2):  # the output of one call is sized unlike the next one's
            got = whir_pcs.sparse_sums(ctx, f[:batch], n, packed[l])
            assert got.shape == (batch, l, 4)
            assert ints(oracle, got) == [want[b][i] for b in range(batch) for i in range(l)], (n, batch, l)
            assert np.array_equal(got, whir_pcs.weighted_sums(ctx, f[:batch], n, dense[:l])), (n, batch, l)
    again = whir_pcs.sparse_sums(ctx, f[:3], n, packed[16])
    assert ints(oracle, again) == [want[b][i] for b in range(3) for i in range(16)]
    assert whir_pcs.sparse_sums(ctx, f[:2], n, whir_pcs.SparseWeights()).shape == (2, 0, 4)  # l = 0: nothing to do
    for x in f + dense + list(packed.values()):
        x.free()


@functools.lru_cache(maxsize=None)
def finish_case():
    """n_vars = 17, the smallest size whose grid reaches 512 workgroups: three polynomials, a weight with an entry at every position
    (every workgroup of every grid has one), a weight of 256 W + 1 entries (on a grid of 257 the last workgroup takes exactly one; on
    512 the workgroups beyond it write zero partials) and an empty one, with their Python-int sums, computed once"""
    n, W = 17, step()
    polys = [K.many_ints(1 << n, 50 + b) for b in range(3)]
    some = sorted(int(x) for x in np.random.default_rng(9).choice(1 << n, size=256 * W + 1, replace=False))
    ws = [(list(range(1 << n)), K.many_ints(1 << n, 60)), (some, K.many_ints(len(some), 61)), ([], [])]
    return n, polys, ws, S.sums(polys, ws)


def stride_case():
    """G workgroups of W lanes and G W - 1, G W, G W + 1 and 2 G W + 1 entries, on small grids"""
    n, W, G = 13, step(), 2
    polys = K.polynomials(n, 3, seed=5)
    ws = [S.random_weight(n, nnz, 40 + nnz) for nnz in (G * W - 1, G * W, G * W + 1, 2 * G * W + 1, 0, 1)]
    return n, polys, ws, S.sums(polys, ws)


# (the case, the library's own grid for its longest weight, wsum_grid(n), the grids handed to the probe)
@pytest.mark.parametrize("case,own,full,grids", [(stride_case, 5, 32, (2, 1, 3, 32)), (finish_case, 512, 512, (1, 2, 256, 257, 512))],
                         ids=["stride loop", "finish kernel"])
def test_sparse_sums_with_a_stride_loop_on_any_grid(ctx, oracle, case, own, full, grids):
    """a weight longer than its grid's extent, on a small grid handed to the launch through the probe (the library's own grid
    reaches this only at a large size); the bits do not depend on the grid.  The second case is the finish kernel's: rows of
    SPARSE_PASS = 8 partial sums of which three are used, summed over 1, 2, 256 (one partial per lane), 257 (one lane makes a
    second trip) and 512 (all do) workgroups"""
    import pk_probes
    from provekit_amd import whir_pcs

    n, polys, ws, sums = case()
    want = [x for row in sums for x in row]
    f = [ctx.upload(L.mont(oracle, p)) for p in polys]
    sw = S.pack(oracle, ws).upload(ctx)
    assert pk_probes.lib.pk_probe_whir_sparse_grid(n, max(len(idx) for idx, _ in ws), 1) == own and pk_probes.lib.pk_probe_whir_wsum_grid(n) == full
    ref = whir_pcs.sparse_sums(ctx, f, n, sw)
    assert ints(oracle, ref) == want
    for grid in grids:
        out = np.zeros_like(ref)
        ctx._check(pk_probes.lib.pk_probe_whir_sparse_sums(ctx.handle, ptrs(f), 3, n, sw.offsets.ctypes.data, sw.d_index.ptr, sw.d_value.ptr, sw.l, grid,
                                                           out.ctypes.data))
        assert np.array_equal(out, ref), grid
    out = np.zeros_like(ref)
    assert pk_probes.lib.pk_probe_whir_sparse_sums(ctx.handle, ptrs(f), 3, n, sw.offsets.ctypes.data, sw.d_index.ptr, sw.d_value.ptr, sw.l, full + 1,
                                                   out.ctypes.data) == -1  # beyond the scratch
    for x in f + [sw]:
        x.free()


@pytest.mark.parametrize("nnz", [257, 512, 2050])
def test_sparse_sums_of_all_p_minus_1(ctx, oracle, nnz):
    """the largest addends: every polynomial element and every value p - 1 (as limbs: the operands of a Montgomery product), a lane
    ending in every phase of a reduction group on a grid of one (1, 2 and 8 or 9 entries per lane)"""
    import pk_probes

    n = 12
    top = oracle.ints_to_limbs([K.P - 1] * (1 << n))
    f = [ctx.upload(top) for _ in range(4)]
    idx = np.arange(nnz, dtype=np.uint32) + 7
    from provekit_amd import whir_pcs

    sw = whir_pcs.SparseWeights([(idx, top[:nnz])] * 2).upload(ctx)
    want = oracle.ints_to_limbs([(K.P - 1) ** 2 * nnz * pow(1 << 256, -1, K.P) % K.P])[0]  # a sum of Montgomery products
    for grid in (0, 1):
        out = np.zeros((4, 2, 4), dtype=np.uint64)
        ctx._check(pk_probes.lib.pk_probe_whir_sparse_sums(ctx.handle, ptrs(f), 4, n, sw.offsets.ctypes.data, sw.d_index.ptr, sw.d_value.ptr, 2, grid,
                                                           out.ctypes.data))
        assert (out == want).all(), grid
    for x in f + [sw]:
        x.free()


def test_sparse_accumulate_against_python_ints(ctx, oracle):
    """all 16 weights on one position; all 16 full; a table of p - 1; scales 0, 1 and p - 1; positions no entry names keep their bits"""
    from provekit_amd import whir_pcs

    n = 8
    N = 1 << n
    scales = K.random_ints(16, 17)
    scales[3], scales[7], scales[15] = 0, 1, K.P - 1
    msc = L.mont(oracle, scales)
    cases = {
        "one position": ([([5], [K.random_ints(1, 60 + i)[0] if i else K.P - 1]) for i in range(16)], K.random_ints(N, 3)),
        "all full": ([(list(range(N)), K.random_ints(N, 100 + i)) for i in range(16)], [K.P - 1] * N),
        "mixed, on p - 1": (S.weights(n, 16), [K.P - 1] * N),
        "two weights": (S.weights(n, 2, seed=4), K.random_ints(N, 9)),
    }
    for name, (ws, before) in cases.items():
        l = len(ws)
        mbefore = L.mont(oracle, before)
        table = ctx.upload(mbefore)
        sw = S.pack(oracle, ws).upload(ctx)
        whir_pcs.sparse_accumulate(ctx, table, n, sw, msc[:l])
        got = ctx.download_fe(table.ptr, N)
        assert ints(oracle, got) == S.accumulate(before, ws, scales[:l]), name
        named = sorted({i for idx, _ in ws for i in idx})
        rest = np.setdiff1d(np.arange(N), np.array(named, dtype=np.int64))
        assert np.array_equal(got[rest], mbefore[rest]), name
        table.free()
        sw.free()
    table = ctx.upload(L.mont(oracle, before))
    whir_pcs.sparse_accumulate(ctx, table, n, whir_pcs.SparseWeights(), np.zeros((0, 4), dtype=np.uint64))  # l = 0
    whir_pcs.sparse_accumulate(ctx, table, n, S.pack(oracle, [([], []), ([], [])]), msc[:2])  # no entries, no lists
    assert np.array_equal(ctx.download_fe(table.ptr, N), L.mont(oracle, before))
    table.free()


def special_points(n, seed):
    rnd = K.random_ints(max(n, 1), seed)[:n]
    corner = [(0, 1, K.P - 1)[j % 3] for j in range(n)]
    bits = [(0x2D5A96B >> (j % 27)) & 1 for j in range(n)]
    return {"random": rnd, "0, 1 and -1": corner, "a vertex": bits}


@pytest.mark.parametrize("n", [1, 7, 8, 9, 13])
def test_sparse_evaluate_equals_the_dense_evaluation_and_python_ints(ctx, oracle, n):
    from provekit_amd import whir_pcs

    N = 1 << n
    ws = S.weights(n, 16, seed=50 + n)  # none, one at either end, full, shared, random lengths
    sw = S.pack(oracle, ws).upload(ctx)
    dense = [ctx.upload(L.mont(oracle, S.densify(n, w))) for w in ws]
    for name, point in special_points(n, 3 * n).items():
        mpt = L.mont(oracle, point)
        got = whir_pcs.sparse_evaluate(ctx, n, sw, mpt)
        assert ints(oracle, got) == S.evaluate(n, ws, point), (n, name)
        want = np.concatenate([whir_pcs.evaluate(ctx, dense[i : i + 4], n, mpt.reshape(1, n, 4))[:, 0] for i in range(0, 16, 4)])
        assert np.array_equal(got, want), (n, name)
    vertex = special_points(n, 0)["a vertex"]  # eq is an indicator there: the weight's value at that position
    at = int("".join(map(str, vertex)), 2)
    assert ints(oracle, whir_pcs.sparse_evaluate(ctx, n, sw, L.mont(oracle, vertex))) == [dict(zip(*w)).get(at, 0) for w in ws]
    assert N - 1 in ws[3][0] and ws[2][0] == [0]
    for x in dense + [sw]:
        x.free()


@pytest.mark.parametrize("n", [0, 17, 25, 30])
def test_sparse_evaluate_without_any_table_against_python_ints(ctx, oracle, n):
    """sizes at which no dense table is ever built: entries at 0, 2^n - 1 and on both sides of every chunk boundary bit, and one
    weight long enough for several steps per lane"""
    import pk_probes
    from provekit_amd import whir_pcs

    b = pk_probes.lib.pk_probe_whir_sparse_chunk_bits()
    N = 1 << n
    edge = sorted({0, N - 1} | {x for c in range(0, n + 1, b) for x in ((1 << c) - 1, 1 << c, (1 << c) + 1) if 0 <= x < N})
    rng = np.random.default_rng(n)
    long = sorted({int(x) for x in rng.integers(0, N, size=5000)}) if n else [0]
    ws = [(edge, K.random_ints(len(edge), 5 + n)), ([], []), (long, K.random_ints(len(long), 6 + n)), ([N - 1], [K.P - 1])]
    sw = S.pack(oracle, ws).upload(ctx)
    for name, point in special_points(n, 7 * n + 1).items():
        mpt = L.mont(oracle, point) if n else np.zeros((0, 4), dtype=np.uint64)
        assert ints(oracle, whir_pcs.sparse_evaluate(ctx, n, sw, mpt)) == S.evaluate(n, ws, point), (n, name)
    sw.free()


def bad_lists(oracle, n):
    """a well-formed pair of weights (250 and 20 entries: entries 255 and 256 of the concatenated lists, the two sides of the
    validation pass's first workgroup boundary, are entries 5 and 6 of weight 1) and the four ways to break the index rule"""
    from provekit_amd import whir_pcs

    good = S.pack(oracle, [(list(range(250)), K.random_ints(250, 1)), (list(range(10, 250, 12)), K.random_ints(20, 2))])

    def with_index(k, x):
        idx = good.index.copy()
        idx[k] = x
        return whir_pcs.SparseWeights(offsets=good.offsets, index=idx, value=good.value)

    return good, {
        "an index = 2^n_vars": (with_index(249, 1 << n), "weight 0, entry 249"),
        "an index = 2^32 - 1": (with_index(250, 0xFFFFFFFF), "weight 1, entry 0"),
        "an equal neighbouring pair": (with_index(101, 100), "weight 0, entry 101"),
        "a pair that decreases across a workgroup boundary": (with_index(256, int(good.index[255]) - 1), "weight 1, entry 6"),
    }


def test_lists_that_break_the_index_rule_are_refused_by_every_entry_point_and_nothing_is_left_broken(ctx, oracle):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError
    from provekit_amd.field import random_field

    n = 8
    N = 1 << n
    cfg = K.small_config(n, 2)
    polys = [random_field(N, 40 + b) for b in range(2)]
    f = [ctx.upload(p) for p in polys]
    scheme = whir_pcs.Scheme(ctx, cfg)
    com = scheme.commit(f)
    good, bad = bad_lists(oracle, n)
    good.upload(ctx)
    tags, point, scales = random_field(2, 8), random_field(n, 9), random_field(2, 10)
    before = random_field(N, 11)
    table = ctx.upload(before)
    first = scheme.open_sparse(com, None, good, tags)
    calls = {
        "pkw_sparse_sums": lambda w: whir_pcs.sparse_sums(ctx, f, n, w),
        "pkw_sparse_accumulate": lambda w: whir_pcs.sparse_accumulate(ctx, table, n, w, scales),
        "pkw_sparse_evaluate": lambda w: whir_pcs.sparse_evaluate(ctx, n, w, point),
        "pkw_open_sparse": lambda w: scheme.open_sparse(com, None, w, tags),
    }
    for name, (w, says) in bad.items():
        w.upload(ctx)
        for entry, call in calls.items():
            with pytest.raises(ProveKitHipError) as e:
                call(w)
            assert e.value.code == -1 and says in str(e.value) and NAMES_BOTH.search(str(e.value)), (name, entry, str(e.value))
        w.free()
    assert np.array_equal(ctx.download_fe(table.ptr, N), before)  # refused before any scatter
    # bad offsets are refused on the host
    for offsets, says in (([1, 250, 270], "offsets[0]"), ([0, 200, 100], "weight 1"), ([0, 257, 270], "weight 0")):
        w = whir_pcs.SparseWeights(offsets=np.array(offsets, dtype=np.uint64), index=good.index, value=good.value)
        w.d_index, w.d_value = good.d_index, good.d_value
        for entry, call in calls.items():
            with pytest.raises(ProveKitHipError) as e:
                call(w)
            assert e.value.code == -1 and says in str(e.value), (offsets, entry, str(e.value))
        w.d_index = w.d_value = None
    # the context, the scheme and the commitment are as usable as before: the right bits right after
    again = scheme.open_sparse(com, None, good, tags)
    assert again[2] == first[2] and np.array_equal(again[1], first[1])
    assert whir_pcs.verify_sparse(cfg, None, tags, good, again[2], expected_root=com.root()).result.accepted
    dense = np.zeros((2, N, 4), dtype=np.uint64)
    for i in range(2):
        lo, hi = int(good.offsets[i]), int(good.offsets[i + 1])
        dense[i][good.index[lo:hi]] = good.value[lo:hi]
    d_w = [ctx.upload(t) for t in dense]
    assert np.array_equal(whir_pcs.sparse_sums(ctx, f, n, good), whir_pcs.weighted_sums(ctx, f, n, d_w))
    assert np.array_equal(whir_pcs.sparse_evaluate(ctx, n, good, point), whir_pcs.evaluate(ctx, d_w, n, point.reshape(1, n, 4))[:, 0])
    for x in f + d_w + [table, good, com, scheme]:
        (x.free if hasattr(x, "free") else x.close)()


def proof_weights(n, l):
    """the weight set of the whole-proof tests: whir_pcs_sparse_cases.weights where l is large enough to hold every kind; for
    smaller l: no entry, one entry, every position, and the same positions again"""
    if l >= 6 or l < 4:
        return S.weights(n, l)
    N = 1 << n
    return [([], []), ([N // 3], [K.P - 1]), (list(range(N)), K.random_ints(N, 71)), (list(range(N)), K.random_ints(N, 72))][:l]


@pytest.mark.parametrize("shape", L.SHAPES + [(16, 2, 1, 4)])
def test_open_sparse_writes_the_bytes_of_open_linear_on_the_densified_tables(ctx, oracle, shape):
    from provekit_amd import whir_pcs

    n, batch, q, l = shape
    cfg = K.small_config(n, batch)
    polys, pts = K.polynomials(n, batch), (K.points(n, q) if q else [])
    ws, tags = proof_weights(n, l), L.tags(l)
    mpts = K.mont_points(oracle, pts) if q else None
    mtags = L.mont(oracle, tags)
    mdense = [L.mont(oracle, S.densify(n, w)) for w in ws]
    scheme = whir_pcs.Scheme(ctx, cfg)
    f = [ctx.upload(L.mont(oracle, p)) for p in polys]
    com = scheme.commit(f)
    d_w = [ctx.upload(w) for w in mdense]
    sw = S.pack(oracle, ws).upload(ctx)
    want = scheme.open_linear(com, mpts, d_w, mtags)
    got = scheme.open_sparse(com, mpts, sw, mtags)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(got[2]) == len(want[2]) and got[2] == want[2]
    assert ints(oracle, got[1]) == [s for row in S.sums(polys, ws) for s in row]
    v = whir_pcs.verify_sparse(cfg, mpts, mtags, sw, got[2], expected_root=com.root())
    assert v.result.accepted and v.result.offset == len(got[2]) and np.array_equal(v.sums, got[1]), v.result
    d = whir_pcs.verify_linear(cfg, mpts, mtags, mdense, got[2], expected_root=com.root())
    assert d.result.accepted and d.unchecked == 0 and np.array_equal(d.deferred, v.deferred), d.result
    assert scheme.open_sparse(com, mpts, sw, mtags)[2] == got[2]  # a second opening over the same arena
    if shape == (8, 2, 2, 3):  # ... and they are the oracle prover's bytes, those the CPU suite verifies
        ref, root, _, _ = L.oracle_linear_opening(oracle, cfg, polys, pts, [S.densify(n, w) for w in S.weights(n, l)], tags,
                                                  whir_pcs.io_pattern_linear(cfg, q, l))
        assert root == com.root() and got[2] == ref
    for x in f + d_w + [sw, com, scheme]:
        (x.free if hasattr(x, "free") else x.close)()


def test_cpp_host_opens_sparse_weights_verifies_and_sees_a_tampered_entry_rejected():
    assert os.path.exists(DEMO), "examples/pcs_sparse_demo is built by __graft_entry__.build()"
    out = subprocess.run([DEMO, "12", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n_vars=12 points=1 weights=3 entries=")
    assert "rejected, check=DEFERRED" in lines[1] and "weight 1" in lines[1]
