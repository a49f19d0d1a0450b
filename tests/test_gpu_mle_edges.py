"""GPU: the MLE / sumcheck kernels (csrc/mle.hip, csrc/reduce.hpp) at their reduction and size edges, bit-exact.

test_gpu_mle.py is the parity suite on uniformly random inputs in plain mode.  This file goes where that one does not: both grid
rules of the reduction (plain and latency mode) on both sides of each of their boundaries, the entry points that have no C ABI
(through tools/probes: sumcheck_cubic_launch with the eq array as the weight, sumcheck_quadratic_launch), Horner above 2^21 coefficients, the largest addends the accumulating kernels can be given, challenges
0, 1 and -1, and to_coeffs / to_evals compared at every index up to 22 variables.  References are Python-int definitions and closed
forms (tests/mle_edge_refs.py, checked on the CPU by test_mle_edge_refs_host.py); the C oracle where the size needs it."""
import ctypes as C
import functools

import numpy as np
import pytest

import mle_edge_refs as E

pytestmark = pytest.mark.gpu
P = E.P
N_MAX = 1 << 20  # no geometry case needs more elements per array
HORNER_MAX = (1 << 21) + 12345  # 916 workgroups of 9 x 256 coefficients: a capped grid, a partly filled last workgroup, base bits 20 and 21


def L(v):
    return E.limbs([v])[0]


@functools.lru_cache(maxsize=None)
def host_pool():
    """four random arrays of N_MAX elements (a, b, c, eq -- or w, f, g) and three weight rows of N_MAX elements each"""
    from provekit_amd.field import random_field

    return [random_field(N_MAX, 900 + k) for k in range(4)], random_field(3 * N_MAX, 950)


@pytest.fixture(scope="module")
def pool(ctx):
    arrs, rows = host_pool()
    dev = [ctx.upload(a) for a in arrs], ctx.upload(rows)
    yield dev
    for b in dev[0] + [dev[1]]:
        b.free()


@pytest.fixture(scope="module")
def consts(ctx):
    """constant arrays: p - 1, the field's one and two; weight rows p - 1, p - 3, p - 5 (N_MAX elements each)"""
    host = [E.const(N_MAX, v) for v in (E.TOP, E.ONE, 2 * E.ONE % P)]
    rows = np.concatenate([E.const(N_MAX, P - 1 - 2 * k) for k in range(3)])
    dev = [ctx.upload(h) for h in host], ctx.upload(rows)
    yield dev
    for b in dev[0] + [dev[1]]:
        b.free()


# ---- thin callers ---------------------------------------------------------------------------------------------------------------------
def num_cus(ctx):
    from tools.pk_probes import lib as probes

    n = C.c_int()
    ctx._check(probes.pk_probe_num_cus(ctx.handle, C.byref(n)))
    return n.value


def grid_of(ctx, items):
    from tools.pk_probes import lib as probes

    b = C.c_uint()
    ctx._check(probes.pk_probe_reduction_blocks(ctx.handle, items, C.byref(b)))
    return b.value


def dot(ctx, w, f, n):
    from provekit_amd._lib import lib

    out = np.full(4, 0xA5, dtype=np.uint64)
    ctx._check(lib.pk_dot(ctx.handle, w, f, n, out.ctypes.data))
    return E.ints(out)[0]


def dot2(ctx, w, f, g, n):
    from provekit_amd._lib import lib

    out = np.full((2, 4), 0xA5, dtype=np.uint64)
    ctx._check(lib.pk_dot2(ctx.handle, w, f, g, n, out.ctypes.data))
    return E.ints(out)


def dot_rows(ctx, w, stride, f, g, n):
    """-> [[<w_k, f>, <w_k, g>] for the three rows]  (one column without g)"""
    from tools.pk_probes import lib as probes

    nv = 2 if g is not None else 1
    out = np.full((3 * nv, 4), 0xA5, dtype=np.uint64)
    ctx._check(probes.pk_probe_dot_rows(ctx.handle, w, stride, 3, f, g, n, out.ctypes.data))
    v = E.ints(out)
    return [v[nv * k: nv * k + nv] for k in range(3)]


def cubic(ctx, d, length, fold=None):
    from provekit_amd import sumcheck as sc

    return E.ints(sc.sumcheck_fold_map_reduce(ctx, *d, length, None if fold is None else L(fold)))


def quadratic(ctx, f, w, length, fold=None, fo=None, wo=None):
    from provekit_amd import sumcheck as sc

    return E.ints(sc.sumcheck_quadratic_round(ctx, f, w, length, None if fold is None else L(fold), fo, wo))


def set_mode(ctx, latency):
    ctx.set_latency_mode(latency)


# ---- reduction geometry ----------------------------------------------------------------------------------------------------------------
DOT_CASES = [(lat, n) for lat in (False, True) for n in E.geometry_items(lat)]
# non-folding rounds take the powers of two on each side: (latency, elements, workgroups of the lane-per-pair kernels)
ROUND_CASES = [(False, 1 << 11, 1), (False, 1 << 12, 2), (False, 1 << 19, 256), (False, 1 << 20, 512),
               (True, 1 << 9, 1), (True, 1 << 10, 2), (True, 1 << 17, 256), (True, 1 << 18, 512), (True, 1 << 19, 1024), (True, 1 << 20, 1024),
               # the quadratic round's four-lanes-per-pair kernel (up to 16384 pairs) has a grid of its own: 64 pairs per workgroup
               (False, 1 << 7, 1), (False, 1 << 8, 2)]


def test_the_grid_rule_is_the_one_the_cases_rest_on(ctx):
    """reduce.hpp reduction_blocks: ceil(items / (256 * items per thread)) workgroups, 4 items per thread (1 in latency mode), at most
    4 per compute unit and at most 1024.  The cases below straddle the boundaries of a 1024-workgroup cap: a part with fewer than 256
    compute units needs another look at them."""
    cus = num_cus(ctx)
    assert min(4 * cus, E.RED_MAX_BLOCKS) == 1024
    try:
        for latency in (False, True):
            set_mode(ctx, latency)
            for items, blocks in E.geometry_items(latency).items():
                assert grid_of(ctx, items) == blocks == E.reduction_blocks(items, latency, cus), (latency, items)
            for lat, length, blocks in ROUND_CASES:
                if lat == latency and length > 1 << 8:
                    assert grid_of(ctx, length // 2) == blocks, (latency, length)
    finally:
        set_mode(ctx, False)


@functools.lru_cache(maxsize=None)
def random_dot_refs(n):
    import oracle_lib as oracle

    (w, f, g, _), rows = host_pool()
    r = [rows[k * N_MAX: k * N_MAX + n] for k in range(3)]
    return (E.ints(oracle.dot(w[:n], f[:n]))[0], E.ints(oracle.dot(w[:n], g[:n]))[0],
            [[E.ints(oracle.dot(r[k], f[:n]))[0], E.ints(oracle.dot(r[k], g[:n]))[0]] for k in range(3)])


@functools.lru_cache(maxsize=None)
def random_round_refs(length):
    import oracle_lib as oracle

    a, b, c, eq = (x[:length] for x in host_pool()[0])
    return E.ints(oracle.sumcheck_cubic_round(a, b, c, eq)[0]), E.ints(oracle.sumcheck_quadratic_round(a, b)[0])


@pytest.mark.parametrize("latency,n", DOT_CASES)
def test_dot_family_on_both_sides_of_each_grid_boundary(ctx, pool, latency, n):
    (w, f, g, _), rows = pool
    wf, wg, by_row = random_dot_refs(n)
    try:
        set_mode(ctx, latency)
        assert grid_of(ctx, n) == E.geometry_items(latency)[n]
        assert dot(ctx, w.ptr, f.ptr, n) == wf
        assert dot2(ctx, w.ptr, f.ptr, g.ptr, n) == [wf, wg]
        assert dot_rows(ctx, rows.ptr, N_MAX, f.ptr, g.ptr, n) == by_row
        assert dot_rows(ctx, rows.ptr, N_MAX, f.ptr, None, n) == [r[:1] for r in by_row]
    finally:
        set_mode(ctx, False)


@pytest.mark.parametrize("latency,n", DOT_CASES)
def test_dot_family_with_the_largest_addends(ctx, consts, latency, n):
    """w = p - 1 and f = the field's one: every product is the stored value p - 1, the sum is (p - n) mod p; g = two makes the second
    output (p - 2n) mod p and rows p - 1, p - 3, p - 5 give the six outputs of dot_rows -n, -2n, -3n, -6n, -5n, -10n: a swapped row or
    f read for g cannot go unseen"""
    (top, one, two), rows = consts
    want = [[E.dot_of_constants(n, P - 1 - 2 * k, E.ONE), E.dot_of_constants(n, P - 1 - 2 * k, 2 * E.ONE % P)] for k in range(3)]
    assert want[0] == [(P - n) % P, (P - 2 * n) % P] and len({v for r in want for v in r}) == 6
    try:
        set_mode(ctx, latency)
        assert dot(ctx, top.ptr, one.ptr, n) == want[0][0]
        assert dot2(ctx, top.ptr, one.ptr, two.ptr, n) == want[0]
        assert dot2(ctx, top.ptr, two.ptr, one.ptr, n) == want[0][::-1]
        assert dot_rows(ctx, rows.ptr, N_MAX, one.ptr, two.ptr, n) == want
        assert dot_rows(ctx, rows.ptr, N_MAX, two.ptr, None, n) == [r[1:] for r in want]
    finally:
        set_mode(ctx, False)


@pytest.mark.parametrize("latency,length,blocks", ROUND_CASES)
def test_rounds_on_both_sides_of_each_grid_boundary(ctx, pool, latency, length, blocks):
    d = [b.ptr for b in pool[0]]
    want_cubic, want_quadratic = random_round_refs(length)
    try:
        set_mode(ctx, latency)
        assert cubic(ctx, d, length) == want_cubic
        assert quadratic(ctx, d[0], d[1], length) == want_quadratic
    finally:
        set_mode(ctx, False)


# lower / upper half of the cubic round's arrays, even / odd elements of the quadratic round's: the first sum's addends are all p - 1
CUBIC_HALVES = dict(a=(E.TOP, P - 2), b=(E.ONE, 2 * E.ONE % P), c=(0, E.TOP), eq=(E.ONE, E.MINUS_ONE))
QUADRATIC_PAIR = dict(f=(E.TOP, P - 2), w=(E.ONE, E.MINUS_ONE))


@pytest.mark.parametrize("latency,length,blocks", ROUND_CASES)
def test_rounds_with_the_largest_addends(ctx, latency, length, blocks):
    """arrays constant on each half (cubic: the partner of i is i + len/2) resp. alternating (quadratic: adjacent pairs): every pair
    adds the same three terms, so each sum is pairs * term -- with p - 1 the term of the first sum"""
    pairs = length // 2
    h = CUBIC_HALVES
    terms = E.cubic_map(h["a"][0], h["a"][1], h["b"][0], h["b"][1], h["c"][0], h["c"][1], h["eq"][0], h["eq"][1])
    assert terms[0] == P - 1 and len(set(terms)) == 3 and 0 not in terms
    d = [ctx.upload(np.concatenate([E.const(pairs, lo), E.const(pairs, hi)])) for lo, hi in h.values()]
    q = QUADRATIC_PAIR
    qterms = E.quadratic_map(q["f"][0], q["f"][1], q["w"][0], q["w"][1])
    assert qterms[0] == P - 1 and len(set(qterms)) == 3 and 0 not in qterms
    df, dw = (ctx.upload(E.periodic(length, pair)) for pair in q.values())
    try:
        set_mode(ctx, latency)
        assert cubic(ctx, [b.ptr for b in d], length) == [pairs * t % P for t in terms]
        assert quadratic(ctx, df.ptr, dw.ptr, length) == [pairs * t % P for t in qterms]
    finally:
        set_mode(ctx, False)
        for b in d + [df, dw]:
            b.free()


@pytest.mark.parametrize("latency", [False, True])
def test_the_ticket_is_rearmed_without_a_stream_sync_in_between(ctx, pool, latency):
    """launch, take the sums from the pinned page by their sequence number (no stream synchronisation), launch again: the workgroup
    that drew the last ticket of the first launch must have put the ticket back"""
    from tools.pk_probes import lib as probes

    d = [b.ptr for b in pool[0]]
    got = []
    try:
        set_mode(ctx, latency)
        for kind, length in (("cubic", 1 << 14), ("quadratic", 1 << 17), ("cubic", 1 << 13), ("cubic", 1 << 14)):
            assert grid_of(ctx, length // 2) > 1
            seq, out = C.c_uint(0), np.full((3, 4), 0xA5, dtype=np.uint64)
            if kind == "cubic":
                ctx._check(probes.pk_probe_sumcheck_cubic_launch(ctx.handle, *d, length, None, C.byref(seq)))
            else:
                ctx._check(probes.pk_probe_sumcheck_quadratic_launch(ctx.handle, d[0], d[1], length, None, None, None, C.byref(seq)))
            assert seq.value != 0
            ctx._check(probes.pk_probe_sumcheck_collect_spin(ctx.handle, seq.value, out.ctypes.data))
            got.append((kind, length, E.ints(out)))
        ctx.sync()
    finally:
        set_mode(ctx, False)
    for kind, length, sums in got:
        assert sums == random_round_refs(length)[0 if kind == "cubic" else 1], (kind, length)


# ---- entry points without a C ABI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_dot_rows(ctx, oracle, n):
    """three distinct rows against f and g, row_stride == n and > n, with and without g: six dot products, each on its own"""
    from provekit_amd.field import random_field

    f, g = random_field(max(n, 1), 11 + n)[:n], random_field(max(n, 1), 12 + n)[:n]
    df, dg = ctx.upload(f if n else np.zeros((1, 4), np.uint64)), ctx.upload(g if n else np.zeros((1, 4), np.uint64))
    for stride in (n, n + 37):
        w = random_field(max(3 * stride, 1), 13 + stride)
        dw = ctx.upload(w)
        rows = [w[k * stride: k * stride + n] for k in range(3)]
        if n <= 257:
            ip = lambda x, y: sum(E.mul(u, v) for u, v in zip(E.ints(x), E.ints(y))) % P
        else:
            ip = lambda x, y: E.ints(oracle.dot(x, y))[0]
        want = [[ip(r, f), ip(r, g)] for r in rows]
        if n:
            assert len({v for r in want for v in r}) == 6
        assert dot_rows(ctx, dw.ptr, stride, df.ptr, dg.ptr, n) == want, (n, stride)
        assert dot_rows(ctx, dw.ptr, stride, df.ptr, None, n) == [r[:1] for r in want], (n, stride)
        assert dot_rows(ctx, dw.ptr, stride, dg.ptr, None, n) == [r[1:] for r in want], (n, stride)
        dw.free()
    df.free()
    dg.free()


@functools.lru_cache(maxsize=None)
def horner_polys():
    from provekit_amd.field import random_field

    return random_field(HORNER_MAX, 700), random_field(HORNER_MAX, 701)


@pytest.fixture(scope="module")
def horner_dev(ctx):
    dev = [ctx.upload(p) for p in horner_polys()]
    yield dev
    for b in dev:
        b.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, 70000, HORNER_MAX])
def test_eval_univariate_multi(ctx, oracle, horner_dev, n):
    """two polynomials at one point in one launch == two single evaluations == the definition; at z = 0, 1 and -1 the definition is
    c[0], the sum and the alternating sum of the coefficients, at every size"""
    from provekit_amd import sumcheck as sc
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    polys = [p[:n] for p in horner_polys()]
    closed = [E.horner_closed_forms(p) for p in polys]
    ptrs = (C.c_void_p * 2)(horner_dev[0].ptr, horner_dev[1].ptr)
    zs = dict(E.CHALLENGES, random=E.ints(random_field(1, 1234 + n))[0])
    for name, z in zs.items():
        if name in closed[0]:
            want = [c[name] for c in closed]
        elif n <= 2049:
            want = [E.horner(E.ints(p), z) for p in polys]
        else:
            want = [E.ints(oracle.eval_univariate(p, L(z)))[0] for p in polys]
        out, zl = np.full((2, 4), 0xA5, dtype=np.uint64), L(z)
        ctx._check(probes.pk_probe_eval_univariate_multi(ctx.handle, ptrs, 2, n, zl.ctypes.data, out.ctypes.data))
        assert E.ints(out) == want, (n, name)
        assert want[0] != want[1]
        single = [E.ints(sc.eval_univariate(ctx, d, n, L(z)))[0] for d in horner_dev]
        assert single == want, (n, name)


@pytest.mark.parametrize("n", [1, 257, 5001])
def test_lincomb2(ctx, n):
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    a, b = random_field(n, 21 + n), random_field(n, 22 + n)
    a[0], b[0] = L(E.TOP), L(E.TOP)
    da, db, do = ctx.upload(a), ctx.upload(b), ctx.alloc_fe(n)
    for name, beta in dict(E.CHALLENGES, random=E.ints(random_field(1, 23))[0]).items():
        ctx.zero(do, 32 * n)
        bl = L(beta)
        ctx._check(probes.pk_probe_lincomb2(ctx.handle, do.ptr, da.ptr, bl.ctypes.data, db.ptr, n))
        assert np.array_equal(ctx.download_fe(do, n), E.axpy(a, beta, b)), (n, name)
    assert np.array_equal(ctx.download_fe(da, n), a) and np.array_equal(ctx.download_fe(db, n), b)  # sources untouched
    for x in (da, db, do):
        x.free()


@pytest.mark.parametrize("length", [2, 4, 512, 1 << 13])
def test_fold_pairs2(ctx, length):
    """two arrays folded by one challenge in one launch: each output == the single-array fold == v[2i] + r (v[2i+1] - v[2i])"""
    from provekit_amd import sumcheck as sc
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    v = [random_field(length, 31 + length), random_field(length, 32 + length)]
    v[0][:2] = E.limbs([E.TOP, 0])
    dv = [ctx.upload(x) for x in v]
    out, single = [ctx.alloc_fe(length // 2) for _ in range(2)], ctx.alloc_fe(length // 2)
    for name, r in dict(E.CHALLENGES, random=E.ints(random_field(1, 33))[0]).items():
        for o in out:
            ctx.zero(o, 16 * length)
        rl = L(r)
        ctx._check(probes.pk_probe_fold_pairs2(ctx.handle, dv[0].ptr, out[0].ptr, dv[1].ptr, out[1].ptr, length, rl.ctypes.data))
        for k in range(2):
            got = ctx.download_fe(out[k], length // 2)
            assert np.array_equal(got, E.fold_pairs(v[k], r)), (length, name, k)
            sc.fold_pairs(ctx, dv[k], length, L(r), single)
            assert np.array_equal(got, ctx.download_fe(single, length // 2)), (length, name, k)
        assert not np.array_equal(ctx.download_fe(out[0], length // 2), ctx.download_fe(out[1], length // 2))
    for k in range(2):
        assert np.array_equal(ctx.download_fe(dv[k], length), v[k])  # inputs untouched
    for x in dv + out + [single]:
        x.free()


# ---- structured values through the accumulating kernels --------------------------------------------------------------------------------
def family(oracle, name, n, seed):
    """four arrays of n elements: "top" every element p - 1; "equal" one value per array; "alternating" 0 and p - 1 (b and eq start
    with p - 1); "hadamard" a o b = c from short periodic patterns, so the f(0) addends are exactly zero"""
    from provekit_amd.field import random_field

    if name == "top":
        return [E.const(n, E.TOP) for _ in range(4)]
    if name == "equal":
        return [E.const(n, v) for v in E.ints(random_field(4, seed))]
    if name == "alternating":
        return [E.periodic(n, pat) for pat in ((0, E.TOP), (E.TOP, 0), (0, E.TOP), (E.TOP, 0))]
    pools = E.ints(random_field(15, seed))
    a, b, eq = E.periodic(n, pools[:5]), E.periodic(n, pools[5:12]), E.periodic(n, pools[12:])
    return [a, b, oracle.hadamard(a, b), eq]


FAMILIES = ["top", "equal", "alternating", "hadamard"]


@pytest.mark.parametrize("log_len", [1, 2, 16, 17])  # folding: 2^14 pairs is the last size of the eight-lanes-per-pair kernel
@pytest.mark.parametrize("name", FAMILIES)
def test_cubic_round_on_structured_values(ctx, oracle, name, log_len):
    n = 1 << log_len
    arrs = family(oracle, name, n, 50 + log_len)
    for challenge, r in dict(E.CHALLENGES, none=None).items():
        if r is not None and n < 4:
            continue
        d = [ctx.upload(x) for x in arrs]
        want, folded = E.cubic_round(*arrs, r)
        assert cubic(ctx, [b.ptr for b in d], n, r) == want, (name, log_len, challenge)
        if name == "equal":
            assert want[2] == 0  # every difference vanishes
        if name == "hadamard" and challenge in ("none", "zero", "one"):
            assert want[0] == 0  # a o b - c stays zero where folding picks one of the two halves
        if r is not None:
            for k in range(4):
                assert np.array_equal(ctx.download_fe(d[k], n // 2), folded[k]), (name, log_len, challenge, k)
                assert np.array_equal(ctx.download_fe(d[k].view_fe(n // 2), n // 2), arrs[k][n // 2:])  # the upper half is only read
            if name == "equal":
                assert all(np.array_equal(folded[k], arrs[k][: n // 2]) for k in range(4))
        for b in d:
            b.free()


@pytest.mark.parametrize("log_len", [1, 2, 16, 17])  # folding: 2^14 pairs is the last size of the four-lanes-per-pair kernel
@pytest.mark.parametrize("name", FAMILIES)
def test_quadratic_round_on_structured_values(ctx, oracle, name, log_len):
    n = 1 << log_len
    arrs = family(oracle, name, n, 60 + log_len)
    f, w = (arrs[0], arrs[1]) if name != "hadamard" else (arrs[2], arrs[3])
    df, dw, fo, wo = ctx.upload(f), ctx.upload(w), ctx.alloc_fe(n), ctx.alloc_fe(n)
    for challenge, r in dict(E.CHALLENGES, none=None).items():
        if r is not None and n < 4:
            continue
        want, folded = E.quadratic_round(f, w, r)
        if r is None:
            assert quadratic(ctx, df.ptr, dw.ptr, n) == want, (name, log_len)
            continue
        ctx.zero(fo, 32 * n)
        ctx.zero(wo, 32 * n)
        assert quadratic(ctx, df.ptr, dw.ptr, n, r, fo.ptr, wo.ptr) == want, (name, log_len, challenge)
        assert np.array_equal(ctx.download_fe(fo, n // 2), folded[0]) and np.array_equal(ctx.download_fe(wo, n // 2), folded[1])
        if name == "equal":  # f' = f, w' = w, and h(2) = h(0) = h(1)
            assert np.array_equal(folded[0], f[: n // 2]) and want[0] == want[1] == want[2]
    assert np.array_equal(ctx.download_fe(df, n), f) and np.array_equal(ctx.download_fe(dw, n), w)
    for b in (df, dw, fo, wo):
        b.free()


@pytest.mark.parametrize("n_vars,k", [(17, 4), (18, 4), (10, 0), (10, 1), (10, 8)])  # k = 4: 8192 outputs is the last size of the 16-lane kernel
def test_fold_coeffs_on_structured_values(ctx, n_vars, k):
    """with every r_b the field's one all weights are one: c = p - 1 then gives the 16-lane limb sums sixteen addends of p - 1"""
    from provekit_amd import sumcheck as sc
    from provekit_amd.field import random_field

    n = 1 << n_vars
    pool9 = E.ints(random_field(9, 70 + n_vars))
    inputs = {"top": E.const(n, E.TOP), "equal": E.const(n, pool9[0]), "alternating": E.periodic(n, (0, E.TOP)), "periodic": E.periodic(n, pool9)}
    mixed = [0, E.ONE, E.MINUS_ONE, E.TOP, pool9[1], E.ONE, 0, E.MINUS_ONE]
    challenges = dict({name: [v] * 8 for name, v in E.CHALLENGES.items()}, mixed=mixed)
    out = ctx.alloc_fe(n >> k)
    for name, c in inputs.items():
        d = ctx.upload(c)
        for cname, rs in challenges.items():
            rs = rs[:k]
            ctx.zero(out, 32 * (n >> k))
            sc.fold_coeffs(ctx, d, n_vars, E.limbs(rs) if k else np.zeros((0, 4), np.uint64), out)
            assert np.array_equal(ctx.download_fe(out, n >> k), E.fold_coeffs(c, k, rs)), (n_vars, k, name, cname)
        assert np.array_equal(ctx.download_fe(d, n), c)
        d.free()
    assert E.ints(E.fold_coeffs(inputs["top"][: 1 << k], k, [E.ONE] * k)) == [(P - (1 << k)) % P]
    out.free()


def indicator_point(n_vars, idx):
    """the point of {0, 1}^n whose eq table is one at idx and zero elsewhere: variable 0 is the most significant index bit"""
    return [E.ONE if idx >> (n_vars - 1 - j) & 1 else 0 for j in range(n_vars)]


@pytest.mark.parametrize("n_vars", [5, 6])
@pytest.mark.parametrize("q", [1, 4, 5, 8])
def test_eq_accumulate_on_structured_points(ctx, n_vars, q):
    """points of {0, 1}^n: eq_accumulate adds the scale at one index and leaves every other element bit-unchanged -- q times p - 1 on
    one element fills a dot29 group with the largest products; then coordinates 0, 1, -1 and p - 1 against the definition"""
    import random

    from provekit_amd import sumcheck as sc

    N = 1 << n_vars
    rnd = random.Random(100 * n_vars + q)
    spread = [0, N - 1, 5, 5, 5, 5, 17, N - 1][:q]
    base = [E.TOP if i % 3 else rnd.randrange(P) for i in range(N)]
    for label, idxs, scales in (("one index", [N - 1] * q, [E.TOP] * q), ("spread", spread, [E.TOP - t for t in range(q)])):
        pts = [indicator_point(n_vars, i) for i in idxs]
        for overwrite in (False, True):
            want = [0] * N if overwrite else list(base)
            for i, s in zip(idxs, scales):
                want[i] = (want[i] + s) % P
            assert want == E.eq_accumulate(base, pts, scales, overwrite)
            d = ctx.upload(E.limbs(base))
            sc.eq_accumulate(ctx, d, n_vars, np.stack([E.limbs(p) for p in pts]), E.limbs(scales), overwrite=overwrite)
            assert E.ints(ctx.download_fe(d, N)) == want, (label, n_vars, q, overwrite)
            d.free()
    coords = [0, E.ONE, E.MINUS_ONE, E.TOP]
    pts = [[coords[(t + 3 * j) % 4] if (t + j) % 3 else rnd.randrange(P) for j in range(n_vars)] for t in range(q)]
    scales = [coords[(t + 1) % 4] if t % 2 else rnd.randrange(P) for t in range(q)]
    d = ctx.upload(E.limbs(base))
    sc.eq_accumulate(ctx, d, n_vars, np.stack([E.limbs(p) for p in pts]), E.limbs(scales))
    assert E.ints(ctx.download_fe(d, N)) == E.eq_accumulate(base, pts, scales)
    d.free()


def test_axpy_on_structured_values(ctx):
    from provekit_amd import sumcheck as sc
    from provekit_amd.field import random_field

    n = 1000
    pool = E.ints(random_field(7, 80))
    for yname, y in (("top", E.const(n, E.TOP)), ("alternating", E.periodic(n, (0, E.TOP))), ("periodic", E.periodic(n, pool))):
        for xname, x in (("top", E.const(n, E.TOP)), ("one", E.const(n, E.ONE)), ("alternating", E.periodic(n, (E.TOP, 0, E.MINUS_ONE)))):
            dx = ctx.upload(x)
            for bname, beta in E.CHALLENGES.items():
                dy = ctx.upload(y)
                sc.axpy(ctx, dy, L(beta), dx, n)
                assert np.array_equal(ctx.download_fe(dy, n), E.axpy(y, beta, x)), (yname, xname, bname)
                dy.free()
            assert np.array_equal(ctx.download_fe(dx, n), x)
            dx.free()


# ---- to_coeffs / to_evals at every index -----------------------------------------------------------------------------------------------
def product_tables(oracle, n_vars):
    """f[i] = prod_j (bit_j(i) ? x_j : 1) and its coefficients prod_j (x_j - 1)^bit_j(i), built with the oracle's vector operations"""
    from provekit_amd.field import random_field

    xs = random_field(n_vars, 300 + n_vars)
    xs[3], xs[n_vars - 2], xs[12] = L(0), L(E.MINUS_ONE), L(E.TOP)
    one = E.limbs([E.ONE])
    table, coeffs = one, one
    for x in xs:
        xm = oracle.binop("pko_fe_sub", x, one[0])[0]
        table = np.concatenate([table, oracle.vec_axpy(np.zeros_like(table), x, table)])
        coeffs = np.concatenate([coeffs, oracle.vec_axpy(np.zeros_like(coeffs), xm, coeffs)])
    return table, coeffs


@pytest.mark.parametrize("kind", ["ones", "product"])
@pytest.mark.parametrize("n_vars", [16, 21, 22])  # 22: a second high sweep (11 + 9 + 2 index bits)
def test_to_coeffs_at_every_index(ctx, oracle, n_vars, kind):
    from provekit_amd import sumcheck as sc
    from provekit_amd._lib import lib

    n = 1 << n_vars
    if kind == "ones":  # the constant polynomial 1
        table = E.const(n, E.ONE)
        coeffs = np.zeros((n, 4), dtype=np.uint64)
        coeffs[0] = L(E.ONE)
    else:
        table, coeffs = product_tables(oracle, n_vars)
    d, src, dst = ctx.upload(table), ctx.upload(table), ctx.alloc_fe(n)
    sc.to_coeffs(ctx, d, n_vars)
    assert np.array_equal(ctx.download_fe(d, n), coeffs)
    sc.to_evals(ctx, d, n_vars)
    assert np.array_equal(ctx.download_fe(d, n), table)  # round trip
    ctx._check(lib.pk_to_coeffs_into(ctx.handle, src.ptr, dst.ptr, n_vars))
    assert np.array_equal(ctx.download_fe(dst, n), coeffs)
    assert np.array_equal(ctx.download_fe(src, n), table)  # source untouched
    ctx._check(lib.pk_to_evals_into(ctx.handle, dst.ptr, d.ptr, n_vars))
    assert np.array_equal(ctx.download_fe(d, n), table)
    for b in (d, src, dst):
        b.free()
