"""GPU: the sumcheck routes that leave out redundant work, bit-exact against the routes they replace.  In csrc/mle.hip the two cubic
routes are the two weight policies of one round body (cubic_round_wide, and cubic_round_small for few pairs): CubicWeight::Level
against CubicWeight::EqArray, both behind sumcheck_cubic_launch; the two- and three-sum quadratic routes are the NS of one kernel.

  * suffix equality tables: every level E_i = eq(r[i+1 .. n), .) against oracle/pyref.py's eq table;
  * the cubic round without the eq array (a, b, c folded, one level entry per pair, three host scalars) against
    pk_sumcheck_cubic_round on an explicit eq array, through all m_0 rounds with the same challenges;
  * the quadratic round that forms h(0) and h(2) and takes h(1) from the claim against pk_sumcheck_quadratic_round;
  * whole proofs against oracle/prover_ref.py, plain and latency mode.

Field arithmetic is exact and every value is fully reduced, so "equal" is equality of the 32 bytes."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import mle_edge_refs as E  # noqa: E402
import pyref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
P = E.P
HALF = pow(2, -1, P) * E.R % P  # stored 1/2
SMALL_ROUND_PAIRS = 16384  # mle.hip (sumcheck_cubic_launch, sumcheck_quadratic_launch): up to this many pairs a folding cubic round (any quadratic round) spreads a pair over several lanes


def rnd(n, seed):
    from provekit_amd.field import random_field

    return random_field(n, seed)


def suffix_tables(ctx, r, n):
    from provekit_amd._lib import lib

    d = ctx.alloc_fe(1 << n)
    ctx._check(lib.pk_selftest_eq_suffix_tables(ctx.handle, np.ascontiguousarray(r).ctypes.data, n, d.ptr))
    return d


# 11 | 12 is the boundary of the build (mle.hip EQ_SUFFIX_ONE_WG_VARS = 11): up to 11 variables one workgroup builds every level, from
# 12 on two workgroups build the short levels and the factor tables and a grid-wide kernel expands the long levels
@pytest.mark.parametrize("n", [1, 2, 9, 10, 11, 12, 13])
def test_every_suffix_level_is_the_eq_table_of_the_remaining_variables(ctx, n):
    r = rnd(n, 400 + n)
    r_canon = [x * E.R_INV % P for x in E.ints(r)]
    d = suffix_tables(ctx, r, n)
    got = E.ints(ctx.download_fe(d, 1 << n))
    d.free()
    N = 1 << n
    for i in range(n):
        off, size = N - (N >> i), N >> (i + 1)
        want = [x * E.R % P for x in pr.eq_table(r_canon[i + 1:])]
        assert len(want) == size and got[off: off + size] == want, (n, i)


CUBIC_LOG_LEN = [2, 16, 17]  # length 4: the smallest folding round; 2 * 16384 and 4 * 16384 pairs in round 0: the folding rounds pass SMALL_ROUND_PAIRS from above


@pytest.mark.parametrize("latency", [False, True])
@pytest.mark.parametrize("n", CUBIC_LOG_LEN)
def test_cubic_rounds_without_the_eq_array_equal_the_four_array_rounds(ctx, n, latency):
    """both routes through all n rounds with the same challenges: every round's f(0), f(-1), f_inf and the folded a, b, c"""
    from provekit_amd import sumcheck as sc
    from provekit_amd._lib import lib

    N = 1 << n
    assert N // 2 in (2, 2 * SMALL_ROUND_PAIRS, 4 * SMALL_ROUND_PAIRS)
    abc = [rnd(N, 500 + 10 * n + k) for k in range(3)]
    r, alphas = rnd(n, 540 + n), np.ascontiguousarray(rnd(n, 560 + n))
    old = [ctx.upload(x) for x in abc] + [sc.calculate_evaluations_over_boolean_hypercube_for_eq(ctx, r)]
    new = [ctx.upload(x) for x in abc]
    tables = suffix_tables(ctx, r, n)
    ctx.set_latency_mode(latency)
    try:
        length = N
        for t in range(n):
            want = sc.sumcheck_fold_map_reduce(ctx, *old, length, alphas[t - 1] if t else None)
            got = np.full((3, 4), 0xA5, dtype=np.uint64)
            ctx._check(lib.pk_selftest_sumcheck_cubic_spliteq(ctx.handle, new[0].ptr, new[1].ptr, new[2].ptr, tables.ptr, n, t, r.ctypes.data,
                                                              alphas.ctypes.data, got.ctypes.data))
            assert np.array_equal(got, want), (n, t, E.ints(got), E.ints(want))
            if t:
                length //= 2
            for k in range(3):
                assert np.array_equal(ctx.download_fe(new[k], length), ctx.download_fe(old[k], length)), (n, t, "abc"[k])
    finally:
        ctx.set_latency_mode(False)
        for b in old + new + [tables]:
            b.free()


def quad_at(h, x):
    """the quadratic through h(0), h(1), h(2) at x, on stored values"""
    c2 = E.mul(HALF, (h[2] - 2 * h[1] + h[0]) % P)
    c1 = (h[1] - h[0] - c2) % P
    return (h[0] + E.mul(x, (c1 + E.mul(x, c2)) % P)) % P


# lengths 4, 2 * 16384 and 4 * 16384 pairs as the cubic test, and 16384 pairs: the largest round of the four-lanes-per-pair kernel that does not fold
@pytest.mark.parametrize("latency", [False, True])
@pytest.mark.parametrize("log_len", [2, 15, 16, 17])
def test_quadratic_rounds_from_the_claim_equal_the_three_sum_rounds(ctx, log_len, latency):
    """round 0 without a fold, then every folding round down to one pair: h(0), h(2) and the derived h(1) = claim - h(0) against the
    three-sum kernel's, and the folded f, w; the claim is <f, w> first and the previous round's h(r) afterwards, as in the prover"""
    from provekit_amd import sumcheck as sc
    from provekit_amd._lib import lib

    N = 1 << log_len
    f, w = rnd(N, 600 + log_len), rnd(N, 620 + log_len)
    rs = np.ascontiguousarray(rnd(log_len, 640 + log_len))
    old = [[ctx.upload(f), ctx.alloc_fe(N // 2)], [ctx.upload(w), ctx.alloc_fe(N // 2)]]
    new = [[ctx.upload(f), ctx.alloc_fe(N // 2)], [ctx.upload(w), ctx.alloc_fe(N // 2)]]
    claim = E.ints(sc.weighted_sum(ctx, old[0][0], old[1][0], N))[0]
    ctx.set_latency_mode(latency)
    try:
        cur, length = 0, N
        for t in range(log_len):
            fold = rs[t - 1] if t else None
            want = sc.sumcheck_quadratic_round(ctx, old[0][cur], old[1][cur], length, fold, old[0][1 - cur], old[1][1 - cur])
            got = np.full((3, 4), 0xA5, dtype=np.uint64)
            ctx._check(lib.pk_selftest_sumcheck_quadratic_claim(ctx.handle, new[0][cur].ptr, new[1][cur].ptr, length, fold.ctypes.data if t else None,
                                                                new[0][1 - cur].ptr, new[1][1 - cur].ptr, E.limbs([claim]).ctypes.data, got.ctypes.data))
            assert np.array_equal(got, want), (log_len, t, E.ints(got), E.ints(want))
            if t:
                cur, length = 1 - cur, length // 2
                for k in range(2):
                    assert np.array_equal(ctx.download_fe(new[k][cur], length), ctx.download_fe(old[k][cur], length)), (log_len, t, "fw"[k])
            claim = quad_at(E.ints(want), E.ints(rs[t])[0])
    finally:
        ctx.set_latency_mode(False)
        for pair in old + new:
            for b in pair:
                b.free()


PROOF_CASES = {9: (7, 100, 60, 5.0), 12: (9, 500, 700, 4.0)}  # m: m_0, constraints, inputs, pow bits -- the small cases of test_gpu_prove.py
SEED = 4


@functools.lru_cache(maxsize=None)
def oracle_case(m):
    """the instance, its configs and the oracle prover's proof, once per size"""
    import oracle_lib as oracle
    import prover_ref as PR
    from test_gpu_prove import _vcfg
    from test_prover_ref import small_instance

    from provekit_amd.scheme import WhirConfig, blinding_config_for, create_io_pattern

    m_0, nc, n_in, pow_bits = PROOF_CASES[m]
    nw, z, coeffs, trips, mats = small_instance(nc, n_in, 31)
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    zm = oracle.to_mont(oracle.ints_to_limbs(z))
    cfg_w, cfg_b = WhirConfig.for_size(m, pow_bits), blinding_config_for(m_0, pow_bits)
    ds = create_io_pattern(m_0, cfg_w, cfg_b)
    want = PR.prove(ds, m, m_0, _vcfg(cfg_w), _vcfg(cfg_b), (nc, nw, mats, interner), zm, SEED.to_bytes(32, "little"))
    return nc, nw, trips, interner, zm, cfg_w, cfg_b, ds, want


@pytest.mark.parametrize("latency", [False, True])
@pytest.mark.parametrize("m", sorted(PROOF_CASES))
def test_whole_proofs_equal_the_oracle_provers(ctx, m, latency):
    from test_gpu_prove import to_sparse

    from provekit_amd.scheme import WhirR1CSScheme
    from provekit_amd.sparse_matrix import R1CS

    nc, nw, trips, interner, zm, cfg_w, cfg_b, ds, want = oracle_case(m)
    r1cs = R1CS(ctx, *(to_sparse(nc, nw, t) for t in trips), interner)
    scheme = WhirR1CSScheme(ctx, r1cs, m, PROOF_CASES[m][0], cfg_w, cfg_b)
    assert scheme.domain_separator == ds
    ctx.set_latency_mode(latency)
    try:
        got = scheme.prove(ctx.upload(zm), seed=SEED)
    finally:
        ctx.set_latency_mode(False)
    assert len(got) == len(want)
    if got != want:
        first = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f"pk_prove's transcript differs from the oracle prover's from byte {first} of {len(got)}")
    scheme.close()
    r1cs.close()
