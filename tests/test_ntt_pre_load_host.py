"""CPU: the load of an NTT pass that carries pass 1 (ntt_regs.hpp pre_load_sum, the exact __host__ __device__ source of ntt.hip's
PassParams::pre_terms path) executed on the host through pk_selftest_pre_load, at the extremes of its contract: one to three
nonzero rows of pass 1, rows past the nonzero inputs, inputs up to 2^256 - 1 and multipliers 0, 1 and p - 1.  Its result enters the
register network, which takes normalised limbs and values below 1.2p (test_fe29_host.py::test_ntt_butterfly_network_on_the_host)."""
import numpy as np
import pytest

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HI = 12 * P // 10


def rand_fe(n, seed, bound=P):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % bound for _ in range(n)]


def pre_load(oracle, xs, tws, terms, live):
    from provekit_amd._lib import lib

    n = len(xs) // terms
    out = np.empty((n, 4), dtype=np.uint64)
    a, t = oracle.ints_to_limbs(xs), oracle.ints_to_limbs(tws)
    assert lib.pk_selftest_pre_load(a.ctypes.data, t.ctypes.data, out.ctypes.data, terms, live, n) == 0
    return oracle.limbs_to_ints(out)


@pytest.mark.parametrize("terms", [1, 2, 3])
def test_ntt_pre_load_on_the_host(oracle, terms):
    edge_x = [0, 1, P - 1, P, HI, 2 * P - 1, 5 * P, (1 << 256) - 1]
    edge_w = [0, 1, P - 1, P // 2]
    xs, tws = [], []
    for x in edge_x:  # every term at the same extreme: the sum of the products at its largest
        for w in edge_w:
            xs += [x] * terms
            tws += [w] * terms
    n_rand = 300
    xs += rand_fe(n_rand * terms, 70 + terms, 1 << 256)
    tws += rand_fe(n_rand * terms, 80 + terms)
    for live in range(terms + 1):  # rows n1 >= live lie past the nonzero inputs: their terms are left out
        got = pre_load(oracle, xs, tws, terms, live)
        for i, y in enumerate(got):
            want = sum(xs[terms * i + k] * tws[terms * i + k] for k in range(live)) % P
            assert y % P == want, (terms, live, i)
            assert y < HI, (terms, live, i, y / P)  # what the network takes
