"""GPU: the prover's host tail (pk_selftest_set_host_tail; csrc/host_tail.hpp, csrc/prover.hip sumcheck_round_loop).  Whole proofs with the
switch at 0 -- every sumcheck round on the device -- against every threshold 2^1 .. 2^11, byte for byte, plain and in latency mode, and at
m <= 10 against the oracle's prover (oracle/prover_ref.py).  With folding factor 4 (the other folds, 1 .. 8, with the boundary inside each
opening: tests/test_gpu_prove_shapes.py) the thresholds meet every position of the boundary:

  zk sumcheck (tables of 2^m_0):  2^11 >= 2^m_0: before the first round, all rounds on the host;  in between: in the middle;
                                  2^2: the last round alone (its tables have 4 entries before its fold);  2^1: never reached
  WHIR openings (2^n entries):    >= 2^n: the opening's tables go to the host before round 0 (the blinding opening: they are formed there);
                                  2^(n-4), 2^(n-8): a length reached exactly where a sumcheck_rounds call ends;  the others: inside a call;
                                  m = 12: 2^12 > 2^11, so the first rounds always stay on the device

The launch scopes (pk_profile_*) tell that the rounds really moved: a silent no-op of the switch would pass the byte comparison."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
THRESHOLDS = range(1, 12)
SIZES = [(6, 4), (8, 6), (9, 7), (12, 9)]  # m, m_0


@pytest.fixture(scope="module")
def own_ctx():
    """a context of this module's own: the switch is per context, and the session's context keeps the build's default"""
    import torch

    torch.cuda.is_available()
    import provekit_amd

    c = provekit_amd.Context(0)
    yield c
    c.close()


def statement(m, m_0, zero_tail):
    """(nc, nw, z, coeffs, trips): the witness at the scheme's capacity 2^(m-1) - 5, or -- zero_tail -- half of it, then zeros that no
    constraint reads (trailing zero support of the witness and of the statement's rows)"""
    from test_gpu_commit_fused import instance_of_length

    cap = (1 << (m - 1)) - 5
    if not zero_tail:
        return instance_of_length(cap, m_0)
    nc, nw, z, coeffs, trips = instance_of_length(cap // 2, m_0)
    return nc, cap, list(z) + [0] * (cap - nw), coeffs, trips


def make_scheme(c, oracle, m, m_0, zero_tail):
    from test_gpu_prove import to_sparse

    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
    from provekit_amd.sparse_matrix import R1CS

    nc, nw, z, coeffs, trips = statement(m, m_0, zero_tail)
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    zm = oracle.to_mont(oracle.ints_to_limbs(z))
    cfg_w, cfg_b = WhirConfig.for_size(m, 4.0), blinding_config_for(m_0, 4.0)
    r1cs = R1CS(c, *(to_sparse(nc, nw, t) for t in trips), interner)
    return WhirR1CSScheme(c, r1cs, m, m_0, cfg_w, cfg_b), r1cs, zm, (nc, nw, trips, interner, cfg_w, cfg_b)


@pytest.mark.parametrize("zero_tail", [False, True], ids=["capacity", "zero-tail"])
@pytest.mark.parametrize("m,m_0", SIZES)
def test_whole_proofs_are_the_same_bytes_at_every_threshold(own_ctx, oracle, m, m_0, zero_tail):
    c = own_ctx
    scheme, r1cs, zm, (nc, nw, trips, interner, cfg_w, cfg_b) = make_scheme(c, oracle, m, m_0, zero_tail)
    d_z = c.upload(zm)
    try:
        c.set_host_tail(0)
        want = scheme.prove(d_z, seed=7)
        if m <= 10 and not zero_tail:  # ... which is the oracle prover's proof string
            import prover_ref as PR
            from test_gpu_prove import _vcfg

            mats = []
            for rows, cols, vals in trips:
                rows = np.array(rows, dtype=np.int64)
                mats.append((np.searchsorted(rows, np.arange(nc)).astype(np.uint32), np.array(cols, dtype=np.uint32), np.array(vals, dtype=np.uint32)))
            ref = PR.prove(scheme.domain_separator, m, m_0, _vcfg(cfg_w), _vcfg(cfg_b), (nc, nw, mats, interner), zm, (7).to_bytes(32, "little"))
            assert want == ref
        for latency in (False, True):
            c.set_latency_mode(latency)
            for log2_len in (0, *THRESHOLDS):
                c.set_host_tail(log2_len)
                got = scheme.prove(d_z, seed=7)
                if got != want:
                    first = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
                    raise AssertionError(f"threshold 2^{log2_len}, latency mode {latency}: the proof differs from byte {first} of {len(want)} ({len(got)})")
    finally:
        c.set_latency_mode(False)
        scheme.close()
        r1cs.close()


def launches(c, scheme, d_z):
    c.profile(True)
    c.profile_reset()
    scheme.prove(d_z, seed=3)
    prof = c.profile_read()
    c.profile(False)
    c.profile_reset()
    return {k: v[0] for k, v in prof.items()}


@pytest.mark.parametrize("latency", [False, True], ids=["plain", "latency"])
def test_the_rounds_move_to_the_host_and_zero_brings_them_back(own_ctx, oracle, latency):
    """m = 12, m_0 = 9: at 0 the zk sumcheck is 9 cubic launches and nothing goes through the tables' transfer; at 2^11 no cubic launch is
    left, the only quadratic launch is the witness opening's round 1, and the transfers are three: the four blinding tables (f, g and
    their coefficient forms), the zk tables, the witness opening's p and w; at 2^4 the first 6 cubic rounds stay; back at 0, the first counts"""
    c = own_ctx
    m, m_0 = 12, 9
    scheme, r1cs, zm, _ = make_scheme(c, oracle, m, m_0, False)
    d_z = c.upload(zm)
    c.set_latency_mode(latency)
    try:
        c.set_host_tail(0)
        off = launches(c, scheme, d_z)
        assert off["sumcheck_cubic"] == m_0 and "tables_to_host" not in off
        c.set_host_tail(11)
        on = launches(c, scheme, d_z)
        assert "sumcheck_cubic" not in on and on["tables_to_host"] == 3
        # the witness opening: round 0 inside the opening's first launch, round 1 folds 2^12 entries on the device; round 2 would fold 2^11
        assert on.get("opening_first", 0) == 1 and on.get("sumcheck_quadratic", 0) == 1 and "fold_pairs" not in on
        assert off["sumcheck_quadratic"] > 1 and off["fold_pairs"] >= 1
        c.set_host_tail(4)  # tables of 16 entries before the fold: rounds 0 .. 5 of 9 stay
        mid = launches(c, scheme, d_z)
        assert mid["sumcheck_cubic"] == 6
        c.set_host_tail(0)
        assert launches(c, scheme, d_z) == off
    finally:
        c.set_latency_mode(False)
        scheme.close()
        r1cs.close()


def test_the_setter_refuses_what_it_cannot_take(own_ctx):
    from provekit_amd._lib import ProveKitHipError, lib

    for bad in (12, 13, 64, 2**31):
        with pytest.raises(ProveKitHipError) as e:
            own_ctx.set_host_tail(bad)
        assert e.value.code == -1 and "host tail" in str(e.value)
    assert lib.pk_selftest_set_host_tail(None, 9) == -1
    for ok in (0, 1, 11, 9):
        own_ctx.set_host_tail(ok)
