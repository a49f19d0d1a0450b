"""GPU: the blinding WHIR on the host thread (csrc/host_whir.hpp; csrc/prover.hip commit_witness, prove_blinding, pow_round).

(a) Whole proofs, one statement per size.  The blinding configurations blinding_config_for derives (fold 4, rate 1/2, batch 2, one OOD
sample at the commitment):

  m =  9, m_0 =  7:  6 variables, no round;  124 final queries, 4 bits;   a tree of  8 leaves of width 32
  m = 13, m_0 = 11:  7 variables, no round;  123 final queries, 5 bits;   a tree of 16 leaves of width 32
  m = 18, m_0 = 17:  8 variables, one round: 122 queries, 6 bits, then 31 final queries, 4 bits;  32 leaves of width 32, then 16 of width 16
                     (the configuration of the bench statement, m_0 = 20)

Every case keeps these real blinding bits; the witness opening's grinding is test_pow_bits = 4 (at m = 18 its real 16 bits three times over
would be the run time), which also puts witness grinds under the host grinder's bound (4 bits by default).  For each size the proof
under the build's default threshold (the host route) and under pk_selftest_set_host_tail(0) (every line of the device route) from the same seed are the same bytes,
and the compiled verifier's host core (libprovekit_verify) accepts them -- at m = 9 the oracle's Python verifier too.  At m = 18 the
threshold is also set to exactly the blinding table length 2^8 (host route) and one step below (device route); once in latency mode, once
with hash version 1, once with the host grinder's bound at 0 and at 8.  The launch scopes tell that the work really moved.

(b) Components: pk_selftest_host_commit against pk_commit on the device -- root, leaf matrix and nodes -- for batch 2 at n = 4 and n = 8
and batch 1 at n = 4 and rate 1/16, and pk_selftest_host_pow against pk_pow_solve for three challenges at 1, 6 and 8 bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SIZES = [(9, 7, 6), (13, 11, 7), (18, 17, 8)]  # m, m_0, the blinding polynomial's variables
NW = 200  # witness entries: far below every capacity, so one small statement serves the three sizes


@pytest.fixture(scope="module")
def own_ctx():
    """a context of this module's own: the switches are per context, and the session's context keeps the build's defaults"""
    import torch

    torch.cuda.is_available()
    import provekit_amd

    c = provekit_amd.Context(0)
    yield c
    c.close()


class Case:
    def __init__(self, c, oracle, m, m_0):
        from test_gpu_commit_fused import instance_of_length
        from test_gpu_prove import to_sparse

        from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
        from provekit_amd.sparse_matrix import R1CS

        self.c, self.m, self.m_0 = c, m, m_0
        self.nc, self.nw, z, self.coeffs, self.trips = instance_of_length(NW, m_0)
        self.interner = oracle.to_mont(oracle.ints_to_limbs(self.coeffs))
        self.cfg_w, self.cfg_b = WhirConfig.for_size(m, 4.0), blinding_config_for(m_0)
        self.sparse = [to_sparse(self.nc, self.nw, t) for t in self.trips]
        self.r1cs = R1CS(c, *self.sparse, self.interner)
        self.scheme = WhirR1CSScheme(c, self.r1cs, m, m_0, self.cfg_w, self.cfg_b)
        self.d_z = c.upload(oracle.to_mont(oracle.ints_to_limbs(z)))

    def prove(self, seed=11):
        return self.scheme.prove(self.d_z, seed=seed)

    def accepted(self, proof, hash_version=2):
        from provekit_amd.verify import Verifier

        v = Verifier.for_scheme(self.scheme, tuple(self.sparse), self.interner, hash_version=hash_version, attach=False)
        try:
            return v.verify(proof).accepted
        finally:
            v.close()

    def close(self):
        self.scheme.close()
        self.r1cs.close()


@pytest.fixture(scope="module", params=SIZES, ids=[f"m{m}" for m, _, _ in SIZES])
def case(request, own_ctx, oracle):
    m, m_0, nvars = request.param
    k = Case(own_ctx, oracle, m, m_0)
    assert k.cfg_b.n_vars == nvars
    yield k
    k.close()


def same(got, want, what):
    if got != want:
        first = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
        raise AssertionError(f"{what}: the proof differs from byte {first} of {len(want)} ({len(got)})")


def scopes(c, k):
    c.profile(True)
    c.profile_reset()
    k.prove(seed=3)
    prof = c.profile_read()
    c.profile(False)
    c.profile_reset()
    return {name: v[0] for name, v in prof.items()}


def test_the_blinding_configurations_are_the_ones_the_docstring_names(own_ctx):
    from provekit_amd.scheme import blinding_config_for  # (after own_ctx: torch's HIP runtime is loaded before the library's)

    got = [(c.n_vars, c.num_queries, c.pow_bits, c.final_queries, c.final_pow_bits) for c in (blinding_config_for(m_0) for _, m_0, _ in SIZES)]
    assert got == [(6, [], [], 124, 4.0), (7, [], [], 123, 5.0), (8, [122], [6.0], 31, 4.0)]
    assert blinding_config_for(20).__dict__ == blinding_config_for(17).__dict__


def test_host_route_and_device_route_write_the_same_bytes(case, own_ctx, oracle):
    c, k = own_ctx, case
    try:
        c.set_host_tail(0)
        want = k.prove()
        assert k.accepted(want)
        c.set_host_tail(10)  # the build's default
        same(k.prove(), want, f"m = {k.m}, default threshold")
        if k.m == 9:  # the oracle's Python verifier, independent of every line of the library
            import verifier as V
            from test_gpu_prove import _vcfg

            mats = [(t[0], t[1], [k.coeffs[v] for v in t[2]]) for t in k.trips]
            assert V.verify(want, k.scheme.domain_separator, k.m, k.m_0, _vcfg(k.cfg_w), _vcfg(k.cfg_b), r1cs=(k.nc, k.nw, mats))
    finally:
        c.set_host_tail(10)


def test_the_switch_sits_exactly_at_the_blinding_table_length(own_ctx, oracle):
    """m = 18: tables of 2^8 entries.  Threshold 2^8: host route; 2^7: device route (and the opening's tables no longer start on the host)"""
    c = own_ctx
    k = Case(c, oracle, 18, 17)
    try:
        c.set_host_tail(0)
        want = k.prove()
        off = scopes(c, k)
        c.set_host_tail(8)
        same(k.prove(), want, "threshold 2^8")
        on = scopes(c, k)
        c.set_host_tail(7)
        same(k.prove(), want, "threshold 2^7")
        below = scopes(c, k)
        print("scopes at 0:", off, "\nat 2^8:", on, "\nat 2^7:", below)
        # the witness commitment is one leaf hash and one tree, the witness opening's three rounds one each; the blinding's two of each are gone
        assert off["leaf_hash"] == 6 and on["leaf_hash"] == 4 and off["merkle_inner"] == 6 and on["merkle_inner"] == 4
        assert below["leaf_hash"] == 6 and below["merkle_inner"] == 6
        # ... and its round's fold and final fold, its two OOD evaluations (the commitment's two polynomials in one launch, the round's one)
        for other in (off, below):
            assert other["fold_coeffs"] - on["fold_coeffs"] == 2 and other["eval_univariate"] - on["eval_univariate"] == 2
            assert other["to_coeffs"] == on["to_coeffs"] == 2  # the tables are still drawn and transformed on the device
        # threshold 0 grinds everything on the device: the blinding's 6 and 4 bits, the witness opening's four grinds of 4 bits; otherwise
        # only the blinding round's 6 bits are above the default bound of 4
        assert off["pow_search"] == 6 and on["pow_search"] == 1 and below["pow_search"] == 1
        # one transfer each for the zk tables, the witness opening's p and w, and the blinding tables: on the host route all four of them
        # (f, g and their coefficient forms) before the commitment, one step below p and w after the opening's first rounds
        assert below["tables_to_host"] == on["tables_to_host"] == 3
    finally:
        c.set_host_tail(10)
        k.close()


@pytest.mark.parametrize("how", ["latency", "hash1", "pow0", "pow8"])
def test_modes_that_meet_the_host_route(own_ctx, oracle, how):
    c = own_ctx
    k = Case(c, oracle, 18, 17)
    try:
        if how == "latency":
            c.set_latency_mode(True)
        if how == "hash1":
            c.set_hash_version(1)
        c.set_host_tail(0)
        want = k.prove()
        assert k.accepted(want, hash_version=1 if how == "hash1" else 2)
        c.set_host_tail(10)
        if how == "pow0":
            c.set_host_pow(0)
            assert scopes(c, k)["pow_search"] == 2 + 4  # the blinding's two grinds and the witness opening's four, all on the device
        if how == "pow8":
            c.set_host_pow(8)
            assert "pow_search" not in scopes(c, k)  # 6 and 4 bits, and test_pow_bits = 4
        same(k.prove(), want, how)
    finally:
        c.set_latency_mode(False)
        c.set_hash_version(2)
        c.set_host_pow(4)
        c.set_host_tail(10)
        k.close()


def test_the_setter_of_the_grinder_bound_refuses_what_it_cannot_take(own_ctx):
    from provekit_amd._lib import ProveKitHipError, lib

    for bad in (9, 11, 64, 2**31):
        with pytest.raises(ProveKitHipError) as e:
            own_ctx.set_host_pow(bad)
        assert e.value.code == -1 and "host grinder" in str(e.value)
    assert lib.pk_selftest_set_host_pow(None, 4) == -1
    for ok in (0, 1, 8, 4):  # the last one: the build's default
        own_ctx.set_host_pow(ok)


@pytest.mark.parametrize("batch,n,log_inv_rate", [(2, 4, 1), (2, 8, 1), (1, 4, 4)])
def test_host_commitment_equals_the_device_commitment(ctx, batch, n, log_inv_rate):
    from provekit_amd._lib import lib
    from provekit_amd.field import random_field
    from provekit_amd.whir import commit_batch

    fold = 4
    rows, width = 1 << (n + log_inv_rate - fold), batch << fold
    polys = [random_field(1 << n, 90 + 7 * n + b) for b in range(batch)]
    polys[0][:3] = 0  # zero, and Montgomery 1 and p - 1 come with the asan driver; here the device's own bits
    dev = commit_batch(ctx, [ctx.upload(p) for p in polys], n, log_inv_rate, fold)
    try:
        assert (dev.n_leaves, dev.width) == (rows, width)
        d_leaves = ctx.download(dev.d_leaves, (width, rows, 4))
        d_nodes = ctx.download(dev.d_nodes, (2 * rows, 4))
        coeffs = np.ascontiguousarray(np.concatenate(polys), dtype=np.uint64)
        leaves = np.zeros((width, rows, 4), dtype=np.uint64)
        nodes = np.zeros((2 * rows, 4), dtype=np.uint64)
        assert lib.pk_selftest_host_commit(2, coeffs.ctypes.data, batch, n, log_inv_rate, fold, leaves.ctypes.data, nodes.ctypes.data) == 0
        assert np.array_equal(leaves, d_leaves)
        assert np.array_equal(nodes, d_nodes)
        assert nodes[1].tobytes() == dev.root
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [1.0, 6.0, 8.0])
def test_host_nonce_equals_the_device_nonce(ctx, bits):
    from provekit_amd._lib import lib
    from provekit_amd.pow import SkyscraperPoW

    rng = np.random.default_rng(int(bits))
    for i in range(3):
        ch = bytes(rng.integers(0, 256, size=32, dtype=np.uint8)) if i else b"\xff" * 32  # once a challenge above p
        n = C.c_uint64(0)
        assert lib.pk_selftest_host_pow((C.c_uint8 * 32)(*ch), bits, C.byref(n)) == 0
        assert n.value == SkyscraperPoW(ch, bits, ctx).solve()
