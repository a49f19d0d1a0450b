"""GPU: pk_prove over every scheme shape pk_scheme_create accepts (the grid of prove_shape_cases.py), byte for byte against the oracle
prover (oracle/prover_ref.py).  The other suites prove with WhirConfig.for_size / blinding_config_for alone -- fold 4, rate 1/2, one OOD
sample, the derived round count -- so WhirProver (csrc/prover.hip) otherwise never runs away from k = 4.

  A  the oracle's bytes with the host tail off (everything on the device), at the build's default (2^10), and at a threshold that puts the
     boundary inside an opening; a mismatch names the first differing byte and its region
  B  the same bytes in latency mode: the blinding commitment on the side stream (threshold 0) and on the host thread (default)
  C  the same bytes under hash version 1
  D  the compiled verifier (provekit_amd.verify) accepts each device proof and refuses it with a final coefficient changed
  E  the launch scopes (pk_profile_*) tell that the route claimed is the route taken
  F  pk_scheme_create refuses each bound of the family with an error that names the cause, creates the neighbour and proves with it
  G  one scheme proves two statements back to back, then the first again: leftovers in the arena would show
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prove_shape_cases as G  # noqa: E402

ids = lambda e: e.id if isinstance(e, G.Entry) else None  # noqa: E731
DEFAULT_TAIL = 10  # PK_HOST_TAIL_DEFAULT_LOG2 (csrc/ctx.hpp): the setter has no getter


@pytest.fixture(scope="module")
def own_ctx():
    """a context of this module's own: the switches are per context, and the session's context keeps the build's defaults"""
    import torch

    torch.cuda.is_available()
    import provekit_amd

    c = provekit_amd.Context(0)
    yield c
    c.close()


class Prover:
    """an entry's R1CS, scheme and witness on the device.  The empty witness: pk_prove wants a non-null pointer, so one element that
    nothing reads, with n_witness = 0"""

    def __init__(self, c, oracle, entry):
        from test_gpu_prove import to_sparse

        from provekit_amd.scheme import WhirR1CSScheme
        from provekit_amd.sparse_matrix import R1CS

        self.c, self.entry, self.inst = c, entry, G.instance(oracle, entry)
        self.cw, self.cb = entry.cfgs()
        self.r1cs = R1CS(c, *(to_sparse(self.inst.nc, self.inst.nw, t) for t in self.inst.trips), self.inst.interner)
        self.scheme = WhirR1CSScheme(c, self.r1cs, entry.m, entry.m_0, self.cw, self.cb)
        self.d_z = self.upload(self.inst.zm)

    def upload(self, zm):
        return self.c.upload(zm if self.inst.nw else np.full((1, 4), 0xDEADBEEF, dtype=np.uint64))

    def prove(self, seed=G.SEED, d_z=None):
        return self.scheme.prove(self.d_z if d_z is None else d_z, seed=seed)

    def close(self):
        self.scheme.close()
        self.r1cs.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.set_latency_mode(False)
        self.c.set_hash_version(2)
        self.c.set_host_tail(DEFAULT_TAIL)
        self.close()


def same_bytes(got, want, p, what):
    diff = G.first_difference(got, want, p.entry.m_0, p.cw, p.cb)
    assert not diff, f"{p.entry.id}, {what}: {diff}"


def thresholds(entry):
    """0: everything on the device; the build's default; and the largest power of two below the witness table and below the blinding
    table (where that is 2 entries or more): the boundary falls inside each opening"""
    inside = {entry.m - 1, G.nb_vars(entry.m_0) - 1} - {0}
    return [0, DEFAULT_TAIL] + sorted(inside - {DEFAULT_TAIL})


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_a_the_oracle_provers_bytes_at_every_shape_and_threshold(own_ctx, oracle, entry):
    want = G.oracle_proof(oracle, entry)[0]
    with Prover(own_ctx, oracle, entry) as p:
        assert len(thresholds(entry)) >= 3
        for log2_len in thresholds(entry):
            own_ctx.set_host_tail(log2_len)
            same_bytes(p.prove(), want, p, f"host tail 2^{log2_len}" if log2_len else "host tail off")


def test_a_ran_over_the_whole_grid():
    assert len(G.GRID) == 38 and len({e.id for e in G.GRID}) == 38


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.LATENCY, ids=ids)
def test_b_latency_mode_writes_the_same_bytes(own_ctx, oracle, entry):
    """threshold 0: the blinding commitment on the side stream; the default: on the host thread (Proof::init, csrc/prover.hip)"""
    want = G.oracle_proof(oracle, entry)[0]
    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_latency_mode(True)
        for log2_len in thresholds(entry):
            own_ctx.set_host_tail(log2_len)
            same_bytes(p.prove(), want, p, f"latency mode, host tail 2^{log2_len}" if log2_len else "latency mode, host tail off")
        own_ctx.set_latency_mode(False)
        same_bytes(p.prove(), want, p, "plain mode again")


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.HASH_V1, ids=ids)
def test_c_hash_version_1(own_ctx, oracle, entry):
    want = G.oracle_proof(oracle, entry, hash_version=1)[0]
    assert want != G.oracle_proof(oracle, entry)[0]
    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_hash_version(1)
        for latency in (False, True):
            own_ctx.set_latency_mode(latency)
            for log2_len in thresholds(entry):
                own_ctx.set_host_tail(log2_len)
                same_bytes(p.prove(), want, p, f"hash version 1, latency mode {latency}, host tail 2^{log2_len}")


# ---- D ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_d_the_compiled_verifier_accepts_the_device_proof(own_ctx, oracle, entry):
    from provekit_amd.verify import Verifier

    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_host_tail(0)
        proof = p.prove()
        ver = Verifier(entry.m, entry.m_0, p.cw, p.cb)
        try:
            r = ver.verify(proof)
            assert r.accepted and r.check == "NONE" and r.offset == len(proof), (entry.id, r)
            pos = G.offsets(proof, entry.m_0, p.cw, p.cb)
            for side in ("witness", "blinding"):
                bad = bytearray(proof)
                bad[pos[f"{side}/final_coeffs"]] ^= 1
                r = ver.verify(bytes(bad))
                assert not r.accepted and r.check != "NONE" and r.message, (entry.id, side, r)
        finally:
            ver.close()


# ---- E ------------------------------------------------------------------------------------------------------------------------------------
def launches(p):
    """{scope: launches} of one proof on the prover's own context (csrc/mle.hip, csrc/pow.hip ProfScope names)"""
    c = p.c
    c.profile(True)
    c.profile_reset()
    p.prove(seed=3)
    prof = c.profile_read()
    c.profile(False)
    c.profile_reset()
    return {k: v[0] for k, v in prof.items() if v[0]}


def first_launches(entry):
    """how many launches of opening_first_launch (scope "opening_first") a proof of `entry` makes with the host tail off, from
    WhirProver::start's condition and round_weights' (csrc/prover.hip): per side, the opening's own first launch -- tables of two entries
    or more, one row or three rows of equal length at equal stride: never an empty witness, whose three rows coincide -- and one per
    folding round whose tables still have two entries or more"""
    n = 0
    for c, rows_ok in zip(entry.cfgs(), (entry.nw >= 1, True)):
        n += int(rows_ok and c.n_vars >= 1 and c.folding_factor >= 1)
        n += sum(1 for r in range(c.n_rounds) if c.n_vars - c.folding_factor * (r + 1) >= 1)
    return n


SIBLING = next(e for e in G.GRID if e.id == "witness-of-one")  # EMPTY_NC0's shape and configs with a witness of one element


@pytest.mark.parametrize("entry", [G.NO_ROUND, G.M1, G.WITNESS_FOLDS[1], G.WITNESS_FOLDS[8], G.BLINDING_FOLDS[7], G.FINAL5, G.CAPACITY, G.EMPTY, G.EMPTY_NC0, SIBLING], ids=ids)
def test_e_the_first_launches_are_taken_where_start_says_so(own_ctx, oracle, entry):
    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_host_tail(0)
        off = launches(p)
        assert off.get("opening_first", 0) == first_launches(entry), (entry.id, off)
        assert "tables_to_host" not in off and off["sumcheck_cubic"] == entry.m_0, (entry.id, off)
    if entry is G.NO_ROUND:
        assert first_launches(entry) == 2  # the blinding opening's and the witness opening's, and no round's


def test_e_an_empty_witness_takes_the_plain_route_and_skips_its_dot_products(own_ctx, oracle):
    """against the same shape with a witness of one element: one first launch fewer (start_plain), and two "dot" scopes fewer: the witness
    statement's dot_rows and the deferred hint's (its else arm forms the eq table and has no entry to multiply)"""
    assert (G.EMPTY_NC0.m, G.EMPTY_NC0.m_0, G.EMPTY_NC0.w, G.EMPTY_NC0.b) == (SIBLING.m, SIBLING.m_0, SIBLING.w, SIBLING.b) and SIBLING.nw == 1
    counts = {}
    for entry in (G.EMPTY_NC0, SIBLING):
        with Prover(own_ctx, oracle, entry) as p:
            own_ctx.set_host_tail(0)
            counts[entry.id] = launches(p)
    empty, one = counts[G.EMPTY_NC0.id], counts[SIBLING.id]
    assert one["opening_first"] - empty["opening_first"] == 1, (empty, one)
    assert one["dot"] - empty.get("dot", 0) == 2, (empty, one)


@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_e_at_the_default_threshold_no_sumcheck_launch_is_left(own_ctx, oracle, entry):
    """m, m_0 <= 10: every sumcheck table is within 2^10 entries before its first round"""
    assert entry.m <= 10 and entry.m_0 <= 10
    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_host_tail(DEFAULT_TAIL)
        on = launches(p)
        for scope in ("sumcheck_cubic", "sumcheck_quadratic", "opening_first", "fold_pairs"):
            assert scope not in on, (entry.id, on)
        assert on["tables_to_host"] == 3, (entry.id, on)  # the four blinding tables; the zk tables; the witness opening's p and w


@pytest.mark.parametrize("entry", G.SINGLE_GRIND, ids=ids)
def test_e_the_grinder_is_the_one_pow_round_names(own_ctx, oracle, entry):
    """at most PK_HOST_POW_MAX_BITS = 4 bits and a host tail: the host thread; above, or with the host tail off: the device ("pow_search")"""
    bits = entry.only[2]
    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_host_tail(DEFAULT_TAIL)
        on = launches(p)
        assert on.get("pow_search", 0) == (1 if bits > 4 else 0), (entry.id, on)
        own_ctx.set_host_tail(0)
        assert launches(p).get("pow_search", 0) == 1, entry.id


# ---- F ------------------------------------------------------------------------------------------------------------------------------------
def raw_create(c, r1cs, entry):
    from provekit_amd._lib import lib

    sw, sb = entry.structs()
    h = C.c_void_p()
    rc = lib.pk_scheme_create(c.handle, r1cs.handle, entry.nc, entry.nw, entry.scheme[0], entry.scheme[1], C.byref(sw), C.byref(sb), C.byref(h))
    if rc == 0:
        lib.pk_scheme_destroy(c.handle, h)
    return rc, c.last_error()


@pytest.mark.parametrize("what,cause,refused,accepted,provable,of_the_config", G.BOUNDS, ids=[b[0] for b in G.BOUNDS])
def test_f_the_bounds_refuse_with_the_cause_and_the_neighbour_proves(own_ctx, oracle, what, cause, refused, accepted, provable, of_the_config):
    from test_gpu_prove import to_sparse

    from provekit_amd.sparse_matrix import R1CS

    inst = G.instance(oracle, refused)
    r1cs = R1CS(own_ctx, *(to_sparse(inst.nc, inst.nw, t) for t in inst.trips), inst.interner)
    try:
        rc, why = raw_create(own_ctx, r1cs, refused)
        assert rc == -1 and re.search(cause, why), (what, rc, why)
    finally:
        r1cs.close()
    if accepted is not None:
        with Prover(own_ctx, oracle, accepted) as p:  # created
            if provable:
                same_bytes(p.prove(), G.oracle_proof(oracle, accepted)[0], p, f"the accepted neighbour of {what}")
    # after the refusal the context still proves
    with Prover(own_ctx, oracle, G.WITNESS_FOLDS[3]) as p:
        same_bytes(p.prove(), G.oracle_proof(oracle, G.WITNESS_FOLDS[3])[0], p, f"after the refusal of {what}")


# ---- G ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_len", [0, DEFAULT_TAIL], ids=["tail-off", "tail-default"])
@pytest.mark.parametrize("entry", G.REUSE, ids=ids)
def test_g_one_scheme_proves_two_statements_and_the_first_again(own_ctx, oracle, entry, log2_len):
    """another witness where the statement has one, another key where it has none (the empty witness): what the second proof leaves in the
    arena -- w0 with no point to overwrite it, the rows of a longer opening -- must not reach the third"""
    with Prover(own_ctx, oracle, entry) as p:
        own_ctx.set_host_tail(log2_len)
        first = G.oracle_proof(oracle, entry)[0]
        z2 = p.inst.other_witness(oracle, 11)
        second = G.oracle_proof(oracle, entry, seed=G.SEED + 1, witness=z2)[0]
        d_z2 = p.upload(z2)
        assert second != first
        same_bytes(p.prove(), first, p, "the first proof")
        same_bytes(p.prove(seed=G.SEED + 1, d_z=d_z2), second, p, "the second statement")
        same_bytes(p.prove(), first, p, "the first statement again")
