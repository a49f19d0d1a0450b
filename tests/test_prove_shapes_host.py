"""CPU: the grid of prove_shape_cases.py -- every scheme shape pk_scheme_create accepts, far from the fold-4, rate-1/2, one-OOD-sample
configs the other suites prove with -- on the ORACLE's side: the oracle prover's proof of every entry is accepted by the oracle
verifier (matrix check included) and refused after tampering in each named region, and the host-only entry points that take a config
(pk_whir_r1cs_io_pattern, pk_io_pattern_check, pk_scheme_arena_bytes) take every grid config and state the config bounds as BOUNDS does.
tests/test_gpu_prove_shapes.py then asks pk_prove for the same bytes."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prove_shape_cases as G  # noqa: E402

ids = lambda e: e.id if isinstance(e, G.Entry) else None  # noqa: E731


def test_the_grid_reaches_every_shape_it_names():
    cfgs = [e.cfgs() for e in G.GRID]
    assert len(G.GRID) == 38 and len({e.id for e in G.GRID}) == len(G.GRID)
    for e in G.GRID:
        assert e.fits() and e.patch is None and e.scheme == (e.m, e.m_0), e.id
        assert e.m <= 10 and e.m_0 <= e.m, e.id
    assert {cw.folding_factor for cw, _ in cfgs} == set(range(1, 9)) and {cb.folding_factor for _, cb in cfgs} == set(range(1, 8))
    assert {cw.starting_log_inv_rate for cw, _ in cfgs} == {1, 2} and {cb.starting_log_inv_rate for _, cb in cfgs} == {1, 3}
    assert {cw.n_rounds for cw, _ in cfgs} >= {0, 1, 2, 5, 8} and {cb.n_rounds for _, cb in cfgs} >= {0, 1, 2, 4}
    assert {e.final_vars()[0] for e in G.GRID} >= {0, 1, 5, 6} and {e.final_vars()[1] for e in G.GRID} >= {0, 1, 2, 4}
    assert {cw.commitment_ood_samples for cw, _ in cfgs} == {0, 1, 4} and {cb.commitment_ood_samples for _, cb in cfgs} == {0, 1, 3}
    assert {o for cw, cb in cfgs for o in cw.ood_samples + cb.ood_samples} == {0, 1, 2, 4}
    for side in (0, 1):  # each position grinds alone, at a host grinder's difficulty and at a device grinder's
        alone = {(bool(c.n_rounds and c.pow_bits[0]), bool(c.final_pow_bits), bool(c.final_folding_pow_bits), max(c.pow_bits + [c.final_pow_bits, c.final_folding_pow_bits]))
                 for c in (p[side] for p, e in zip(cfgs, G.GRID) if e.only and e.only[0] == "wb"[side])}
        assert alone == {(a == 0, a == 1, a == 2, bits) for a in range(3) for bits in (G.GRIND_BITS, G.DEVICE_GRIND_BITS)}
    assert G.GRIND_BITS <= 4 < G.DEVICE_GRIND_BITS  # PK_HOST_POW_MAX_BITS (csrc/ctx.hpp)
    assert {(e.m, e.m_0) for e in G.GRID} >= {(1, 1), (2, 1)}
    assert {e.nw for e in G.GRID} >= {0, 1, 27} and any(e.nw == 1 << (e.m - 1) for e in G.GRID)
    assert {e.nc for e in G.GRID} >= {0, 1} and sum(e.nc == 1 << e.m_0 for e in G.GRID) >= 2
    assert all(e in G.GRID for e in G.LATENCY + G.HASH_V1 + G.TAMPERED + G.REUSE)
    assert {e.cfgs()[0].folding_factor for e in G.LATENCY} == set(range(1, 9))


def test_oracle_built_proofs_are_accepted_at_every_shape(oracle):
    """every entry in one test, so that the count is this test's own: none skipped, none deselected"""
    import verifier as V

    ran = 0
    for e in G.GRID:
        proof, ds, (vw, vb), inst = G.oracle_proof(oracle, e)
        assert V.verify(proof, ds, e.m, e.m_0, vw, vb, r1cs=(inst.nc, inst.nw, inst.canonical)), e.id
        regions = G.walk(proof, e.m_0, *e.cfgs())  # the layout the tampering tests and the device tests' reports rely on
        assert regions[-1][2] == len(proof), e.id
        ran += 1
    assert ran == len(G.GRID) == 38


@pytest.mark.parametrize("entry", G.HASH_V1, ids=ids)
def test_the_version_1_proofs_are_accepted_under_version_1_only(oracle, entry):
    import verifier as V

    proof, ds, (vw, vb), inst = G.oracle_proof(oracle, entry, hash_version=1)
    assert proof != G.oracle_proof(oracle, entry)[0]
    assert V.verify(proof, ds, entry.m, entry.m_0, vw, vb, r1cs=(inst.nc, inst.nw, inst.canonical), hash_version=1)
    with pytest.raises(V.VerifyError):
        V.verify(proof, ds, entry.m, entry.m_0, vw, vb, hash_version=2)


@pytest.mark.parametrize("entry", G.TAMPERED, ids=ids)
def test_a_proof_tampered_in_each_named_region_is_refused(oracle, entry):
    import verifier as V

    proof, ds, (vw, vb), inst = G.oracle_proof(oracle, entry)
    pos = G.offsets(proof, entry.m_0, *entry.cfgs())
    assert set(pos) == {"first_commitment"} | {f"{s}/{r}" for s in ("blinding", "witness") for r in ("opening_hint", "final_coeffs", "deferred_hint")}
    for name, off in pos.items():
        bad = bytearray(proof)
        bad[off] ^= 1
        with pytest.raises(V.VerifyError):
            V.verify(bytes(bad), ds, entry.m, entry.m_0, vw, vb, r1cs=(inst.nc, inst.nw, inst.canonical))
            print(f"{entry.id}: a flipped bit in {name} (byte {off}) was accepted")


@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_the_compiled_verifier_accepts_the_oracle_proofs(oracle, entry):
    """libprovekit_verify's host core (no device) on the bytes the device test asks pk_prove for, the matrix evaluation included: its
    statement rule takes every shape pk_scheme_create takes -- folds 5 .. 8 and m = 1 among them"""
    from test_gpu_prove import to_sparse

    from provekit_amd.verify import Verifier

    proof, ds, _, inst = G.oracle_proof(oracle, entry)
    cw, cb = entry.cfgs()
    ver = Verifier(entry.m, entry.m_0, cw, cb)
    try:
        ver.set_r1cs(*(to_sparse(inst.nc, inst.nw, t) for t in inst.trips), inst.interner)
        r = ver.verify(proof)
        assert r.accepted and r.check == "NONE" and r.offset == len(proof), r
        pos = G.offsets(proof, entry.m_0, cw, cb)
        for name in ("witness/final_coeffs", "blinding/final_coeffs", "witness/deferred_hint"):
            bad = bytearray(proof)
            bad[pos[name]] ^= 1
            r = ver.verify(bytes(bad))
            assert not r.accepted and r.check != "NONE" and r.message, (name, r)
    finally:
        ver.close()


def test_the_arena_is_sized_up_to_m_27_and_no_further():
    from provekit_amd.scheme import _cfg_struct

    s = _cfg_struct(G.config(27, 4, 1))
    rc, nbytes = raw_arena_bytes(27, 26, 1 << 26, s)
    assert rc == 0 and nbytes >= 32 * 8 * (1 << 27)
    s.n_vars = 28  # no evaluation domain in the field: n_vars + starting_log_inv_rate <= 28
    assert raw_arena_bytes(28, 26, 1 << 26, s)[0] == -1


def raw_io_pattern(m_0, sw, sb):
    from provekit_amd._lib import lib

    n = C.c_size_t()
    return lib.pk_whir_r1cs_io_pattern(m_0, C.byref(sw), C.byref(sb), None, 0, C.byref(n)), n.value


def raw_arena_bytes(m, m_0, nw, sw):
    from provekit_amd._lib import lib

    n = C.c_size_t()
    return lib.pk_scheme_arena_bytes(m, m_0, nw, C.byref(sw), C.byref(n)), n.value


@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_the_host_entry_points_take_every_grid_config(entry):
    from provekit_amd.scheme import create_io_pattern, io_pattern_check

    cw, cb = entry.cfgs()
    sw, sb = entry.structs()
    rc, n = raw_io_pattern(entry.m_0, sw, sb)
    pattern = create_io_pattern(entry.m_0, cw, cb)
    assert rc == 0 and n == len(pattern) and io_pattern_check(pattern, entry.m_0, cw, cb) == ""
    rc, nbytes = raw_arena_bytes(entry.m, entry.m_0, entry.nw, sw)
    # at least the eight tables of 2^m entries the witness side holds at once: f, g in both forms, c, p, w, the first codeword
    assert rc == 0 and nbytes >= 32 * 8 * (1 << entry.m)


CONFIG_BOUNDS = [b for b in G.BOUNDS if b[5]]


@pytest.mark.parametrize("what,cause,refused,accepted,provable,of_the_config", CONFIG_BOUNDS, ids=[b[0] for b in CONFIG_BOUNDS])
def test_the_host_entry_points_state_the_config_bounds(what, cause, refused, accepted, provable, of_the_config):
    sw, sb = refused.structs()
    assert raw_io_pattern(refused.m_0, sw, sb)[0] == -1, what
    if refused.id.startswith("w-"):  # the arena takes the witness side's config alone
        assert raw_arena_bytes(refused.m, refused.m_0, refused.nw, sw)[0] == -1, what
    if accepted is not None:
        sw, sb = accepted.structs()
        assert raw_io_pattern(accepted.m_0, sw, sb)[0] == 0 and raw_arena_bytes(accepted.m, accepted.m_0, accepted.nw, sw)[0] == 0, what


def test_the_bounds_name_both_sides_of_every_bound_the_issue_lists():
    assert len(G.BOUNDS) == 20 and len(CONFIG_BOUNDS) == 7
    for what, cause, refused, accepted, provable, of_the_config in G.BOUNDS:
        assert refused.id not in {e.id for e in G.GRID} and (accepted is None or (accepted.patch is None and accepted.fits())), what
        assert not provable or accepted is not None, what


def test_the_io_pattern_takes_m_0_from_1_to_27():
    sw, sb = G.M1.structs()
    assert raw_io_pattern(0, sw, sb)[0] == -1 and raw_io_pattern(1, sw, sb)[0] == 0
    sb27 = G.Entry("", 9, 27, 0, 0, G.F2, G.F2).structs()[1]  # 8 variables
    assert sb27.n_vars == 8 and raw_io_pattern(27, sw, sb27)[0] == 0 and raw_io_pattern(28, sw, sb27)[0] == -1
