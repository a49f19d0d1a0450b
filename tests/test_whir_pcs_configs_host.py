"""CPU: pkw_verify over the grid of whir_pcs_config_cases.py -- every fold, rate, batch, round count, OOD count and grinding position
the library accepts -- on openings the ORACLE prover builds: acceptance with the oracle's evaluations, the linear and the sparse
statement on their subset, tampering at the regions the other suites' configs do not have (a final sumcheck, no OOD sample, a last
tree of two leaves), and the bounds of the family with the accepted neighbour of each."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_config_cases as G  # noqa: E402
import whir_pcs_sparse_cases as S  # noqa: E402

ids = lambda e: e.id if isinstance(e, G.Entry) else None  # noqa: E731


def ints(oracle, limbs):
    return oracle.limbs_to_ints(oracle.from_mont(limbs.reshape(-1, 4)))


def test_the_grid_reaches_every_shape_it_names():
    """rounds 0..8, final polynomials of 0, 1, 2, 5 and 6 variables, every fold, batch, OOD count and grinding position"""
    cfgs = [e.cfg() for e in G.GRID]
    assert len(G.FOLD_EDGES) == 19 and len(G.GRID) == 41
    assert {c.n_rounds for c in cfgs} >= {0, 1, 2, 3, 4, 7, 8}
    assert {e.final_vars() for e in G.GRID} == {0, 1, 2, 5, 6}
    assert {(c.folding_factor, c.batch_size) for c in cfgs} >= {(k, 1) for k in (1, 2, 3, 4)} | {(2, 3), (3, 4), (4, 3), (4, 4), (1, 2)}
    assert {c.starting_log_inv_rate for c in cfgs} == {1, 2, 3}
    assert {c.commitment_ood_samples for c in cfgs} == {0, 1, 2, 4} == {o for c in cfgs for o in c.ood_samples}
    assert max(c.n_vars for c in cfgs) == 14
    grinds = {(bool(c.n_rounds and c.pow_bits[0]), bool(c.final_pow_bits), bool(c.final_folding_pow_bits)) for c in cfgs if c.n_rounds}
    assert grinds >= {(True, False, False), (False, True, False), (False, False, True), (False, False, False), (True, True, True)}


@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_oracle_built_openings_are_accepted_at_every_config(oracle, entry):
    from provekit_amd import whir_pcs

    o = G.opening(oracle, entry)
    want = K.expected_evals(o.polys, o.pts)
    assert o.vals == want
    for kw in ({"io_pattern": o.pattern}, {}):  # the pattern passed and defaulted
        r, evals = whir_pcs.verify(o.cfg, o.mpts, o.proof, expected_root=o.root, **kw)
        assert r.accepted and r.check == "NONE" and r.offset == len(o.proof), r
        assert ints(oracle, evals) == [v for row in want for v in row]
    G.walk(o.proof, o.cfg, o.q)  # the layout the tampering tests and the device tests' reports rely on


@pytest.mark.parametrize("entry", G.GRID, ids=ids)
def test_the_arena_is_the_sum_of_an_openings_buffers(entry):
    """pkw_scheme_arena_bytes (plan() in csrc/whir_pcs/pcs.hpp) against the buffers of an opening, listed from its steps: a buffer
    plan() forgets is PK_ERR_OOM from pkw_open on the device, one it counts twice is memory no opening uses"""
    from provekit_amd import whir_pcs

    cfg = entry.cfg()
    assert whir_pcs.arena_bytes(cfg) == 32 * G.arena_fes(cfg), G.opening_buffers(cfg)


@pytest.mark.parametrize("entry,weights", G.INITIAL_WEIGHTS, ids=ids)
def test_the_initial_weight_counts_straddle_the_chunk_of_32(oracle, entry, weights):
    c = entry.cfg()
    assert c.commitment_ood_samples + entry.q == weights and weights in (32, 33, 68)


@pytest.mark.parametrize("entry,distinct", G.ROUND_WEIGHTS, ids=ids)
def test_the_round_weight_counts_straddle_the_chunk_of_32(oracle, entry, distinct):
    """a condition of the device test of the same entries: the oracle's transcript draws this many distinct STIR indexes"""
    o = G.opening(oracle, entry)
    asked, got, rows = o.counts[0]
    assert (asked, rows) == (o.cfg.num_queries[0], 64) and got == distinct
    assert o.cfg.ood_samples[0] + got in (31, 32, 33, 34)


def test_the_all_rows_entry_opens_every_row(oracle):
    o = G.opening(oracle, G.ALL_ROWS)
    assert o.counts[0] == (400, 32, 32)


@pytest.mark.parametrize("q,l", G.LINEAR_COUNTS)
@pytest.mark.parametrize("entry", G.LINEAR, ids=ids)
def test_linear_and_sparse_statements_are_accepted_with_and_without_the_tables(oracle, entry, q, l):
    from provekit_amd import whir_pcs

    o = G.linear_opening(oracle, entry, q, l)
    want_sums = [s for row in o.sums for s in row]
    want_evals = [v for row in o.vals for v in row]
    for kw in ({"io_pattern": o.pattern}, {}):
        v = whir_pcs.verify_linear(o.cfg, o.mpts, o.mtags, o.mdense, o.proof, expected_root=o.root, **kw)
        assert v.result.accepted and v.result.check == "NONE" and v.result.offset == len(o.proof) and v.unchecked == 0, v.result
        assert ints(oracle, v.sums) == want_sums and ints(oracle, v.evals) == want_evals
    bare = whir_pcs.verify_linear(o.cfg, o.mpts, o.mtags, None, o.proof, expected_root=o.root)
    assert bare.result.accepted and bare.result.offset == len(o.proof) and bare.unchecked == l, bare.result
    point = ints(oracle, bare.fold_point)
    assert ints(oracle, bare.deferred) == S.evaluate(o.n, o.ws, point)  # what the caller would have to check
    s = whir_pcs.verify_sparse(o.cfg, o.mpts, o.mtags, S.pack(oracle, o.ws), o.proof, expected_root=o.root)
    assert s.result.accepted and s.result.check == "NONE" and s.result.offset == len(o.proof), s.result
    assert ints(oracle, s.sums) == want_sums and ints(oracle, s.deferred) == ints(oracle, bare.deferred)


def neighbours(entry):
    """configs whose pattern differs: one more round where the family has it (else one fewer), and grinding toggled"""
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    c = entry.cfg()
    out = {}
    for rounds in (c.n_rounds + 1, c.n_rounds - 1):
        try:
            n = G.config(*entry.args, **dict(entry.kw, rounds=rounds))
            whir_pcs.io_pattern(n, entry.q)
        except ProveKitHipError:
            continue
        out[f"{rounds} rounds"] = n
        break
    out["grinding toggled"] = G.config(*entry.args, **dict(entry.kw, grind=not entry.kw.get("grind", True)))
    assert len(out) == 2
    return out


@pytest.mark.parametrize("entry", G.TAMPERED, ids=ids)
def test_every_tampering_is_rejected_with_its_check(oracle, entry):
    from provekit_amd import whir_pcs

    o = G.opening(oracle, entry)
    pos = G.offsets(o.proof, o.cfg, o.q)
    final_vars = entry.final_vars()

    def verify(proof=o.proof, **kw):
        return whir_pcs.verify(o.cfg, o.mpts, proof, expected_root=o.root, **kw)[0]

    def flipped(off):
        t = bytearray(o.proof)
        t[off] ^= 1
        return bytes(t)

    assert verify().accepted
    expect = {
        "a leaf element of the first tree": (dict(proof=flipped(pos["first_tree_leaf"])), {"MERKLE"}),
        "a leaf element of the last tree": (dict(proof=flipped(pos["last_tree_leaf"])), {"MERKLE"}),
        "a deferred value": (dict(proof=flipped(pos["deferred_value"])), {"WHIR_FINAL"}),
        "a final coefficient": (dict(proof=flipped(pos["final_coeffs"])), None),
        "truncated by 1 byte": (dict(proof=o.proof[:-1]), None),
        "one appended byte": (dict(proof=o.proof + b"\0"), None),
    }
    if final_vars:
        assert entry is G.FINAL_SUMCHECK and final_vars == 5
        # the message of final round t is checked against the claim round t - 1 left: the walk's sumcheck relation
        expect["the first final-sumcheck polynomial"] = (dict(proof=flipped(pos["final_sumcheck"])), {"WHIR_SUMCHECK"})
        expect["the last final-sumcheck polynomial"] = (dict(proof=flipped(pos["final_sumcheck"] + 96 * (final_vars - 1) + 64)), {"WHIR_FINAL"})
    else:
        assert "final_sumcheck" not in pos
    for name, cfg in neighbours(entry).items():
        expect[f"the pattern of the neighbour with {name}"] = (dict(io_pattern=whir_pcs.io_pattern(cfg, o.q)), {"IO_PATTERN"})
    for name, (kw, checks) in expect.items():
        r = verify(**kw)
        print(f"{entry.id}: {name}: {r}")
        assert not r.accepted and r.check != "NONE" and r.message, (name, r)
        if checks is not None:
            assert r.check in checks and len(checks) == 1, (name, r)


@pytest.mark.parametrize("what,refused,accepted,runnable", G.BOUNDS, ids=[b[0] for b in G.BOUNDS])
def test_the_bounds_of_the_family_refuse_with_a_reason_and_accept_the_neighbour(what, refused, accepted, runnable):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    bad = G.config(*refused[0], **refused[1])
    for call in (lambda c: whir_pcs.io_pattern(c, 2), whir_pcs.arena_bytes):
        with pytest.raises(ProveKitHipError) as e:
            call(bad)
        assert e.value.code == -1 and str(e.value).strip() and whir_pcs.lib.pkw_create_error(), what
    good = G.config(*accepted[0], **accepted[1])
    pattern = whir_pcs.io_pattern(good, 2)
    assert pattern.startswith(b"provekit-hip/whir-pcs/v1\0") and pattern != whir_pcs.io_pattern(good, 3)
    assert whir_pcs.arena_bytes(good) >= 32 * 3 * (1 << good.n_vars)
