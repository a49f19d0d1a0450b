"""CPU: libprovekit_whir.so's host side.  The header/library/binding symbol match; pkw_verify on opening proofs the ORACLE prover
builds (oracle/prover_ref.py's parts over pkw_io_pattern's bytes): acceptance with the evaluations of oracle/verifier.py's
mle_eval_table, every tampering with the verdict it must give, hostile framing."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
HEADER = os.path.join(ROOT, "include", "provekit_whir.h")

import whir_pcs_cases as K  # noqa: E402

STRUCTURAL = {"TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT"}


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import verify, whir_pcs

    def declared_in(name):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        return sorted(set(re.findall(r"\b(pkw_[a-z0-9_]+)\s*\(", src)))

    nm = subprocess.run(["nm", "-D", "--defined-only", whir_pcs.WHIR_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkw_[a-z0-9_]+)$", nm, flags=re.M)))
    declared = declared_in("provekit_whir.h")  # the header's own text: what it includes is the linear test's
    assert len(declared) == 15 and set(declared) <= set(exported) and set(declared) <= set(whir_pcs.SIGNATURES)
    # the whole: the four topical headers between them declare what the one library exports and the one table binds
    topics = [declared, declared_in("provekit_whir_linear.h"), declared_in("provekit_whir_sparse.h"), declared_in("provekit_whir_hiding.h")]
    assert [len(t) for t in topics] == [15, 4, 5, 7]
    assert all(not set(a) & set(b) for i, a in enumerate(topics) for b in topics[i + 1 :])
    assert sorted(sum(topics, [])) == exported == sorted(whir_pcs.SIGNATURES) and len(exported) == 31
    assert ctypes.CDLL(whir_pcs.WHIR_LIB_PATH).pkw_abi_version() == 1
    assert [whir_pcs.lib.pkw_check_name(i).decode() for i in range(len(whir_pcs.CHECKS))] == list(whir_pcs.CHECKS)
    assert whir_pcs.CHECKS[: len(verify.CHECKS)] == verify.CHECKS  # the walk's verdicts keep the verifier's numbers
    # the library calls the product only through its C ABI
    und = subprocess.run(["nm", "-D", "--undefined-only", whir_pcs.WHIR_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\bpkv_\w+", und), und


def test_io_pattern_lists_the_operations_and_configs_are_refused_with_a_reason():
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    cfg = K.small_config(8, 2)
    pat = whir_pcs.io_pattern(cfg, 3)
    parts = pat.split(b"\0")
    assert parts[0] == b"provekit-hip/whir-pcs/v1"
    assert parts[1:7] == [b"A1merkle_digest", b"S1ood_query", b"A2ood_ans", b"S1batching_randomness", b"A24points", b"A6evaluations"]
    assert parts[-1] == b"Hdeferred_weight_evaluations"
    assert whir_pcs.io_pattern(cfg, 4) != pat and whir_pcs.io_pattern(K.small_config(8, 1), 3) != pat
    assert whir_pcs.arena_bytes(cfg) > 32 * 5 * 256
    for q in (0, 65):
        with pytest.raises(ProveKitHipError, match="1..64"):
            whir_pcs.io_pattern(cfg, q)
    bad = K.small_config(8, 2)
    bad.batch_size = 5
    with pytest.raises(ProveKitHipError):
        whir_pcs.io_pattern(bad, 1)
    bad = K.small_config(8, 2)
    bad.folding_factor = 5  # the product's pattern takes it (n_vars >= 5 * 2 fails first there); either way a reason comes back
    with pytest.raises(ProveKitHipError) as e:
        whir_pcs.arena_bytes(bad)
    assert str(e.value)


class Case:
    def __init__(self, oracle, n_vars, batch, q):
        from provekit_amd import whir_pcs

        self.cfg = K.small_config(n_vars, batch)
        self.n, self.batch, self.q = n_vars, batch, q
        self.polys = K.polynomials(n_vars, batch)
        self.pts = K.points(n_vars, q)
        self.mpts = K.mont_points(oracle, self.pts)
        self.pattern = whir_pcs.io_pattern(self.cfg, q)
        self.proof, self.root, self.vals = K.oracle_opening(oracle, self.cfg, self.polys, self.pts, self.pattern)
        self.eval_offset = 32 + 32 * self.cfg.commitment_ood_samples * batch + 32 * q * n_vars

    def verify(self, proof=None, **kw):
        from provekit_amd import whir_pcs

        kw.setdefault("expected_root", self.root)
        pts = kw.pop("points", self.mpts)
        return whir_pcs.verify(self.cfg, pts, self.proof if proof is None else proof, **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    return {s: Case(oracle, *s) for s in K.SHAPES}


@pytest.mark.parametrize("shape", K.SHAPES)
def test_oracle_built_openings_are_accepted_with_the_oracles_evaluations(oracle, cases, shape):
    c = cases[shape]
    for kw in ({}, {"io_pattern": c.pattern}, {"expected_root": None}):
        r, evals = c.verify(**kw)
        assert r.accepted and r.check == "NONE" and r.offset == len(c.proof), r
        got = oracle.limbs_to_ints(oracle.from_mont(evals.reshape(-1, 4)))
        assert got == [v for row in c.vals for v in row]
    assert c.vals == K.expected_evals(c.polys, c.pts)


@pytest.mark.parametrize("shape", [(8, 2, 3), (12, 1, 3)])
def test_every_tampering_is_rejected_with_its_check(oracle, cases, shape):
    from provekit_amd import whir_pcs

    c = cases[shape]
    assert c.verify()[0].accepted

    def flipped(off):
        t = bytearray(c.proof)
        t[off] ^= 1
        return bytes(t)

    other_points = c.mpts.copy()
    other_points[c.q - 1, c.n - 1] = oracle.to_mont(oracle.ints_to_limbs([12345]))[0]
    wrong_root = bytes([c.root[0] ^ 1]) + c.root[1:]
    expect = {
        "one evaluation changed in the proof": (dict(proof=flipped(c.eval_offset + 32 * (c.q * c.batch - 1))), "WHIR_SUMCHECK"),
        "one point changed in the proof": (dict(proof=flipped(c.eval_offset - 32)), "POINTS"),
        "one point changed in the call": (dict(points=other_points), "POINTS"),
        "a wrong expected root": (dict(expected_root=wrong_root), "ROOT"),
        "a deferred value changed": (dict(proof=flipped(K.deferred_offset(c.proof, c.q) + 32 * (c.q - 1))), "WHIR_FINAL"),
        "truncated by 1 byte": (dict(proof=c.proof[:-1]), "TRANSCRIPT_SHORT"),
        "one appended byte": (dict(proof=c.proof + b"\0"), "TRAILING_BYTES"),
        "a pattern for q + 1": (dict(io_pattern=whir_pcs.io_pattern(c.cfg, c.q + 1)), "IO_PATTERN"),
        "the root changed in the proof": (dict(proof=flipped(0), expected_root=None), "WHIR_SUMCHECK"),
        "the other hash version": (dict(hash_version=1), "MERKLE"),
    }
    for name, (kw, check) in expect.items():
        r, _ = c.verify(**kw)
        print(f"{name}: {r}")
        assert not r.accepted and r.check == check and r.message, (name, r)


def test_weights_of_other_points_than_the_statements_fail_the_deferred_check(oracle):
    """a prover that runs WHIR honestly, but over the weights of ANOTHER point than the one it put on the transcript, and claims
    the evaluations there: every WHIR relation holds, the deferred value is eq(other point, folding point) -- only the
    verifier's own recomputation of eq(point, folding point) can tell"""
    from provekit_amd import whir_pcs

    n, batch, q = 8, 1, 1
    cfg = K.small_config(n, batch)
    polys, pts = K.polynomials(n, batch), K.points(n, q)
    other = K.points(n, q, seed=77)
    proof, root, _ = K.oracle_opening(oracle, cfg, polys, pts, whir_pcs.io_pattern(cfg, q), weight_points=other, claimed=K.expected_evals(polys, other))
    r, _ = whir_pcs.verify(cfg, K.mont_points(oracle, pts), proof, expected_root=root)
    assert not r.accepted and r.check == "DEFERRED", r
    # ... and claiming the true evaluations at `pts` over those weights fails inside WHIR already
    proof, root, _ = K.oracle_opening(oracle, cfg, polys, pts, whir_pcs.io_pattern(cfg, q), weight_points=other)
    r, _ = whir_pcs.verify(cfg, K.mont_points(oracle, pts), proof, expected_root=root)
    assert not r.accepted and r.check == "WHIR_SUMCHECK", r


def test_hostile_framing_is_rejected_structurally(cases):
    c = cases[(8, 2, 3)]
    hostile = {"zero length": b"", "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes()}
    d0 = K.deferred_offset(c.proof, c.q)
    for e in (32, 63):
        t = bytearray(c.proof)
        struct.pack_into("<Q", t, d0 - 8, 1 << e)  # the Vec<F> count of the deferred hint
        hostile[f"deferred count = 2^{e}"] = bytes(t)
    t = bytearray(c.proof)
    struct.pack_into("<I", t, d0 - 12, 0xFFFFFFFF)
    hostile["hint length = 2^32 - 1"] = bytes(t)
    # the first hint of the proof (stir_answers of round 0): its leaf count
    first_hint = c.eval_offset + 32 * c.q * c.batch + 32 * 3 * c.cfg.folding_factor + 32 + 32 * c.cfg.ood_samples[0] + 8
    (ln,) = struct.unpack_from("<I", c.proof, first_hint)
    (k,) = struct.unpack_from("<Q", c.proof, first_hint + 4)
    assert 0 < k <= c.cfg.num_queries[0] and ln == 8 + k * (8 + 32 * c.batch * 16), "the layout walk missed the stir_answers hint"
    for e in (32, 40, 63):
        t = bytearray(c.proof)
        struct.pack_into("<Q", t, first_hint + 4, 1 << e)
        hostile[f"leaf count = 2^{e}"] = bytes(t)
    for name, proof in hostile.items():
        r, _ = c.verify(proof=proof)
        assert not r.accepted and r.check in STRUCTURAL and r.message, (name, r)
