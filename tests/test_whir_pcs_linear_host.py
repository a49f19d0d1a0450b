"""CPU: the linear statements of libprovekit_whir.so on the host.  The symbols; pkw_io_pattern_linear's operations and refusals;
pkw_verify_linear on openings the ORACLE prover builds (oracle/prover_ref.py's parts over pkw_io_pattern_linear's bytes), with the
weight tables given and withheld; every tampering with the verdict it must give; the register tile's arithmetic on the host at the
column bound; hostile framing through the sanitizer build of the host verifier (a program of its own, run as a subprocess)."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
HEADER = os.path.join(ROOT, "include", "provekit_whir.h")
LINEAR_HEADER = os.path.join(ROOT, "include", "provekit_whir_linear.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkw_verify_asan")

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_linear_cases as L  # noqa: E402

STRUCTURAL = {"TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT"}
LINEAR = ["pkw_io_pattern_linear", "pkw_open_linear", "pkw_verify_linear", "pkw_weighted_sums"]


def test_the_linear_header_declares_four_names_the_library_exports_and_the_binding_binds():
    """the four C names live in include/provekit_whir_linear.h (which provekit_whir.h includes); libprovekit_whir.so exports them"""
    from provekit_amd import whir_pcs

    def declared_in(path):
        return sorted(set(re.findall(r"\b(pkw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))))

    def exported_by(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(set(re.findall(r" [A-Za-z] (pkw_[a-z0-9_]+)$", nm, flags=re.M)))

    assert declared_in(LINEAR_HEADER) == sorted(LINEAR) and len(LINEAR) == 4
    assert set(LINEAR) <= set(exported_by(whir_pcs.WHIR_LIB_PATH)) and set(LINEAR) <= set(whir_pcs.SIGNATURES)
    assert exported_by(whir_pcs.WHIR_LIB_PATH) == sorted(whir_pcs.SIGNATURES)
    assert re.search(r'^#include "provekit_whir_linear.h"', open(HEADER).read(), flags=re.M)
    assert re.search(r"#define PKW_MAX_WEIGHTS 16\b", open(LINEAR_HEADER).read()) and whir_pcs.MAX_WEIGHTS == 16
    assert ctypes.CDLL(whir_pcs.WHIR_LIB_PATH).pkw_abi_version() == 1  # additive: the ABI version and every verdict number stay
    assert [whir_pcs.lib.pkw_check_name(i).decode() for i in range(len(whir_pcs.CHECKS))] == list(whir_pcs.CHECKS)
    assert whir_pcs.CHECKS[-3:] == ("POINTS", "ROOT", "DEFERRED")


@pytest.mark.parametrize("q,l", [(0, 1), (2, 3), (64, 16)])
def test_io_pattern_linear_lists_the_operations(q, l):
    from provekit_amd import whir_pcs

    cfg = K.small_config(8, 2)
    parts = whir_pcs.io_pattern_linear(cfg, q, l).split(b"\0")
    assert parts[0] == b"provekit-hip/whir-pcs-linear/v1"
    want = [b"A1merkle_digest", b"S1ood_query", b"A2ood_ans", b"S1batching_randomness"]
    if q:
        want.append(b"A%dpoints" % (8 * q))
    want.append(b"A%dtags" % l)
    if q:
        want.append(b"A%devaluations" % (2 * q))
    want += [b"A%dsums" % (2 * l), b"S1initial_combination_randomness"]
    assert parts[1 : 1 + len(want)] == want
    assert parts[-1] == b"Hdeferred_weight_evaluations"
    # what follows the statement is the WHIR proof's pattern, the one pkw_io_pattern ends in
    tail = whir_pcs.io_pattern(cfg, 1).split(b"\0")
    at = tail.index(b"S1initial_combination_randomness")
    assert parts[len(want) :] == tail[at:]
    single = whir_pcs.io_pattern_linear(K.small_config(8, 1), q, l).split(b"\0")
    assert b"S1batching_randomness" not in single and b"A%dsums" % l in single


def test_io_pattern_linear_refuses_counts_out_of_range_with_a_reason():
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    cfg = K.small_config(8, 2)
    for q, l, why in ((1, 0, "1..16"), (1, 17, "1..16"), (65, 1, "0..64")):
        with pytest.raises(ProveKitHipError, match=why) as e:
            whir_pcs.io_pattern_linear(cfg, q, l)
        assert e.value.code == -1  # PK_ERR_BAD_ARG
    r = whir_pcs.ResultStruct()
    c = whir_pcs._cfg_struct(cfg)
    tags = np.zeros((17, 4), dtype=np.uint64)
    pts = np.zeros((65, 8, 4), dtype=np.uint64)
    for q, l, why in ((1, 0, b"1..16"), (1, 17, b"1..16"), (65, 1, b"0..64")):
        rc = whir_pcs.lib.pkw_verify_linear(ctypes.addressof(c), None, 0, 2, None, pts.ctypes.data, q, tags.ctypes.data, None, l, b"x", 1, None, None, None,
                                            None, None, ctypes.byref(r))
        assert rc == -1 and why in whir_pcs.lib.pkw_create_error()


class Case:
    def __init__(self, oracle, n_vars, batch, q, l):
        from provekit_amd import whir_pcs

        self.cfg = K.small_config(n_vars, batch)
        self.n, self.batch, self.q, self.l = n_vars, batch, q, l
        self.polys = K.polynomials(n_vars, batch)
        self.pts = K.points(n_vars, q) if q else []
        self.mpts = K.mont_points(oracle, self.pts) if q else None
        self.weights = L.weight_tables(oracle, n_vars, l)
        self.mweights = [L.mont(oracle, w) for w in self.weights]
        self.tags = L.tags(l)
        self.mtags = L.mont(oracle, self.tags)
        self.pattern = whir_pcs.io_pattern_linear(self.cfg, q, l)
        self.proof, self.root, self.vals, self.sums = L.oracle_linear_opening(oracle, self.cfg, self.polys, self.pts, self.weights, self.tags, self.pattern)
        self.tag_offset = 32 + 32 * self.cfg.commitment_ood_samples * batch + 32 * q * n_vars
        self.sum_offset = self.tag_offset + 32 * l + 32 * q * batch

    def verify(self, proof=None, **kw):
        from provekit_amd import whir_pcs

        kw.setdefault("expected_root", self.root)
        weights = kw.pop("weights", self.mweights)
        tags = kw.pop("tags", self.mtags)
        return whir_pcs.verify_linear(self.cfg, self.mpts, tags, weights, self.proof if proof is None else proof, **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    return {s: Case(oracle, *s) for s in L.SHAPES}


@pytest.mark.parametrize("shape", L.SHAPES)
def test_oracle_built_linear_openings_are_accepted_with_and_without_the_tables(oracle, cases, shape):
    import verifier as V

    c = cases[shape]
    assert c.sums == L.expected_sums(c.polys, c.weights)  # Python-int inner products
    for kw in ({}, {"io_pattern": c.pattern}, {"expected_root": None}):
        v = c.verify(**kw)
        assert v.result.accepted and v.result.check == "NONE" and v.result.offset == len(c.proof), v.result
        assert v.unchecked == 0
        assert oracle.limbs_to_ints(oracle.from_mont(v.sums.reshape(-1, 4))) == [s for row in c.sums for s in row]
        if c.q:
            assert oracle.limbs_to_ints(oracle.from_mont(v.evals.reshape(-1, 4))) == [x for row in c.vals for x in row]
    v = c.verify(weights=None)
    assert v.result.accepted and v.result.offset == len(c.proof) and v.unchecked == c.l, v.result
    fold = oracle.limbs_to_ints(oracle.from_mont(v.fold_point))
    got = oracle.limbs_to_ints(oracle.from_mont(v.deferred))
    assert got == [V.mle_eval_table(w, fold) for w in c.weights]  # the condition the caller closes
    if c.l >= 2:  # tables for some weights only: the others are counted
        some = [c.mweights[0]] + [None] * (c.l - 1)
        v = c.verify(weights=some)
        assert v.result.accepted and v.unchecked == c.l - 1


@pytest.mark.parametrize("shape", [(8, 2, 2, 3), (12, 1, 1, 2)])
def test_every_tampering_of_a_linear_opening_is_rejected_with_its_check(oracle, cases, shape):
    from provekit_amd import whir_pcs

    c = cases[shape]
    assert c.verify().result.accepted

    def flipped(off):
        t = bytearray(c.proof)
        t[off] ^= 1
        return bytes(t)

    other_tags = c.mtags.copy()
    other_tags[c.l - 1] = L.mont(oracle, [424242])[0]
    other_table = list(c.mweights)
    other_table[c.l - 1] = c.mweights[c.l - 1].copy()
    other_table[c.l - 1][5] = L.mont(oracle, [77])[0]
    d0 = L.deferred_offset(c.proof, c.q + c.l)
    expect = {
        "one sum changed in the proof": (dict(proof=flipped(c.sum_offset + 32 * (c.l * c.batch - 1))), "WHIR_SUMCHECK"),
        "one tag changed in the proof": (dict(proof=flipped(c.tag_offset + 32 * (c.l - 1))), "POINTS"),
        "one tag changed in the call": (dict(tags=other_tags), "POINTS"),
        "a weight's deferred value changed": (dict(proof=flipped(d0 + 32 * (c.q + c.l - 1))), "WHIR_FINAL"),
        "a weight's deferred value changed, tables withheld": (dict(proof=flipped(d0 + 32 * (c.q + c.l - 1)), weights=None), "WHIR_FINAL"),
        "another table for the last weight": (dict(weights=other_table), "DEFERRED"),
        "a pattern for l + 1": (dict(io_pattern=whir_pcs.io_pattern_linear(c.cfg, c.q, c.l + 1)), "IO_PATTERN"),
        "truncated by 1 byte": (dict(proof=c.proof[:-1]), "TRANSCRIPT_SHORT"),
        "one appended byte": (dict(proof=c.proof + b"\0"), "TRAILING_BYTES"),
    }
    for name, (kw, check) in expect.items():
        v = c.verify(**kw)
        print(f"{name}: {v.result}")
        assert not v.result.accepted and v.result.check == check and v.result.message, (name, v.result)
    v = c.verify(tags=other_tags)
    assert f"tag {c.l - 1}" in v.result.message
    v = c.verify(weights=other_table)
    assert f"weight {c.l - 1}" in v.result.message and v.unchecked == 0


def test_a_proof_run_over_another_weight_than_the_verifiers_fails_the_deferred_check(oracle):
    """a prover that runs WHIR honestly, but over ANOTHER table than the one the verifier holds for the tag, and claims that
    table's true sums: every WHIR relation holds, the deferred value is the other table's extension at the folding point -- only
    the verifier's own pass over its table can tell.  Without the table the verdict is conditional, and the condition fails."""
    import verifier as V
    from provekit_amd import whir_pcs

    n, batch, q, l = 8, 1, 0, 1
    cfg = K.small_config(n, batch)
    polys = K.polynomials(n, batch)
    mine, other = L.weight_tables(oracle, n, 1), L.weight_tables(oracle, n, 1, seed=99)
    tg = L.tags(l)
    proof, root, _, _ = L.oracle_linear_opening(oracle, cfg, polys, [], mine, tg, whir_pcs.io_pattern_linear(cfg, q, l), prove_weights=other,
                                                claimed_sums=L.expected_sums(polys, other))
    v = whir_pcs.verify_linear(cfg, None, L.mont(oracle, tg), [L.mont(oracle, mine[0])], proof, expected_root=root)
    assert not v.result.accepted and v.result.check == "DEFERRED" and "weight 0" in v.result.message, v.result
    v = whir_pcs.verify_linear(cfg, None, L.mont(oracle, tg), None, proof, expected_root=root)
    assert v.result.accepted and v.unchecked == 1
    fold = oracle.limbs_to_ints(oracle.from_mont(v.fold_point))
    assert oracle.limbs_to_ints(oracle.from_mont(v.deferred)) == [V.mle_eval_table(other[0], fold)] != [V.mle_eval_table(mine[0], fold)]
    # ... and claiming the verifier's table's sums over the other table fails inside WHIR already
    proof, root, _, _ = L.oracle_linear_opening(oracle, cfg, polys, [], mine, tg, whir_pcs.io_pattern_linear(cfg, q, l), prove_weights=other)
    v = whir_pcs.verify_linear(cfg, None, L.mont(oracle, tg), [L.mont(oracle, mine[0])], proof, expected_root=root)
    assert not v.result.accepted and v.result.check == "WHIR_SUMCHECK", v.result


@pytest.mark.parametrize("terms", range(1, 10))
def test_the_register_tile_on_the_host_at_the_column_bound(terms):
    """the kernel's accumulate / flush / result code (fe29.hpp's dot29 under csrc/whir_pcs/linear_tile.hpp), compiled for the host:
    every operand p - 1, 1 to 9 products -- every phase of a DOT29_GROUP = 4 reduction group, two groups and a rest"""
    import pk_probes

    R_INV = pow(1 << 256, -1, K.P)
    ops = np.frombuffer((K.P - 1).to_bytes(32, "little") * (2 * terms), dtype="<u8").copy()
    out = np.zeros(16, dtype=np.uint64)
    assert pk_probes.lib.pk_probe_wsum_tile_host(ops.ctypes.data, ops.ctypes.data, terms, out.ctypes.data) == 0
    got = [int.from_bytes(out[4 * i : 4 * i + 4].tobytes(), "little") for i in range(4)]
    assert got == [terms * (K.P - 1) ** 2 * R_INV % K.P] * 4


def test_the_register_tile_on_the_host_with_distinct_operands():
    import pk_probes

    terms, R_INV = 7, pow(1 << 256, -1, K.P)
    f = [K.random_ints(terms, 50 + u) for u in range(2)]
    w = [K.random_ints(terms, 60 + v) for v in range(2)]
    f[0][2] = (1 << 256) - 1  # the first factor may be any 256-bit value
    pack = lambda rows: np.frombuffer(b"".join(x.to_bytes(32, "little") for r in rows for x in r), dtype="<u8").copy()  # noqa: E731
    out = np.zeros(16, dtype=np.uint64)
    assert pk_probes.lib.pk_probe_wsum_tile_host(pack(f).ctypes.data, pack(w).ctypes.data, terms, out.ctypes.data) == 0
    got = [int.from_bytes(out[4 * i : 4 * i + 4].tobytes(), "little") for i in range(4)]
    assert got == [sum(a * b for a, b in zip(f[u], w[v])) * R_INV % K.P for u in range(2) for v in range(2)]


def test_hostile_framing_is_rejected_structurally_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan):
    counts and lengths no proof of this size can hold, with the tables given (the table pass runs on the honest case)"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkw_verify_asan is missing: make -C provekit_amd/csrc asan"
    from provekit_amd import whir_pcs

    c = cases[(8, 2, 2, 3)]
    d0 = L.deferred_offset(c.proof, c.q + c.l)
    hostile = {"honest": c.proof, "zero length": b"",
               "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes()}
    for e in (32, 63):
        t = bytearray(c.proof)
        struct.pack_into("<Q", t, d0 - 8, 1 << e)  # the Vec<F> count of the deferred hint
        hostile[f"deferred count = 2^{e}"] = bytes(t)
    for count in (c.q, c.q + c.l + 1):  # a hint that holds only the points' values; one value too many
        t = bytearray(c.proof[: d0 - 12]) + struct.pack("<IQ", 8 + 32 * count, count) + bytes(32 * count)
        hostile[f"deferred count = {count}"] = bytes(t)
    t = bytearray(c.proof)
    struct.pack_into("<I", t, d0 - 12, 0xFFFFFFFF)
    hostile["hint length = 2^32 - 1"] = bytes(t)
    first_hint = c.sum_offset + 32 * c.l * c.batch + 32 * 3 * c.cfg.folding_factor + 32 + 32 * c.cfg.ood_samples[0] + 8
    (ln,) = struct.unpack_from("<I", c.proof, first_hint)
    (k,) = struct.unpack_from("<Q", c.proof, first_hint + 4)
    assert 0 < k <= c.cfg.num_queries[0] and ln == 8 + k * (8 + 32 * c.batch * 16), "the layout walk missed the stir_answers hint"
    for e in (32, 40, 63):
        t = bytearray(c.proof)
        struct.pack_into("<Q", t, first_hint + 4, 1 << e)
        hostile[f"leaf count = 2^{e}"] = bytes(t)
    hostile["truncated inside the sums"] = c.proof[: c.sum_offset + 40]
    hostile["truncated inside the tags"] = c.proof[: c.tag_offset + 7]

    cs = whir_pcs._cfg_struct(c.cfg)
    blob = struct.pack("<4I", 2, c.q, c.l, 1) + bytes(cs) + struct.pack("<I", len(c.pattern)) + c.pattern
    blob += c.mpts.tobytes() + c.mtags.tobytes() + b"".join(w.tobytes() for w in c.mweights)
    blob += struct.pack("<I", len(hostile)) + b"".join(struct.pack("<Q", len(p)) + p for p in hostile.values())
    f = tmp_path / "cases.bin"
    f.write_bytes(blob)
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    p = subprocess.run([ASAN, "linear", str(f)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(hostile)
    for (name, proof), line in zip(hostile.items(), lines):
        accepted, check, offset, unchecked = line.split()
        if name == "honest":
            assert (accepted, check, int(offset), unchecked) == ("1", "NONE", len(proof), "0"), line
        else:
            assert accepted == "0" and check in STRUCTURAL, (name, line)
        # the library loaded into this process gives the same verdict
        v = c.verify(proof=proof, expected_root=None)
        assert (str(int(v.result.accepted)), v.result.check, v.result.offset) == (accepted, check, int(offset)), (name, line, v.result)
