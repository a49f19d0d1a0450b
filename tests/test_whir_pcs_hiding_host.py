"""CPU: hiding openings on the host (include/provekit_whir_hiding.h).  The symbols; the hiding pattern;
pkw_verify_hiding on openings the ORACLE prover builds over host-built extended tables [f_b || mask_b], g -- acceptance with
f_b(z_i) of oracle/verifier.py's mle_eval_table, the same bytes accepted by plain pkw_verify as a proof of the extended statement,
every tampering with the verdict it must give; the two config rules; truncated proofs and hostile counts through the sanitizer
build (a program of its own, run as a subprocess)."""
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
HIDING_HEADER = os.path.join(ROOT, "include", "provekit_whir_hiding.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkw_verify_asan")

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_hiding_cases as H  # noqa: E402

HIDING = ["pkw_commit_hiding", "pkw_hiding_commitment_destroy", "pkw_hiding_commitment_root", "pkw_hiding_scheme_create", "pkw_io_pattern_hiding",
          "pkw_open_hiding", "pkw_verify_hiding"]
STRUCTURAL = {"TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT"}


def test_the_hiding_header_declares_seven_names_the_library_exports_and_the_other_lists_stay():
    from provekit_amd import whir_pcs

    def declared_in(path):
        return sorted(set(re.findall(r"\b(pkw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))))

    def exported_by(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(set(re.findall(r" [A-Za-z] (pkw_[a-z0-9_]+)$", nm, flags=re.M)))

    assert declared_in(HIDING_HEADER) == sorted(HIDING) and len(HIDING) == 7
    assert set(HIDING) <= set(exported_by(whir_pcs.WHIR_LIB_PATH)) and set(HIDING) <= set(whir_pcs.SIGNATURES)
    others = [declared_in(os.path.join(ROOT, "include", h)) for h in ("provekit_whir.h", "provekit_whir_linear.h", "provekit_whir_sparse.h")]
    assert [len(o) for o in others] == [15, 4, 5] and all(set(o) <= set(whir_pcs.SIGNATURES) and not set(o) & set(HIDING) for o in others)
    assert exported_by(whir_pcs.WHIR_LIB_PATH) == sorted(whir_pcs.SIGNATURES)
    plain = open(os.path.join(ROOT, "include", "provekit_whir.h")).read()
    assert '#include "provekit_whir_hiding.h"' not in plain and "PLAIN WHIR, NOT HIDING" not in plain and "see provekit_whir_hiding.h" in plain  # named, not included
    assert ctypes.CDLL(whir_pcs.WHIR_LIB_PATH).pkw_abi_version() == 1
    assert whir_pcs.CHECKS[-3:] == ("POINTS", "ROOT", "DEFERRED") and whir_pcs.lib.pkw_check_name(len(whir_pcs.CHECKS)) == b"UNKNOWN"  # no verdict added
    mask0, g, proof_streams = H.streams()
    mine = {mask0, mask0 + 1, mask0 + 2, g}
    assert len(mine) == 4 and len(proof_streams) == 6 and not mine & set(proof_streams)


def test_plain_users_of_the_cpp_header_name_no_symbol_of_the_hiding_library_even_unoptimised(tmp_path):
    """provekit_whir.hpp includes the hiding header, but only WhirPcs::hiding, commit_hiding, open_hiding and verify_hiding may name its
    symbols: an -O0 object of a plain, linear or sparse user names none of the hiding entry points"""
    for demo, wants in (("pcs_demo", False), ("pcs_linear_demo", False), ("pcs_sparse_demo", False), ("pcs_hiding_demo", True)):
        obj = tmp_path / f"{demo}.o"
        subprocess.run(["g++", "-O0", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "examples", demo + ".cpp"), "-o", str(obj)],
                       check=True, capture_output=True, text=True)
        und = subprocess.run(["nm", "--undefined-only", str(obj)], capture_output=True, text=True, check=True).stdout
        named = sorted(set(re.findall(r"\b(pkw_\w*hiding\w*)", und)))
        assert bool(named) == wants, (demo, named)


def test_the_hiding_pattern_declares_the_plain_patterns_operations_under_its_own_label():
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    for n1, B, q in H.SHAPES:
        cfg = H.hiding_config(n1, B)
        hid, plain = whir_pcs.io_pattern_hiding(cfg, q).split(b"\0"), whir_pcs.io_pattern(cfg, q).split(b"\0")
        assert hid[0] == H.LABEL == whir_pcs.HIDING_LABEL and plain[0] == b"provekit-hip/whir-pcs/v1"
        assert hid[1:] == plain[1:] and f"A{q * n1}points".encode() in hid and f"A{q * (B + 1)}evaluations".encode() in hid
    cfg = H.hiding_config(8, 1)
    for q in (0, 65):
        with pytest.raises(ProveKitHipError, match="1..64"):
            whir_pcs.io_pattern_hiding(cfg, q)


@pytest.mark.parametrize("shape", H.SHAPES)
def test_oracle_built_hiding_openings_are_accepted_with_the_evaluations_of_f(oracle, shape):
    from provekit_amd import whir_pcs

    c = H.case(oracle, shape)
    assert c.vals[: c.B] == c.expected  # f^_b(0, z) = f_b(z): the extended tables' first B rows are f's evaluations
    for kw in ({}, {"io_pattern": c.pattern}, {"expected_root": None}):
        r, evals = c.verify(**kw)
        assert r.accepted and r.check == "NONE" and r.offset == len(c.proof), r
        assert evals.shape == (c.B, c.q, 4)
        assert oracle.limbs_to_ints(oracle.from_mont(evals.reshape(-1, 4))) == [v for row in c.expected for v in row]
    # a hiding proof is a valid PLAIN proof of the extended statement: same bytes, extended config, points (0, z), the hiding
    # pattern handed in as the caller's pattern
    r, evals = whir_pcs.verify(c.cfg, K.mont_points(oracle, c.ext_pts), c.proof, expected_root=c.root, io_pattern=c.pattern)
    assert r.accepted and r.offset == len(c.proof), r
    assert oracle.limbs_to_ints(oracle.from_mont(evals.reshape(-1, 4))) == [v for row in c.vals for v in row]  # g(0, z_i) included
    # ... and under the plain label the sponge differs from the first challenge on
    r, _ = whir_pcs.verify(c.cfg, K.mont_points(oracle, c.ext_pts), c.proof, expected_root=c.root)
    assert not r.accepted


def test_every_tampering_is_rejected_with_its_check(oracle):
    from provekit_amd import whir_pcs

    c = H.case(oracle, (8, 3, 3))
    assert c.verify()[0].accepted

    def flipped(off):
        t = bytearray(c.proof)
        t[off] ^= 1
        return bytes(t)

    other_points = c.mpts.copy()
    other_points[c.q - 1, c.n - 1] = oracle.to_mont(oracle.ints_to_limbs([12345]))[0]
    wrong_root = bytes([c.root[0] ^ 1]) + c.root[1:]
    expect = {
        "an evaluation of f changed in the proof": (dict(proof=flipped(c.eval_offset)), "WHIR_SUMCHECK"),
        "an evaluation of g changed in the proof": (dict(proof=flipped(c.eval_offset + 32 * (c.q * (c.B + 1) - 1))), "WHIR_SUMCHECK"),
        "a leading zero changed in the proof": (dict(proof=flipped(c.eval_offset - 32 * c.q * c.n1)), "POINTS"),
        "one point changed in the call": (dict(points=other_points), "POINTS"),
        "a wrong expected root": (dict(expected_root=wrong_root), "ROOT"),
        "a pattern for q + 1": (dict(io_pattern=whir_pcs.io_pattern_hiding(c.cfg, c.q + 1)), "IO_PATTERN"),
        "a pattern for q - 1": (dict(io_pattern=whir_pcs.io_pattern_hiding(c.cfg, c.q - 1)), "IO_PATTERN"),
        "a deferred value changed": (dict(proof=flipped(K.deferred_offset(c.proof, c.q))), "WHIR_FINAL"),
        "truncated by 1 byte": (dict(proof=c.proof[:-1]), "TRANSCRIPT_SHORT"),
        "one appended byte": (dict(proof=c.proof + b"\0"), "TRAILING_BYTES"),
        "the other hash version": (dict(hash_version=1), "MERKLE"),
    }
    for name, (kw, check) in expect.items():
        r, _ = c.verify(**kw)
        print(f"{name}: {r}")
        assert not r.accepted and r.check == check and r.message, (name, r)


def test_a_proof_whose_points_start_with_one_is_rejected_at_the_points(oracle):
    """an honest plain opening of the extended batch at (1, z): it reveals evaluations of the MASKS, and is no hiding opening"""
    from provekit_amd import whir_pcs

    c = H.Case(oracle, 8, 1, 1, lead=1)
    r, _ = whir_pcs.verify(c.cfg, K.mont_points(oracle, c.ext_pts), c.proof, expected_root=c.root, io_pattern=c.pattern)
    assert r.accepted, r  # a valid plain proof of ITS statement
    r, _ = c.verify()
    assert not r.accepted and r.check == "POINTS" and "point 0" in r.message and "coordinate 0" in r.message, r


def test_the_two_config_rules_are_enforced_with_a_reason(oracle):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    c = H.case(oracle, (8, 1, 1))
    bad = K.small_config(8, 1)
    bad.num_queries = [6]
    for call in (lambda: whir_pcs.io_pattern_hiding(bad, 1), lambda: whir_pcs.verify_hiding(bad, c.mpts, c.proof)):
        with pytest.raises(ProveKitHipError, match="PK_ERR_BAD_ARG.*batch_size must be 2..4"):
            call()
    # the mask budget on both sides of equality: 2^n = 128 mask coefficients at n + 1 = 8, 16 values per query
    for ood, queries, fits in ((0, 8, True), (1, 7, True), (1, 8, False), (0, 9, False)):
        cfg = H.hiding_config(8, 1)
        cfg.commitment_ood_samples, cfg.num_queries = ood, [queries]
        left, have = H.budget(cfg)
        assert have == 128 and (left <= have) == fits and (left == have) == (ood == 0 and queries == 8)
        if fits:
            assert whir_pcs.io_pattern_hiding(cfg, 1).startswith(H.LABEL)
            r, _ = whir_pcs.verify_hiding(cfg, c.mpts, c.proof)  # taken: a verdict, accepted where this is the config the proof was made under
            assert r.accepted == ((ood, [queries]) == (c.cfg.commitment_ood_samples, list(c.cfg.num_queries))), r
            continue
        for call in (lambda: whir_pcs.io_pattern_hiding(cfg, 1), lambda: whir_pcs.verify_hiding(cfg, c.mpts, c.proof)):
            with pytest.raises(ProveKitHipError, match=f"mask budget: {left} values.*its 128 mask coefficients"):
                call()
        assert whir_pcs.io_pattern(cfg, 1)  # the plain library takes the config: the rule is the hiding mode's


def test_truncated_proofs_and_hostile_counts_under_the_sanitizers(oracle, tmp_path):
    """pkw_verify_hiding alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan):
    points, proof and outputs live in exact-size heap blocks there, so a read or write past any of them is a report"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkw_verify_asan is missing: make -C provekit_amd/csrc asan"
    from provekit_amd import whir_pcs

    c = H.case(oracle, (8, 3, 3))
    d0 = K.deferred_offset(c.proof, c.q)
    proofs = {"honest": c.proof, "zero length": b"", "truncated inside the points": c.proof[: c.eval_offset - 40],
              "truncated inside the evaluations": c.proof[: c.eval_offset + 32 * c.q * c.B + 7], "truncated inside the deferred hint": c.proof[: d0 + 33],
              "truncated by 1 byte": c.proof[:-1], "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes()}
    t = bytearray(c.proof)
    struct.pack_into("<Q", t, d0 - 8, 1 << 63)
    proofs["deferred count = 2^63"] = bytes(t)
    counts = {0: "REFUSED", 65: "REFUSED", 0xFFFFFFFF: "REFUSED", 1 << 31: "REFUSED", c.q + 1: "IO_PATTERN", 1: "IO_PATTERN", 64: "IO_PATTERN"}
    cs = whir_pcs._cfg_struct(c.cfg)
    blob = struct.pack("<4I", 2, c.q, 0, 0) + bytes(cs) + struct.pack("<I", len(c.pattern)) + c.pattern + c.mpts.tobytes()
    blob += struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs.values())
    blob += struct.pack("<I", len(counts)) + b"".join(struct.pack("<I", k) for k in counts)
    f = tmp_path / "cases.bin"
    f.write_bytes(blob)
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    p = subprocess.run([ASAN, "hiding", str(f)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(proofs) + len(counts)
    for (name, proof), line in zip(proofs.items(), lines):
        rc, accepted, check, offset = line.split()[:4]
        if name == "honest":
            assert (rc, accepted, check, int(offset)) == ("0", "1", "NONE", len(proof)), line
        else:
            assert rc == "0" and accepted == "0" and check in STRUCTURAL, (name, line)
        r, _ = c.verify(proof=proof, expected_root=None)  # the library loaded into this process gives the same verdict
        assert (str(int(r.accepted)), r.check, r.offset) == (accepted, check, int(offset)), (name, line, r)
    for (count, want), line in zip(counts.items(), lines[len(proofs) :]):
        if want == "REFUSED":
            assert line.startswith("-1 0 REFUSED") and "1..64" in line, (count, line)
        else:
            assert line.split()[:3] == ["0", "0", want], (count, line)
