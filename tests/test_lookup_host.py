"""CPU: libprovekit_lookup.so's host side.  The header/library/binding symbol match and what the library links; pkl_io_pattern against
the reference's pattern; every refusal with its reason; pkl_verify on proofs the Python reference prover builds (tests/lookup_refs.py):
acceptance with the reference's alpha, points and seven claims, and every tampering with the check and the side both verifiers must
name; hostile framing through the sanitizer build of the host verifier (a program of its own, run as a subprocess)."""
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
HEADER = os.path.join(ROOT, "include", "provekit_lookup.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkl_verify_asan")

import lookup_refs as L  # noqa: E402
import prodcheck_refs as K  # noqa: E402

P = K.P


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import lookup

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkl_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", lookup.LOOKUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkl_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(lookup.SIGNATURES) and len(exported) == 14
    assert ctypes.CDLL(lookup.LOOKUP_LIB_PATH).pkl_abi_version() == 1
    assert ctypes.sizeof(lookup.ClaimsStruct) == 32 * (2 + 2 * 28 + 7) and ctypes.sizeof(lookup.StatementStruct) == 16
    # the library calls the product and the sumcheck library only through their C ABIs, and no other library above the product
    und = subprocess.run(["nm", "-D", "--undefined-only", lookup.LOOKUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pks\w+", und) and not re.findall(r"\bpk[vw]_\w+", und), und
    inc = os.path.join(ROOT, "include")
    assert set(re.findall(r"\bpk_\w+", und)) <= set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", open(os.path.join(inc, "provekit_hip.h")).read()))
    called = set(re.findall(r"\bpks_\w+", und))
    assert {"pks_prove", "pks_verify", "pks_prover_create"} <= called <= set(re.findall(r"\b(pks_[a-z0-9_]+)\s*\(", open(os.path.join(inc, "provekit_sumcheck.h")).read()))
    needed = subprocess.run(["readelf", "-d", lookup.LOOKUP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    libs = set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed))
    assert libs == {"libprovekit_sumcheck.so", "libprovekit_hip.so"}, libs


def test_io_pattern_is_the_references_and_differs_between_sizes():
    from provekit_amd import lookup

    pats = {}
    for n, k in ((1, 1), (2, 1), (1, 3), (8, 8), (12, 8), (28, 28)):
        for n_bind, n_bind2 in ((0, 0), (3, 0), (0, 2), (16, 16)):
            stmt = lookup.Statement(n, k, n_bind, n_bind2)
            pat = lookup.io_pattern(stmt)
            assert pat == L.pattern(n, k, n_bind, n_bind2), (n, k, n_bind, n_bind2)
            assert lookup.proof_bytes(stmt) == L.proof_bytes(n, k) == 32 * (1 + 3 * n + 2 + 3 * k + 3 + 2)
            pats[(n, k, n_bind, n_bind2)] = pat
    assert len(set(pats.values())) == len(pats)
    head = pats[(12, 8, 3, 0)].split(b"\0")
    assert head == [lookup.LABEL + b"/n12/k8", b"A3bind", b"S1alpha", b"A1sum", b"S12tau_f", b"S8tau_t", b"S1seed"]
    assert pats[(12, 8, 0, 2)].split(b"\0")[1:4] == [b"S1alpha", b"A2helpers", b"A1sum"]
    # (n, k) and (k, n): told apart by the label and by which squeeze has which count
    assert lookup.io_pattern(lookup.Statement(3, 5)) != lookup.io_pattern(lookup.Statement(5, 3))


def test_arena_bytes_states_the_arena_and_both_sumcheck_arenas():
    from provekit_amd import lookup

    for n, k in ((1, 1), (12, 8), (10, 13), (28, 20)):
        total = lookup.arena_bytes(lookup.Statement(n, k))
        own = 32 * (2 * 2**n + 3 * 2**k) + 4 * 2**k
        sumchecks = 32 * (2 * 2 ** (n - 1) + 3 * 2 ** (k - 1))
        assert own + sumchecks <= total <= own + sumchecks + 2**22  # partial sums, the sumchecks' scratch and split eq tables
    assert 1 <= lookup.count_lds_max_k() <= 15  # 2^k u32 bins in 160 KiB of LDS
    assert 1 <= lookup.gather_lds_max_k() <= 11  # 2 * 2^k * 32 bytes in 160 KiB of LDS


@pytest.mark.parametrize("stmt, reason", [
    ((0, 4), "n must be"), ((29, 4), "n must be"), ((4, 0), "k must be"), ((4, 29), "k must be"),
    ((4, 4, 17, 0), "n_bind must be"), ((4, 4, 0, 17), "n_bind2 must be"),
])
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import lookup
    from provekit_amd._lib import ProveKitHipError

    s = lookup.Statement(*stmt)
    for call in (lookup.io_pattern, lookup.proof_bytes, lookup.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r = s.struct(), lookup.ResultStruct()  # the verifier refuses the statement before it looks at anything else
    assert lookup.lib.pkl_verify(ctypes.addressof(st), None, 0, None, None, None, 0, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, lookup.lib.pkl_create_error().decode())


def test_verify_refuses_bind_elements_that_do_not_match_the_statement():
    from provekit_amd import lookup
    from provekit_amd._lib import ProveKitHipError

    s = lookup.Statement(3, 2, 1, 1)
    st, r = s.struct(), lookup.ResultStruct()
    one = K.mont([1])
    for bind, bind2, reason in ((None, one.ctypes.data, b"binds elements: pass"), (one.ctypes.data, None, b"after the helper tables")):
        assert lookup.lib.pkl_verify(ctypes.addressof(st), None, 0, bind, bind2, None, 0, None, None, ctypes.byref(r)) == -1
        assert reason in lookup.lib.pkl_create_error()
    too_big = np.array([[2**64 - 1] * 4], dtype=np.uint64)
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p"):
        lookup.verify(s, b"", bind=too_big, bind2=one)
    with pytest.raises(ProveKitHipError, match="bind2 element 0 is not below p"):
        lookup.verify(s, b"", bind=one, bind2=too_big)


SIZES = [(1, 1), (2, 1), (1, 3), (5, 3), (4, 6)]


class Case:
    def __init__(self, n, k):
        self.n, self.k = n, k
        self.f, self.t, self.idx = L.random_case(n, k, seed=10 * n + k)
        self.bind, self.bind2 = K.random_elements(3, seed=5), K.random_elements(2, seed=6)
        self.ref = L.prove(n, k, self.f, self.t, self.idx, self.bind, self.bind2)
        self.proof = self.ref["proof"]

    def both(self, proof=None, bind=None, bind2=None, pattern=None):
        """the library's verdict, after asserting that the reference names the same check and side"""
        from provekit_amd import lookup

        proof = self.proof if proof is None else proof
        bind = self.bind if bind is None else bind
        bind2 = self.bind2 if bind2 is None else bind2
        check, side, ref = L.verify(self.n, self.k, proof, bind, bind2, pattern)
        res, lib_side, claims = lookup.verify(lookup.Statement(self.n, self.k, 3, 2), proof, K.mont(bind), K.mont(bind2), pattern)
        assert (res.check, lib_side) == (check, side) and res.accepted == (check == "NONE"), (res, lib_side, check, side)
        return res, lib_side, claims, ref


@pytest.fixture(scope="module")
def cases():
    return {size: Case(*size) for size in SIZES}


@pytest.mark.parametrize("size", SIZES)
def test_reference_proofs_are_accepted_with_the_references_alpha_points_and_claims(cases, size):
    c = cases[size]
    n, k, ref = c.n, c.k, c.ref
    assert len(c.proof) == L.proof_bytes(n, k) and int.from_bytes(c.proof[:32], "little") == ref["s"]
    # the reference proves what it says: the LogUp sums agree and the claims are the tables' extensions
    assert ref["s"] == sum(ref["h_f"]) % P == sum(pow(ref["alpha"] - v, -1, P) for v in c.f) % P
    tables = {"hf_at_rf": (ref["h_f"], ref["r_f"]), "f_at_rf": (c.f, ref["r_f"]), "ht_at_rt": (ref["h_t"], ref["r_t"]), "t_at_rt": (c.t, ref["r_t"]),
              "m_at_rt": (ref["m"], ref["r_t"]), "hf_at_half": (ref["h_f"], [L.INV2] * n), "ht_at_half": (ref["h_t"], [L.INV2] * k)}
    for name, (table, point) in tables.items():
        assert ref["claims"][name] == L.mle_at(table, point), name
    for kw in ({}, {"pattern": L.pattern(n, k, 3, 2)}):
        res, side, claims, seen = c.both(**kw)
        assert res.accepted and res.check == "NONE" and side == "OUTER" and res.offset == len(c.proof) and res.message == ""
        assert K.unmont(claims.alpha) == [ref["alpha"]] == [seen["alpha"]] and K.unmont(claims.s) == [ref["s"]]
        assert K.unmont(claims.r_f) == ref["r_f"] == seen["r_f"] and K.unmont(claims.r_t) == ref["r_t"] == seen["r_t"]
        for name in L.CLAIMS:
            assert K.unmont(getattr(claims, name)) == [ref["claims"][name]] == [seen["claims"][name]], name


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


@pytest.mark.parametrize("size", SIZES)
def test_every_tampering_is_rejected_at_the_named_check_and_side(cases, size):
    c = cases[size]
    n, k = c.n, c.k
    f_at, t_at = 1, 1 + 1 + 3 * n + 2  # in elements: the F proof, the T proof
    # s enters the challenges of both sumchecks, and the F side is read first.  h_f d_f is 1 at every x, so the F side's round 0 adds up
    # to 1 under ANY tau_f: other challenges show in a later round, or in the final check where the folded columns stay inverse to each
    # other (at tiny n: when idx does not depend on the leading index bits), or not before the T side when idx is constant and the F
    # side's columns are.  The reference names which (both()); here: rejected, by a sumcheck, and not by the F side's round 0
    def other_challenges(res, side):
        assert side in ("F", "T") and res.check in ("ROUND", "FINAL") and (side == "T" or "round 0:" not in res.message), (res, side)

    other_challenges(*c.both(_bump(c.proof, 0))[:2])
    # the sums the two sumchecks state are fixed by the protocol: 1 and 0
    assert c.both(_bump(c.proof, f_at))[:2][0].check == "SUM" and c.both(_bump(c.proof, f_at))[1] == "F"
    res, side, _, _ = c.both(_bump(c.proof, t_at))
    assert (res.check, side) == ("SUM", "T") and res.offset == 32 * (t_at + 1)
    # a round value of each side
    for i in range(n):
        res, side, _, _ = c.both(_bump(c.proof, f_at + 1 + 3 * i))
        assert (res.check, side) == ("ROUND", "F") and f"round {i}:" in res.message and res.offset == 32 * (f_at + 1 + 3 * (i + 1))
    for i in range(k):
        res, side, _, _ = c.both(_bump(c.proof, t_at + 1 + 3 * i))
        assert (res.check, side) == ("ROUND", "T") and f"round {i}:" in res.message and res.offset == 32 * (t_at + 1 + 3 * (i + 1))
    # a final of each side
    for j in range(2):
        res, side, _, _ = c.both(_bump(c.proof, f_at + 1 + 3 * n + j))
        assert (res.check, side) == ("FINAL", "F")
    for j in range(3):
        res, side, _, _ = c.both(_bump(c.proof, t_at + 1 + 3 * k + j))
        assert (res.check, side) == ("FINAL", "T") and res.offset == len(c.proof)
    # bind and bind2 enter nothing but the challenges
    for which in ("bind", "bind2"):
        for e in range(len(getattr(c, which))):
            changed = list(getattr(c, which))
            changed[e] = (changed[e] + 1) % P
            other_challenges(*c.both(**{which: changed})[:2])
    # framing: the three parts have fixed lengths
    for cut in (0, 31, 32, 32 * t_at, len(c.proof) - 1):
        res, side, _, _ = c.both(c.proof[:cut])
        assert (res.check, side, res.offset) == ("TRANSCRIPT_SHORT", "OUTER", cut)
    for extra in (b"\0", bytes(32)):
        res, side, _, _ = c.both(c.proof + extra)
        assert (res.check, side, res.offset) == ("TRAILING_BYTES", "OUTER", len(c.proof))
    # v + p: the same value mod p, not canonical on the wire
    for element, want_side in ((0, "OUTER"), (f_at + 1, "F"), (t_at + 1 + 3 * k, "T")):
        t = bytearray(c.proof)
        v = int.from_bytes(t[32 * element : 32 * element + 32], "little") + P
        if v < 1 << 256:
            t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
            res, side, _, _ = c.both(bytes(t))
            assert (res.check, side, res.offset) == ("NON_CANONICAL", want_side, 32 * (element + 1))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are other challenges
    assert c.both(pattern=L.pattern(n, k, 2, 2))[:2][0].check == "IO_PATTERN"
    res, side, _, _ = c.both(pattern=L.pattern(n + 1, k, 3, 2))
    assert (res.check, side) == ("IO_PATTERN", "OUTER")
    other_challenges(*c.both(pattern=L.pattern(n, k, 3, 2).replace(b"/v1/", b"/v2/"))[:2])


def test_hostile_framing_and_counts_under_the_sanitizers(cases, tmp_path):
    """the host verifier alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan): proofs cut
    at every kind of place and grown, from exact-size heap blocks; statements whose counts would size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkl_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    c = cases[(5, 3)]
    n, k = c.n, c.k
    t_at = 32 * (1 + 1 + 3 * n + 2)
    hostile = {"honest": c.proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(c.proof), "extended": c.proof + bytes(64),
               "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes(),
               "random sides": c.proof[:32] + np.random.default_rng(2).integers(0, 256, size=len(c.proof) - 32, dtype=np.uint8).tobytes(),
               "random T side": c.proof[:t_at] + np.random.default_rng(3).integers(0, 256, size=len(c.proof) - t_at, dtype=np.uint8).tobytes(),
               "sides swapped": c.proof[:32] + c.proof[t_at:] + c.proof[32:t_at]}
    for cut in (1, 31, 33, t_at - 1, t_at, t_at + 1, len(c.proof) - 1):
        hostile[f"cut at {cut}"] = c.proof[:cut]
    for pat in (b"", L.pattern(n, k, 3, 2)):
        blob = struct.pack("<4I", n, k, 3, 2) + struct.pack("<I", len(pat)) + pat + K.mont(c.bind).tobytes() + K.mont(c.bind2).tobytes()
        blob += struct.pack("<I", len(hostile)) + b"".join(struct.pack("<Q", len(p)) + p for p in hostile.values())
        f = tmp_path / "cases.bin"
        f.write_bytes(blob)
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = p.stdout.splitlines()
        assert len(lines) == len(hostile)
        for (name, proof), line in zip(hostile.items(), lines):
            rc, accepted, check, side, offset = line.split()[:5]
            want, want_side, _ = L.verify(n, k, proof, c.bind, c.bind2)
            assert (rc, check, accepted, side) == ("0", want, "1" if want == "NONE" else "0", str(("OUTER", "F", "T").index(want_side))), (name, line)
            assert int(offset) <= max(len(proof), len(c.proof))
    for bad in ([2**31, 3, 0, 0], [5, 2**32 - 1, 0, 0], [5, 3, 2**32 - 1, 0], [5, 3, 0, 2**30], [0, 0, 0, 0]):
        f = tmp_path / "refused.bin"
        f.write_bytes(struct.pack("<4I", *bad))  # nothing after the statement: a count that was believed would read past the block
        p = subprocess.run([ASAN, "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0 and p.stdout.startswith("-1 0 REFUSED"), (bad, p.stdout, p.stderr[-2000:])
