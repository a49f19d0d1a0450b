"""CPU: libprovekit_fracsum.so's host side.  The header/library/binding symbol match and what the library links; the two outer IO
patterns and the proof lengths against the reference's; every refusal with its reason; pkf_verify and pkf_lookup_verify on proofs the
Python reference provers build (tests/fracsum_refs.py): acceptance with the reference's fraction, point and values, and every tampering
with the check, the layer and the offset both verifiers must name; hostile framing through the sanitizer build of the host verifiers (a
program of its own, run as a subprocess)."""
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
HEADER = os.path.join(ROOT, "include", "provekit_fracsum.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkf_verify_asan")

import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402

P = K.P


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import fracsum as fs

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkf_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", fs.FRACSUM_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkf_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(fs.SIGNATURES) and len(exported) == 21
    assert ctypes.CDLL(fs.FRACSUM_LIB_PATH).pkf_abi_version() == 1
    assert ctypes.sizeof(fs.LookupClaimsStruct) == 32 * (4 + 2 * 28) and ctypes.sizeof(fs.StatementStruct) == 12 and ctypes.sizeof(fs.LookupStatementStruct) == 12
    # pks's check numbers unchanged, three new ones after them
    assert [fs.lib.pkf_check_name(i).decode() for i in range(len(fs.CHECKS))] == list(fs.CHECKS) and len(fs.CHECKS) == 24
    assert fs.CHECKS[-3:] == ("FRACTION", "DENOMINATOR", "UNIT") and fs.CHECKS[:-3] == tuple(__import__("provekit_amd.prodcheck", fromlist=["x"]).CHECKS)
    text = open(HEADER).read()
    assert re.search(r"#define PKF_CHECK_FRACTION PKS_CHECK_COUNT\b", text) and re.search(r"#define PKF_CHECK_COUNT \(PKS_CHECK_COUNT \+ 3\)", text)
    assert "PKG_CHECK_PRODUCT" in text  # the header says which other library's number the first one coincides with
    # the library calls the product and the sumcheck library only through their C ABIs, and no other library above the product
    und = subprocess.run(["nm", "-D", "--undefined-only", fs.FRACSUM_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pks\w+", und) and not re.findall(r"\bpk[vwlg]_\w+", und), und
    inc = os.path.join(ROOT, "include")
    assert set(re.findall(r"\bpk_\w+", und)) <= set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", open(os.path.join(inc, "provekit_hip.h")).read()))
    called = set(re.findall(r"\bpks_\w+", und))
    assert {"pks_prove", "pks_verify", "pks_prover_create"} <= called <= set(re.findall(r"\b(pks_[a-z0-9_]+)\s*\(", open(os.path.join(inc, "provekit_sumcheck.h")).read()))
    needed = subprocess.run(["readelf", "-d", fs.FRACSUM_LIB_PATH], capture_output=True, text=True, check=True).stdout
    libs = set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed))
    assert libs == {"libprovekit_sumcheck.so", "libprovekit_hip.so"}, libs


def test_io_patterns_and_proof_lengths_are_the_references_and_differ_between_statements():
    from provekit_amd import fracsum as fs, prodcheck

    pats = {}
    for n in (1, 2, 3, 8, 28):
        for n_bind in (0, 3, 16):
            for unit in (0, 1):
                stmt = fs.Statement(n, n_bind, unit)
                pats[(n, n_bind, unit)] = fs.io_pattern(stmt)
                assert pats[(n, n_bind, unit)] == F.pattern(n, unit, n_bind), (n, n_bind, unit)
                assert fs.proof_bytes(stmt) == F.proof_bytes(n, unit) == 128 + (n - 1) * (48 * n + 160) - 32 * (unit and n >= 2)
                # the length is the sum of the layers' pks_proof_bytes
                assert fs.proof_bytes(stmt) == 128 + sum(prodcheck.proof_bytes(F.layer(n, unit, d).statement()) for d in range(1, n))
            for k in (1, 5):
                ls = fs.LookupStatement(n, k, n_bind)
                pats[("lookup", n, k, n_bind)] = fs.io_pattern(ls)
                assert pats[("lookup", n, k, n_bind)] == F.lookup_pattern(n, k, n_bind)
                assert fs.proof_bytes(ls) == F.lookup_proof_bytes(n, k) == fs.proof_bytes(fs.Statement(n, 1, 1)) + fs.proof_bytes(fs.Statement(k, 1, 0))
    assert len(set(pats.values())) == len(pats)
    assert pats[(1, 0, 0)].split(b"\0") == [fs.LABEL + b"/n1/u0", b"A4top", b"S1rho"]
    assert pats[(3, 3, 0)].split(b"\0") == [fs.LABEL + b"/n3/u0", b"A3bind", b"A4top", b"S1rho"] + [b"S1lambda", b"S1seed", b"A4finals", b"S1rho"] * 2
    # unit: the leaves' layer has three finals
    assert pats[(3, 0, 1)].split(b"\0") == [fs.LABEL + b"/n3/u1", b"A4top", b"S1rho", b"S1lambda", b"S1seed", b"A4finals", b"S1rho", b"S1lambda", b"S1seed",
                                            b"A3finals", b"S1rho"]
    assert pats[("lookup", 8, 5, 3)].split(b"\0") == [fs.LOOKUP_LABEL + b"/n8/k5", b"A3bind", b"S1alpha", b"S2seeds"]
    assert pats[("lookup", 8, 5, 0)].split(b"\0") == [fs.LOOKUP_LABEL + b"/n8/k5", b"S1alpha", b"S2seeds"]


def test_arena_bytes_states_the_trees_the_combined_table_and_the_sumcheck_arenas():
    from provekit_amd import fracsum as fs

    for unit in (0, 1):
        for n in (1, 2, 12, 28):
            total = fs.arena_bytes(fs.Statement(n, 0, unit))
            own = 32 * (2 * 2**n + (2 ** (n - 1) if n > 1 else 0))
            sumchecks = 32 * sum((3 if unit and d == n - 1 else 4) * 2 ** (d - 1) for d in range(1, n))  # the layers' folded copies
            assert own + sumchecks <= total <= own + sumchecks + (n - 1) * 2**21
    n, k = 12, 7
    assert fs.arena_bytes(fs.LookupStatement(n, k)) == fs.arena_bytes(fs.Statement(n, 1, 1)) + fs.arena_bytes(fs.Statement(k, 1, 0)) + 32 * (2**n + 2**k)
    assert 1 <= fs.tail_max_n() <= 11  # two arrays of 2^(t-1) elements of 32 bytes in the 64 KiB of LDS a kernel gets without asking


@pytest.mark.parametrize("kind, stmt, reason", [
    ("fs", (0,), "n must be"), ("fs", (29,), "n must be"), ("fs", (4, 17), "n_bind must be"), ("fs", (4, 0, 2), "unit must be"),
    ("lk", (0, 1), "n must be"), ("lk", (29, 1), "n must be"), ("lk", (4, 0), "k must be"), ("lk", (4, 29), "k must be"), ("lk", (4, 2, 17), "n_bind must be"),
])
def test_every_refusal_is_made_with_a_reason(kind, stmt, reason):
    from provekit_amd import fracsum as fs
    from provekit_amd._lib import ProveKitHipError

    s = fs.Statement(*stmt) if kind == "fs" else fs.LookupStatement(*stmt)
    for call in (fs.io_pattern, fs.proof_bytes, fs.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r = s.struct(), fs.ResultStruct()  # the verifiers refuse the statement before they look at anything else
    if kind == "fs":
        rc = fs.lib.pkf_verify(ctypes.addressof(st), None, 0, None, None, None, 0, None, None, None, None, None, ctypes.byref(r))
    else:
        rc = fs.lib.pkf_lookup_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r))
    assert rc == -1 and re.search(reason, fs.lib.pkf_create_error().decode())


def test_verify_refuses_elements_that_do_not_match_the_statement():
    from provekit_amd import fracsum as fs
    from provekit_amd._lib import ProveKitHipError

    too_big = np.array([[2**64 - 1] * 4], dtype=np.uint64)
    for s, call in ((fs.Statement(3, 1), lambda st, r: fs.lib.pkf_verify(ctypes.addressof(st), None, 0, None, None, None, 0, None, None, None, None, None, ctypes.byref(r))),
                    (fs.LookupStatement(3, 2, 1), lambda st, r: fs.lib.pkf_lookup_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)))):
        st, r = s.struct(), fs.ResultStruct()
        assert call(st, r) == -1 and b"binds elements: pass" in fs.lib.pkf_create_error()  # NULL where elements are due
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p") as e:
        fs.verify(fs.Statement(3, 1), b"", bind=too_big)
    assert e.value.code == -1
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p"):
        fs.lookup_verify(fs.LookupStatement(3, 2, 1), b"", bind=too_big)
    with pytest.raises(ProveKitHipError, match="expected_fraction element 1 is not below p"):
        fs.verify(fs.Statement(3, 0), b"", expected_fraction=np.concatenate([K.mont([1]), too_big]))


SIZES = [1, 2, 3, 5]
TABLES = ("random", "zeros", "unit")  # random p and q; p with zeros; no p


class Case:
    def __init__(self, n, table):
        self.n, self.unit = n, int(table == "unit")
        self.q = F.random_table(n, seed=n)
        self.p = {"random": lambda: K.random_elements(1 << n, seed=n + 30), "zeros": lambda: F.random_table(n, seed=n + 50, zeros=(0, (1 << n) - 1)),
                  "unit": lambda: None}[table]()
        self.bind = K.random_elements(3, seed=5)
        self.ref = F.prove(n, self.p, self.q, self.bind)
        self.proof = self.ref["proof"]

    def layer_at(self, d):
        return F.layer_at(self.n, self.unit, d)

    def both(self, proof=None, bind=None, pattern=None, expected=None):
        """the library's verdict, after asserting that the reference names the same check, layer and (where it states one) offset"""
        from provekit_amd import fracsum as fs

        proof = self.proof if proof is None else proof
        bind = self.bind if bind is None else bind
        check, layer, offset, ref = F.verify(self.n, self.unit, proof, bind, pattern, expected)
        res, lib_layer, out = fs.verify(fs.Statement(self.n, 3, self.unit), proof, K.mont(bind), None if expected is None else K.mont(expected), pattern)
        assert (res.check, lib_layer) == (check, layer) and res.accepted == (check == "NONE"), (res, lib_layer, check, layer)
        assert offset is None or res.offset == offset, (res, offset)
        return res, lib_layer, out, ref


CASES = [(n, t) for n in SIZES for t in TABLES]


@pytest.fixture(scope="module")
def cases():
    return {(n, t): Case(n, t) for n, t in CASES}


@pytest.mark.parametrize("n, table", CASES)
def test_reference_proofs_are_accepted_with_the_references_fraction_point_and_values(cases, n, table):
    c = cases[(n, table)]
    ref = c.ref
    top = ref["p_layers"][1] + ref["q_layers"][1]
    assert len(c.proof) == F.proof_bytes(n, c.unit) and [int.from_bytes(c.proof[32 * i : 32 * i + 32], "little") for i in range(4)] == top
    # the reference proves what it says: P / Q is the sum of the fractions and the claims are the tables' extensions at the point
    assert ref["Q"] != 0 and ref["P"] * pow(ref["Q"], -1, P) % P == F.fraction_sum(c.p, c.q)
    assert ref["value_q"] == F.mle_at(c.q, ref["point"]) and (ref["value_p"] is None) == bool(c.unit)
    if not c.unit:
        assert ref["value_p"] == F.mle_at(c.p, ref["point"])
    twice = (2 * ref["P"] % P, 2 * ref["Q"] % P)  # the same fraction in other terms
    for kw in ({}, {"pattern": F.pattern(n, c.unit, 3)}, {"expected": (ref["P"], ref["Q"])}, {"expected": twice}):
        res, layer, out, seen = c.both(**kw)
        assert res.accepted and res.check == "NONE" and layer == 0 and res.offset == len(c.proof) and res.message == ""
        assert K.unmont(out[0]) == [ref["P"], ref["Q"]] == [seen["P"], seen["Q"]] and K.unmont(out[1]) == ref["point"] == seen["point"]
        assert K.unmont(out[3]) == [ref["value_q"]] == [seen["value_q"]]
        assert (out[2] is None and seen["value_p"] is None) if c.unit else K.unmont(out[2]) == [ref["value_p"]] == [seen["value_p"]]


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


def _set(proof, element, value):
    t = bytearray(proof)
    t[32 * element : 32 * element + 32] = (value % P).to_bytes(32, "little")
    return bytes(t)


@pytest.mark.parametrize("n, table", [(n, t) for n in SIZES for t in ("random", "unit")])
def test_every_tampering_is_rejected_at_the_named_check_layer_and_offset(cases, n, table):
    c = cases[(n, table)]
    unit, ref = c.unit, c.ref
    at = [None] + [c.layer_at(d) // 32 for d in range(1, n + 1)]  # in elements: at[d] is layer d's s
    good = (ref["P"], ref["Q"])
    # each top value: other claims, so layer 1's stated sum is not theirs; at n = 1 there is no layer: another fraction is accepted
    # unless one is expected -- or the statement is unit, whose top numerators are the leaves and must be 1
    for e in range(4):
        res, layer, _, _ = c.both(_bump(c.proof, e))
        want = ("SUM", 1) if n > 1 else ("UNIT", 0) if unit and e < 2 else ("NONE", 0)
        assert (res.check, layer) == want, (e, res)
        if want != ("UNIT", 0):
            res, layer, _, _ = c.both(_bump(c.proof, e), expected=good)
            assert (res.check, layer, res.offset) == ("FRACTION", 0, 128)
    for d in range(1, n):
        m = F.layer(n, unit, d).m
        # s is checked against the running claims; a round value against the claim of its round; a final against the last claim
        res, layer, _, _ = c.both(_bump(c.proof, at[d]))
        assert (res.check, layer, res.offset) == ("SUM", d, 32 * (at[d] + 1))
        for i in range(d):
            for j in (1, 2):  # h(1), h(2): this round's check or, through the next claim, a later one of the same layer
                res, layer, _, _ = c.both(_bump(c.proof, at[d] + 1 + 3 * i + j))
                assert layer == d and res.check in ("ROUND", "FINAL"), res
            res, layer, _, _ = c.both(_bump(c.proof, at[d] + 1 + 3 * i))
            assert (res.check, layer) == ("ROUND", d) and f"round {i}:" in res.message and res.offset == 32 * (at[d] + 1 + 3 * (i + 1))
        for j in range(m):
            res, layer, _, _ = c.both(_bump(c.proof, at[d] + 1 + 3 * d + j))
            assert (res.check, layer, res.offset) == ("FINAL", d, 32 * at[d + 1]), (d, j, res)
    if unit and n > 1:
        # the unit layer's finals (b, c, e): qR + qL u is linear in b, so another e with the b that keeps the sumcheck's final check
        # passes pks_verify -- and is not 1 + lambda c
        d = n - 1
        b_at, e_at = at[d] + 1 + 3 * d, at[d] + 1 + 3 * d + 2
        b, cc, e = (int.from_bytes(c.proof[32 * i : 32 * i + 32], "little") for i in range(b_at, b_at + 3))
        e2 = (e + 1) % P
        b2 = b * e % P * pow(e2, -1, P) % P
        res, layer, _, _ = c.both(_set(_set(c.proof, e_at, e2), b_at, b2))
        assert (res.check, layer, res.offset) == ("UNIT", d, 32 * at[n]), res
    # a bind element enters nothing but the challenges: rho_1 and so the claims change
    for e in range(3):
        changed = list(c.bind)
        changed[e] = (changed[e] + 1) % P
        res, layer, _, _ = c.both(bind=changed)
        assert (res.check, layer) == (("SUM", 1) if n > 1 else ("NONE", 0))
    # framing: every part has a fixed length
    for cut in sorted({0, 31, 64, 128, c.layer_at(max(n - 1, 1)), len(c.proof) - 1} - {len(c.proof)}):
        res, layer, _, _ = c.both(c.proof[:cut])
        assert (res.check, layer, res.offset) == ("TRANSCRIPT_SHORT", 0, cut)
    for extra in (b"\0", bytes(32)):
        res, layer, _, _ = c.both(c.proof + extra)
        assert (res.check, layer, res.offset) == ("TRAILING_BYTES", 0, len(c.proof))
    # v + p: the same value mod p, not canonical on the wire
    for element, want_layer in [(i, 0) for i in range(4)] + [(at[d] + 1, d) for d in range(1, n)] + [(at[d + 1] - 1, d) for d in range(1, n)]:
        t = bytearray(c.proof)
        v = int.from_bytes(t[32 * element : 32 * element + 32], "little") + P
        if v < 1 << 256:
            t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
            res, layer, _, _ = c.both(bytes(t))
            assert (res.check, layer, res.offset) == ("NON_CANONICAL", want_layer, 32 * (element + 1))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are other challenges
    res, layer, _, _ = c.both(pattern=F.pattern(n, unit, 2))
    assert (res.check, layer) == ("IO_PATTERN", 0)
    res, layer, _, _ = c.both(pattern=F.pattern(n + 1, 0, 3))
    assert (res.check, layer) == (("SUM", 1) if n > 1 else ("IO_PATTERN", 0))
    res, layer, _, _ = c.both(pattern=F.pattern(n, unit, 3).replace(b"/v1/", b"/v2/"))
    assert (res.check, layer) == (("SUM", 1) if n > 1 else ("NONE", 0))
    if n > 1:  # the other kind of statement: same length of top, other label
        res, layer, _, _ = c.both(pattern=F.pattern(n, 1 - unit, 3))
        assert (res.check, layer) in (("SUM", 1), ("IO_PATTERN", 0))
    # a wrong expected fraction: judged at the top, before any layer
    res, layer, _, _ = c.both(expected=((ref["P"] + 1) % P, ref["Q"]))
    assert (res.check, layer, res.offset) == ("FRACTION", 0, 128)
    # a zero denominator at the top: Q = 0, whatever is expected
    for e in (2, 3):
        res, layer, _, _ = c.both(_set(c.proof, e, 0), expected=good)
        assert (res.check, layer, res.offset) == ("DENOMINATOR", 0, 128)


def test_a_table_with_a_zero_denominator_is_rejected_whoever_proves_it():
    """what a prover that does not stop at Q = 0 can send: every layer holds, and the top says DENOMINATOR"""
    from provekit_amd import fracsum as fs

    n = 3
    q = F.random_table(n, seed=8, zeros=(5,))
    ref = F.prove(n, None, q, (), validate=False)
    assert ref["Q"] == 0
    res, layer, out = fs.verify(fs.Statement(n, 0, 1), ref["proof"])
    assert (res.check, layer, res.offset, out) == ("DENOMINATOR", 0, 128, None) and F.verify(n, 1, ref["proof"])[0] == "DENOMINATOR"


LOOKUPS = [(1, 1), (3, 2), (2, 4), (4, 3)]


class LookupCase:
    def __init__(self, n, k):
        rng = np.random.default_rng(10 * n + k)
        self.n, self.k = n, k
        self.t = K.random_elements(1 << k, seed=100 * n + k)
        self.f = [self.t[i] for i in rng.integers(0, 1 << k, size=1 << n)]
        self.m = F.multiplicities(self.f, self.t)
        self.bind = K.random_elements(3, seed=9)
        self.ref = F.lookup_prove(n, k, self.f, self.t, self.m, self.bind)
        outside = list(self.f)
        outside[(1 << n) - 1] = (max(self.t) + 1) % P if (max(self.t) + 1) % P not in self.t else 12345  # one entry outside t
        self.outside = F.lookup_prove(n, k, outside, self.t, self.m, self.bind, validate=False)
        wrong_m = list(self.m)
        wrong_m[0] = (wrong_m[0] + 1) % P
        self.wrong_m = F.lookup_prove(n, k, self.f, self.t, wrong_m, self.bind, validate=False)

    def both(self, proof, bind=None, pattern=None):
        from provekit_amd import fracsum as fs

        bind = self.bind if bind is None else bind
        want = F.lookup_verify(self.n, self.k, proof, bind, pattern)
        res, side, layer, claims = fs.lookup_verify(fs.LookupStatement(self.n, self.k, 3), proof, K.mont(bind), pattern)
        assert (res.check, side, layer) == want[:3] and res.accepted == (want[0] == "NONE"), (res, side, layer, want[:3])
        return res, side, layer, claims, want[3]


@pytest.fixture(scope="module")
def lookups():
    return {size: LookupCase(*size) for size in LOOKUPS}


@pytest.mark.parametrize("size", LOOKUPS)
def test_a_lookup_is_accepted_and_an_entry_outside_or_a_wrong_m_is_rejected_at_the_fractions(lookups, size):
    c = lookups[size]
    n, k, ref = c.n, c.k, c.ref
    len_f = F.proof_bytes(n, 1)
    res, side, layer, claims, seen = c.both(ref["proof"])
    assert res.accepted and (side, layer) == ("F", 0) and res.offset == len(ref["proof"]) == F.lookup_proof_bytes(n, k)
    for name in ("alpha", "f_value", "t_value", "m_value"):
        assert K.unmont(getattr(claims, name)) == [ref[name]] == [seen[name]], name
    assert K.unmont(claims.z_f) == ref["z_f"] == seen["z_f"] and K.unmont(claims.z_t) == ref["z_t"] == seen["z_t"]
    # the three claims are the tables' extensions: what the caller opens
    assert F.mle_at(c.f, ref["z_f"]) == ref["f_value"] and F.mle_at(c.t, ref["z_t"]) == ref["t_value"] and F.mle_at(c.m, ref["z_t"]) == ref["m_value"]
    (pf, qf), (pt, qt) = ref["fractions"]
    assert (pf * qt - pt * qf) % P == 0
    # a column that is not inside the table, a wrong m: both fractional sums hold, the fractions differ
    for forged in (c.outside, c.wrong_m):
        (pf, qf), (pt, qt) = forged["fractions"]
        assert (pf * qt - pt * qf) % P != 0
        res, side, layer, _, _ = c.both(forged["proof"])
        assert (res.check, side, layer, res.offset) == ("FRACTION", "T", 0, len_f + 128)
    # the parts of the proof: a tampered side names its side and layer, with offsets of the whole proof
    if k > 1:
        res, side, layer, _, _ = c.both(_bump(ref["proof"], len_f // 32 + 4))
        assert (res.check, side, layer, res.offset) == ("SUM", "T", 1, len_f + 160)
    if n > 1:
        res, side, layer, _, _ = c.both(_bump(ref["proof"], 4))
        assert (res.check, side, layer, res.offset) == ("SUM", "F", 1, 160)
    else:
        res, side, layer, _, _ = c.both(_bump(ref["proof"], 0))
        assert (res.check, side, layer, res.offset) == ("UNIT", "F", 0, 128)
    res, side, layer, _, _ = c.both(_set(ref["proof"], len_f // 32 + 3, 0))
    assert (res.check, side, layer, res.offset) == ("DENOMINATOR", "T", 0, len_f + 128)
    for cut in (0, len_f, len(ref["proof"]) - 1):
        res, side, layer, _, _ = c.both(ref["proof"][:cut])
        assert (res.check, side, layer, res.offset) == ("TRANSCRIPT_SHORT", "F", 0, cut)
    assert c.both(ref["proof"] + b"\0")[0].check == "TRAILING_BYTES"
    assert c.both(ref["proof"], pattern=F.lookup_pattern(n, k, 1))[0].check == "IO_PATTERN"
    changed = list(c.bind)
    changed[2] = (changed[2] + 1) % P  # another root: another alpha and other seeds
    res, side, layer, claims, _ = c.both(ref["proof"], bind=changed)
    if n > 1 or k > 1:
        assert (res.check, layer) == ("SUM", 1)
    else:  # no layer to fail: accepted PROVIDED other claims, which the tables do not meet
        assert res.accepted and K.unmont(claims.f_value) != [ref["f_value"]] and F.mle_at(c.f, K.unmont(claims.z_f)) != K.unmont(claims.f_value)[0]


def _blob(head, pat, bind, proofs):
    blob = struct.pack("<%dI" % len(head), *head) + struct.pack("<I", len(pat)) + pat + K.mont(bind).tobytes()
    return blob + struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, lookups, tmp_path):
    """the host verifiers alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan): proofs
    cut at every kind of place and grown, from exact-size heap blocks; statements whose counts would size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkf_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}

    def run(mode, blob):
        f = tmp_path / "cases.bin"
        f.write_bytes(blob)
        p = subprocess.run([ASAN, mode, str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout.splitlines()

    def hostile_set(proof, boundary):
        rng = np.random.default_rng(1)
        hostile = {"honest": proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(proof), "extended": proof + bytes(64),
                   "random bytes": rng.integers(0, 256, size=len(proof), dtype=np.uint8).tobytes(),
                   "random layers": proof[:128] + rng.integers(0, 256, size=len(proof) - 128, dtype=np.uint8).tobytes(),
                   "random tail": proof[:boundary] + rng.integers(0, 256, size=len(proof) - boundary, dtype=np.uint8).tobytes(),
                   "halves swapped": proof[boundary:] + proof[:boundary]}
        for cut in (1, 31, 127, 129, boundary - 1, boundary, boundary + 1, len(proof) - 1):
            hostile[f"cut at {cut}"] = proof[:cut]
        return hostile

    for table in ("random", "unit"):
        c = cases[(5, table)]
        hostile = hostile_set(c.proof, c.layer_at(4))
        for pat in (b"", F.pattern(5, c.unit, 3)):
            lines = run("verify", _blob([5, 3, c.unit], pat, c.bind, list(hostile.values())))
            assert len(lines) == len(hostile)
            for (name, proof), line in zip(hostile.items(), lines):
                rc, accepted, check, side, layer, offset = line.split()[:6]
                want, want_layer, _, _ = F.verify(5, c.unit, proof, c.bind)
                assert (rc, check, accepted, side, layer) == ("0", want, "1" if want == "NONE" else "0", "0", str(want_layer)), (name, line)
                assert int(offset) <= max(len(proof), len(c.proof))
    m = lookups[(4, 3)]
    proof = m.ref["proof"]
    hostile = hostile_set(proof, F.proof_bytes(4, 1))
    hostile["an entry outside the table"] = m.outside["proof"]
    lines = run("lookup", _blob([4, 3, 3], b"", m.bind, list(hostile.values())))
    assert len(lines) == len(hostile)
    for (name, bad), line in zip(hostile.items(), lines):
        rc, accepted, check, side, layer, offset = line.split()[:6]
        want = F.lookup_verify(4, 3, bad, m.bind)
        assert (rc, check, accepted, side, layer) == ("0", want[0], "1" if want[0] == "NONE" else "0", str("FT".index(want[1])), str(want[2])), (name, line)
    for mode, bad in [("verify", [2**31, 0, 0]), ("verify", [5, 2**32 - 1, 0]), ("verify", [0, 0, 0]), ("verify", [29, 0, 1]), ("verify", [5, 0, 2**31]),
                      ("lookup", [2**31, 1, 0]), ("lookup", [5, 2**32 - 1, 0]), ("lookup", [5, 2, 2**30]), ("lookup", [0, 0, 0])]:
        # nothing after the statement: a count that was believed would read past the block
        lines = run(mode, struct.pack("<%dI" % len(bad), *bad))
        assert lines and lines[0].startswith("-1 0 REFUSED"), (bad, lines)
