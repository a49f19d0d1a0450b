"""CPU: libprovekit_grandproduct.so's host side.  The header/library/binding symbol match and what the library links; the two outer
IO patterns and the proof lengths against the reference's; every refusal with its reason; pkg_verify and pkg_multiset_verify on proofs
the Python reference provers build (tests/grandproduct_refs.py): acceptance with the reference's product, point and value, and every
tampering with the check and the layer both verifiers must name; hostile framing through the sanitizer build of the host verifiers (a
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
HEADER = os.path.join(ROOT, "include", "provekit_grandproduct.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkg_verify_asan")

import grandproduct_refs as G  # noqa: E402
import prodcheck_refs as K  # noqa: E402

P = K.P


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import grandproduct as gp

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkg_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", gp.GRANDPRODUCT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkg_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(gp.SIGNATURES) and len(exported) == 20
    assert ctypes.CDLL(gp.GRANDPRODUCT_LIB_PATH).pkg_abi_version() == 1
    assert ctypes.sizeof(gp.MultisetClaimsStruct) == 32 * (4 + 2 * 28) and ctypes.sizeof(gp.StatementStruct) == 8 and ctypes.sizeof(gp.MultisetStatementStruct) == 12
    # pks's check numbers unchanged, one new one after them
    assert [gp.lib.pkg_check_name(i).decode() for i in range(len(gp.CHECKS))] == list(gp.CHECKS) and gp.CHECKS[-1] == "PRODUCT" and len(gp.CHECKS) == 22
    assert re.search(r"#define PKG_CHECK_PRODUCT PKS_CHECK_COUNT\b", open(HEADER).read())
    # the library calls the product and the sumcheck library only through their C ABIs, and no other library above the product
    und = subprocess.run(["nm", "-D", "--undefined-only", gp.GRANDPRODUCT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\b_ZN3pks\w+", und) and not re.findall(r"\bpk[vwl]_\w+", und), und
    inc = os.path.join(ROOT, "include")
    assert set(re.findall(r"\bpk_\w+", und)) <= set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", open(os.path.join(inc, "provekit_hip.h")).read()))
    called = set(re.findall(r"\bpks_\w+", und))
    assert {"pks_prove", "pks_verify", "pks_prover_create"} <= called <= set(re.findall(r"\b(pks_[a-z0-9_]+)\s*\(", open(os.path.join(inc, "provekit_sumcheck.h")).read()))
    needed = subprocess.run(["readelf", "-d", gp.GRANDPRODUCT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    libs = set(re.findall(r"\[(libprovekit_\w+\.so)\]", needed))
    assert libs == {"libprovekit_sumcheck.so", "libprovekit_hip.so"}, libs


def test_io_patterns_and_proof_lengths_are_the_references_and_differ_between_statements():
    from provekit_amd import grandproduct as gp

    pats = {}
    for n in (1, 2, 3, 8, 28):
        for n_bind in (0, 3, 16):
            stmt = gp.Statement(n, n_bind)
            pats[(n, n_bind)] = gp.io_pattern(stmt)
            assert pats[(n, n_bind)] == G.pattern(n, n_bind), (n, n_bind)
            assert gp.proof_bytes(stmt) == G.proof_bytes(n) == 64 + 48 * (n - 1) * (n + 2)
            for w in (1, 2, 4):
                ms = gp.MultisetStatement(n, w, n_bind)
                pats[(n, w, n_bind)] = gp.io_pattern(ms)
                assert pats[(n, w, n_bind)] == G.multiset_pattern(n, w, n_bind), (n, w, n_bind)
                assert gp.proof_bytes(ms) == G.multiset_proof_bytes(n) == 2 * gp.proof_bytes(stmt)
    assert len(set(pats.values())) == len(pats)
    assert pats[(1, 0)].split(b"\0") == [gp.LABEL + b"/n1", b"A2top", b"S1rho"]
    assert pats[(3, 3)].split(b"\0") == [gp.LABEL + b"/n3", b"A3bind", b"A2top", b"S1rho"] + [b"S1seed", b"A2finals", b"S1rho"] * 2
    # w = 1: no beta squeeze
    assert pats[(8, 1, 3)].split(b"\0") == [gp.MULTISET_LABEL + b"/n8/w1", b"A3bind", b"S1gamma", b"S2seeds"]
    assert pats[(8, 2, 0)].split(b"\0") == [gp.MULTISET_LABEL + b"/n8/w2", b"S1gamma", b"S1beta", b"S2seeds"]


def test_arena_bytes_states_the_tree_and_the_sumcheck_arenas():
    from provekit_amd import grandproduct as gp

    for n in (1, 2, 12, 28):
        total = gp.arena_bytes(gp.Statement(n))
        tree, sumchecks = 32 * 2**n, 32 * sum(2 * 2 ** (d - 1) for d in range(1, n))  # the layers' folded copies
        # per layer: one round's scratch (4104 elements) and the split eq tables (at most 3 * 2^14 elements, at d = 28)
        assert tree + sumchecks <= total <= tree + sumchecks + (n - 1) * 2**21
    assert 1 <= gp.tail_max_n() <= 12  # 2^(t-1) elements of 32 bytes in the 64 KiB of LDS a kernel gets without asking


@pytest.mark.parametrize("kind, stmt, reason", [
    ("gp", (0,), "n must be"), ("gp", (29,), "n must be"), ("gp", (4, 17), "n_bind must be"),
    ("ms", (0, 1), "n must be"), ("ms", (29, 1), "n must be"), ("ms", (4, 0), "w must be"), ("ms", (4, 5), "w must be"), ("ms", (4, 2, 17), "n_bind must be"),
])
def test_every_refusal_is_made_with_a_reason(kind, stmt, reason):
    from provekit_amd import grandproduct as gp
    from provekit_amd._lib import ProveKitHipError

    s = gp.Statement(*stmt) if kind == "gp" else gp.MultisetStatement(*stmt)
    for call in (gp.io_pattern, gp.proof_bytes) + ((gp.arena_bytes,) if kind == "gp" else ()):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r = s.struct(), gp.ResultStruct()  # the verifiers refuse the statement before they look at anything else
    if kind == "gp":
        rc = gp.lib.pkg_verify(ctypes.addressof(st), None, 0, None, None, None, 0, None, None, None, None, ctypes.byref(r))
    else:
        rc = gp.lib.pkg_multiset_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r))
    assert rc == -1 and re.search(reason, gp.lib.pkg_create_error().decode())


def test_verify_refuses_bind_elements_that_do_not_match_the_statement():
    from provekit_amd import grandproduct as gp
    from provekit_amd._lib import ProveKitHipError

    too_big = np.array([[2**64 - 1] * 4], dtype=np.uint64)
    for s, call in ((gp.Statement(3, 1), lambda st, r: gp.lib.pkg_verify(ctypes.addressof(st), None, 0, None, None, None, 0, None, None, None, None, ctypes.byref(r))),
                    (gp.MultisetStatement(3, 2, 1), lambda st, r: gp.lib.pkg_multiset_verify(ctypes.addressof(st), None, 0, None, None, 0, None, None, None, ctypes.byref(r)))):
        st, r = s.struct(), gp.ResultStruct()
        assert call(st, r) == -1 and b"binds elements: pass" in gp.lib.pkg_create_error()  # NULL where elements are due
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p") as e:
        gp.verify(gp.Statement(3, 1), b"", bind=too_big)
    assert e.value.code == -1
    with pytest.raises(ProveKitHipError, match="bind element 0 is not below p"):
        gp.multiset_verify(gp.MultisetStatement(3, 2, 1), b"", bind=too_big)
    with pytest.raises(ProveKitHipError, match="expected_product element 0 is not below p"):
        gp.verify(gp.Statement(3, 0), b"", expected_product=too_big)


SIZES = [1, 2, 3, 5]
TABLES = ("random", "zeros", "ones")


class Case:
    def __init__(self, n, table):
        self.n = n
        self.v = {"random": lambda: G.random_table(n, seed=n), "zeros": lambda: G.random_table(n, seed=n + 50, zeros=(0, (1 << n) - 1)),
                  "ones": lambda: [1] * (1 << n)}[table]()
        self.bind = K.random_elements(3, seed=5)
        self.ref = G.prove(n, self.v, self.bind)
        self.proof = self.ref["proof"]

    def both(self, proof=None, bind=None, pattern=None, expected=None):
        """the library's verdict, after asserting that the reference names the same check and layer"""
        from provekit_amd import grandproduct as gp

        proof = self.proof if proof is None else proof
        bind = self.bind if bind is None else bind
        check, layer, ref = G.verify(self.n, proof, bind, pattern, expected)
        res, lib_layer, out = gp.verify(gp.Statement(self.n, 3), proof, K.mont(bind), None if expected is None else K.mont([expected]), pattern)
        assert (res.check, lib_layer) == (check, layer) and res.accepted == (check == "NONE"), (res, lib_layer, check, layer)
        return res, lib_layer, out, ref


@pytest.fixture(scope="module")
def cases():
    return {(n, t): Case(n, t) for n in SIZES for t in TABLES if t == "random" or n in (2, 5)}


@pytest.mark.parametrize("n, table", [(n, t) for n in SIZES for t in TABLES if t == "random" or n in (2, 5)])
def test_reference_proofs_are_accepted_with_the_references_product_point_and_value(cases, n, table):
    c = cases[(n, table)]
    ref = c.ref
    assert len(c.proof) == G.proof_bytes(n) and [int.from_bytes(c.proof[32 * i : 32 * i + 32], "little") for i in (0, 1)] == ref["layers"][1]
    # the reference proves what it says: P is the table's product and the claim is the table's extension at the point
    want = 1
    for x in c.v:
        want = want * x % P
    assert ref["P"] == want == {"zeros": 0, "ones": 1}.get(table, want) and ref["value"] == G.mle_at(c.v, ref["point"])
    for kw in ({}, {"pattern": G.pattern(n, 3)}, {"expected": ref["P"]}):
        res, layer, out, seen = c.both(**kw)
        assert res.accepted and res.check == "NONE" and layer == 0 and res.offset == len(c.proof) and res.message == ""
        assert K.unmont(out[0]) == [ref["P"]] == [seen["P"]] and K.unmont(out[1]) == ref["point"] == seen["point"]
        assert K.unmont(out[2]) == [ref["value"]] == [seen["value"]]


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


@pytest.mark.parametrize("n", SIZES)
def test_every_tampering_is_rejected_at_the_named_check_and_layer(cases, n):
    c = cases[(n, "random")]
    at = [None] + [G.layer_at(d) // 32 for d in range(1, n + 1)]  # in elements: at[d] is layer d's s
    # either top value: another claim c_1, so layer 1's stated sum is not it; at n = 1 there is no layer and another product is accepted
    for e in (0, 1):
        res, layer, _, _ = c.both(_bump(c.proof, e))
        assert (res.check, layer) == (("SUM", 1) if n > 1 else ("NONE", 0))
        assert c.both(_bump(c.proof, e), expected=c.ref["P"])[0].check == "PRODUCT"
    for d in range(1, n):
        # s is checked against the running claim; a round value against the claim of its round; a final against the last claim
        res, layer, _, _ = c.both(_bump(c.proof, at[d]))
        assert (res.check, layer, res.offset) == ("SUM", d, 32 * (at[d] + 1))
        for i in range(d):
            res, layer, _, _ = c.both(_bump(c.proof, at[d] + 1 + 3 * i))
            assert (res.check, layer) == ("ROUND", d) and f"round {i}:" in res.message and res.offset == 32 * (at[d] + 1 + 3 * (i + 1))
        for j in range(2):
            res, layer, _, _ = c.both(_bump(c.proof, at[d] + 1 + 3 * d + j))
            assert (res.check, layer, res.offset) == ("FINAL", d, 32 * at[d + 1])
    # a bind element enters nothing but the challenges: rho_1 and so c_1 change
    for e in range(3):
        changed = list(c.bind)
        changed[e] = (changed[e] + 1) % P
        res, layer, _, _ = c.both(bind=changed)
        assert (res.check, layer) == (("SUM", 1) if n > 1 else ("NONE", 0))
    # framing: every part has a fixed length
    for cut in sorted({0, 31, 64, G.layer_at(max(n - 1, 1)), len(c.proof) - 1} - {len(c.proof)}):
        res, layer, _, _ = c.both(c.proof[:cut])
        assert (res.check, layer, res.offset) == ("TRANSCRIPT_SHORT", 0, cut)
    for extra in (b"\0", bytes(32)):
        res, layer, _, _ = c.both(c.proof + extra)
        assert (res.check, layer, res.offset) == ("TRAILING_BYTES", 0, len(c.proof))
    # v + p: the same value mod p, not canonical on the wire
    for element, want_layer in [(0, 0), (1, 0)] + [(at[d] + 1, d) for d in range(1, n)] + [(at[d + 1] - 1, d) for d in range(1, n)]:
        t = bytearray(c.proof)
        v = int.from_bytes(t[32 * element : 32 * element + 32], "little") + P
        if v < 1 << 256:
            t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
            res, layer, _, _ = c.both(bytes(t))
            assert (res.check, layer, res.offset) == ("NON_CANONICAL", want_layer, 32 * (element + 1))
    # another statement's pattern: other operations are IO_PATTERN; the same operations under another label are other challenges
    res, layer, _, _ = c.both(pattern=G.pattern(n, 2))
    assert (res.check, layer) == ("IO_PATTERN", 0)
    res, layer, _, _ = c.both(pattern=G.pattern(n + 1, 3))
    assert (res.check, layer) == (("SUM", 1) if n > 1 else ("IO_PATTERN", 0))
    res, layer, _, _ = c.both(pattern=G.pattern(n, 3).replace(b"/v1/", b"/v2/"))
    assert (res.check, layer) == (("SUM", 1) if n > 1 else ("NONE", 0))
    # a wrong expected product: judged at the top, before any layer
    res, layer, _, _ = c.both(expected=(c.ref["P"] + 1) % P)
    assert (res.check, layer, res.offset) == ("PRODUCT", 0, 64)


MULTISET = [(1, 1), (3, 1), (3, 2), (4, 4)]


class MultisetCase:
    def __init__(self, n, w):
        rng = np.random.default_rng(10 * n + w)
        self.n, self.w = n, w
        self.a = [K.random_elements(1 << n, seed=100 * n + 10 * w + j) for j in range(w)]
        perm = rng.permutation(1 << n)
        self.b = [[col[i] for i in perm] for col in self.a]
        self.bind = K.random_elements(2, seed=9)
        self.ref = G.multiset_prove(n, self.a, self.b, self.bind)
        changed = [list(col) for col in self.b]
        changed[w - 1][(1 << n) - 1] = (changed[w - 1][(1 << n) - 1] + 1) % P  # one row, in its last column
        self.forged = G.multiset_prove(n, self.a, changed, self.bind, validate=False)
        self.changed = changed

    def both(self, proof, bind=None, pattern=None):
        from provekit_amd import grandproduct as gp

        bind = self.bind if bind is None else bind
        want = G.multiset_verify(self.n, self.w, proof, bind, pattern)
        res, side, layer, claims = gp.multiset_verify(gp.MultisetStatement(self.n, self.w, 2), proof, K.mont(bind), pattern)
        assert (res.check, side, layer) == want[:3] and res.accepted == (want[0] == "NONE"), (res, side, layer, want[:3])
        return res, side, layer, claims, want[3]


@pytest.fixture(scope="module")
def multisets():
    return {size: MultisetCase(*size) for size in MULTISET}


@pytest.mark.parametrize("size", MULTISET)
def test_a_permuted_side_is_accepted_and_a_changed_row_is_rejected_at_the_products(multisets, size):
    c = multisets[size]
    n, w, ref = c.n, c.w, c.ref
    res, side, layer, claims, seen = c.both(ref["proof"])
    assert res.accepted and (side, layer) == ("A", 0) and res.offset == len(ref["proof"]) == G.multiset_proof_bytes(n)
    for name in ("gamma", "beta", "comb_a", "comb_b"):
        assert K.unmont(getattr(claims, name)) == [ref[name]] == [seen[name]], name
    assert K.unmont(claims.z_a) == ref["z_a"] == seen["z_a"] and K.unmont(claims.z_b) == ref["z_b"] == seen["z_b"]
    assert (ref["beta"] == 1) == (w == 1) and ref["products"][0] == ref["products"][1]
    # the claims are the columns' extensions, combined: what the caller opens
    for cols, z, comb in ((c.a, ref["z_a"], ref["comb_a"]), (c.b, ref["z_b"], ref["comb_b"])):
        assert sum(pow(ref["beta"], j, P) * G.mle_at(col, z) for j, col in enumerate(cols)) % P == comb
    # unequal multisets: both grand products hold, their products differ
    assert c.forged["products"][0] != c.forged["products"][1]
    res, side, layer, _, _ = c.both(c.forged["proof"])
    assert (res.check, side, layer, res.offset) == ("PRODUCT", "B", 0, len(ref["proof"]) // 2 + 64)
    # the parts of the proof: a tampered side B names side B and its layer, with offsets of the whole proof
    half = len(ref["proof"]) // 2
    if n > 1:
        res, side, layer, _, _ = c.both(_bump(ref["proof"], half // 32 + 2))
        assert (res.check, side, layer, res.offset) == ("SUM", "B", 1, half + 96)
        res, side, layer, _, _ = c.both(_bump(ref["proof"], 2))
        assert (res.check, side, layer, res.offset) == ("SUM", "A", 1, 96)
    for cut in (0, half, len(ref["proof"]) - 1):
        res, side, layer, _, _ = c.both(ref["proof"][:cut])
        assert (res.check, side, layer, res.offset) == ("TRANSCRIPT_SHORT", "A", 0, cut)
    assert c.both(ref["proof"] + b"\0")[0].check == "TRAILING_BYTES"
    assert c.both(ref["proof"], pattern=G.multiset_pattern(n, w, 1))[0].check == "IO_PATTERN"
    assert c.both(ref["proof"], pattern=G.multiset_pattern(n, 3 - w if w < 3 else 1, 2))[0].check == "IO_PATTERN"  # a beta squeeze more or less


def _blob(head, pat, bind, proofs):
    blob = struct.pack("<%dI" % len(head), *head) + struct.pack("<I", len(pat)) + pat + K.mont(bind).tobytes()
    return blob + struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs)


def test_hostile_framing_and_counts_under_the_sanitizers(cases, multisets, tmp_path):
    """the host verifiers alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan): proofs
    cut at every kind of place and grown, from exact-size heap blocks; statements whose counts would size buffers if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkg_verify_asan is missing: make -C provekit_amd/csrc asan"
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
                   "random layers": proof[:64] + rng.integers(0, 256, size=len(proof) - 64, dtype=np.uint8).tobytes(),
                   "random tail": proof[:boundary] + rng.integers(0, 256, size=len(proof) - boundary, dtype=np.uint8).tobytes(),
                   "halves swapped": proof[boundary:] + proof[:boundary]}
        for cut in (1, 31, 63, 65, boundary - 1, boundary, boundary + 1, len(proof) - 1):
            hostile[f"cut at {cut}"] = proof[:cut]
        return hostile

    c = cases[(5, "random")]
    hostile = hostile_set(c.proof, G.layer_at(4))
    for pat in (b"", G.pattern(5, 3)):
        lines = run("verify", _blob([5, 3], pat, c.bind, list(hostile.values())))
        assert len(lines) == len(hostile)
        for (name, proof), line in zip(hostile.items(), lines):
            rc, accepted, check, side, layer, offset = line.split()[:6]
            want, want_layer, _ = G.verify(5, proof, c.bind)
            assert (rc, check, accepted, side, layer) == ("0", want, "1" if want == "NONE" else "0", "0", str(want_layer)), (name, line)
            assert int(offset) <= max(len(proof), len(c.proof))
    m = multisets[(3, 2)]
    proof = m.ref["proof"]
    hostile = hostile_set(proof, len(proof) // 2)
    hostile["unequal multisets"] = m.forged["proof"]
    lines = run("multiset", _blob([3, 2, 2], b"", m.bind, list(hostile.values())))
    assert len(lines) == len(hostile)
    for (name, bad), line in zip(hostile.items(), lines):
        rc, accepted, check, side, layer, offset = line.split()[:6]
        want = G.multiset_verify(3, 2, bad, m.bind)
        assert (rc, check, accepted, side, layer) == ("0", want[0], "1" if want[0] == "NONE" else "0", str("AB".index(want[1])), str(want[2])), (name, line)
    for mode, bad in [("verify", [2**31, 0]), ("verify", [5, 2**32 - 1]), ("verify", [0, 0]), ("verify", [29, 0]),
                      ("multiset", [2**31, 1, 0]), ("multiset", [5, 2**32 - 1, 0]), ("multiset", [5, 2, 2**30]), ("multiset", [0, 0, 0])]:
        # nothing after the statement: a count that was believed would read past the block
        lines = run(mode, struct.pack("<%dI" % len(bad), *bad))
        assert lines and lines[0].startswith("-1 0 REFUSED"), (bad, lines)
