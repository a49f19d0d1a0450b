"""CPU: the wide product sumcheck's host side (include/provekit_sumcheck_wide.h, pksw_* in libprovekit_sumcheck.so).  The
header/library/binding symbol match next to the unchanged pks_* list; pksw_io_pattern and pksw_proof_bytes against the reference's for
every catalogue entry (tests/prodcheck_wide_refs.py); every refusal with its reason; pksw_verify on proofs the Python reference prover
builds: acceptance, and the check and offset it names for each tampering; the wide kernel's lane arithmetic compiled for the host, for
every entry and at the value bound, and the wide verifier over case files, both through the sanitizer build (a program of its own, run
as a subprocess); the catalogue held to wide.hip's dispatch list."""
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
HEADER = os.path.join(ROOT, "include", "provekit_sumcheck_wide.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pks_verify_asan")
WIDE_HIP = os.path.join(ROOT, "provekit_amd", "csrc", "sumcheck", "wide.hip")

import prodcheck_refs as K  # noqa: E402
import prodcheck_wide_refs as W  # noqa: E402

P = W.P
EVERY = list(W.CATALOGUE)
MIDDLE = 5  # a few variables: the verifier's work is per round


def test_the_catalogue_holds_what_it_must_and_reaches_every_instantiation_wide_hip_dispatches():
    """wide.hip dispatches on D (its PKSW_DEGREE uses) and on the fold; a prover of n >= 2 launches both folds of its D"""
    src = open(WIDE_HIP).read()
    dispatched = {int(d) for d in re.findall(r"PKSW_DEGREE\((\d+)\)", src)}
    assert dispatched == {1, 2, 3, 4, 5} and "PKS_CASE(" not in src
    assert re.search(r"if \(fold\)\s+wide_round_kernel<D, true>.*\s+else\s+wide_round_kernel<D, false>", src)
    shapes = {name: W.Shape(name, 2) for name in EVERY}
    assert {s.D for s in shapes.values()} == dispatched
    for d in dispatched:  # with and without tau
        assert {s.has_tau for s in shapes.values() if s.D == d} == {True, False}, d
    assert (shapes["plonk"].m, len(shapes["plonk"].terms), shapes["plonk"].D, shapes["plonk"].has_tau) == (8, 5, 3, True)
    assert (shapes["pow5"].m, shapes["pow5"].terms) == (1, [(1, [0] * 5)])
    assert shapes["a2b3c"].terms == [(1, [0, 0, 1, 1, 1]), (P - 1, [2])] and shapes["a2b3c"].has_tau
    assert (shapes["wide16"].m, len(shapes["wide16"].terms)) == (16, 16) and all(0 in f for _, f in shapes["wide16"].terms)
    assert shapes["lin16"].m == 16 and shapes["lin16"].D == 1 and sorted(f[0] for _, f in shapes["lin16"].terms) == list(range(16))
    assert {0, 1, P - 1} < {c for c, _ in shapes["coeffs"].terms} and len({c for c, _ in shapes["coeffs"].terms}) >= 5
    assert shapes["twice"].terms[0][1] == shapes["twice"].terms[1][1]
    assert len(W.TRANSLATED) == 12 and set(W.TRANSLATED.values()) == set(K.SHAPES) | set(K.FORMS)
    assert [shapes[name].D for name in W.ONE_PER_DEGREE] == [1, 2, 3, 4, 5]
    for s in shapes.values():
        assert all(list(f) == sorted(f) and 1 <= len(f) <= 5 for _, f in s.terms) and {j for _, f in s.terms for j in f} == set(range(s.m))


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import prodcheck, prodcheck_wide

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pksw_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", prodcheck.SUMCHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pksw_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(prodcheck_wide.SIGNATURES) and len(exported) == 11
    assert exported == sorted(["pksw_abi_version", "pksw_create_error", "pksw_io_pattern", "pksw_proof_bytes", "pksw_arena_bytes", "pksw_prover_create",
                               "pksw_prover_destroy", "pksw_last_error", "pksw_prove", "pksw_verify", "pksw_round"])
    assert len(set(re.findall(r" [A-Za-z] (pks_[a-z0-9_]+)$", nm, flags=re.M))) == 11 == len(prodcheck.SIGNATURES)
    assert prodcheck_wide.lib.pksw_abi_version() == 1
    assert (prodcheck_wide.MAX_TABLES, prodcheck_wide.MAX_TERMS, prodcheck_wide.MAX_DEGREE) == (16, 16, 5)
    for name, value in (("PKSW_MAX_TABLES", 16), ("PKSW_MAX_TERMS", 16), ("PKSW_MAX_DEGREE", 5)):
        assert re.search(r"#define %s %d\b" % (name, value), src)
    assert ctypes.sizeof(prodcheck_wide.StatementStruct) == 4 * (5 + 16 + 80) + 4 + 32 * 16


def test_io_pattern_and_proof_size_are_the_references_for_every_entry_and_all_patterns_differ():
    from provekit_amd import prodcheck, prodcheck_wide

    pats = {}
    for name in EVERY:
        for n, n_bind in ((1, 0), (MIDDLE, 2), (28, 16)):
            shape = W.Shape(name, n, n_bind)
            pat = prodcheck_wide.io_pattern(shape.statement())
            assert pat == shape.pattern(), (name, n, n_bind)
            assert prodcheck_wide.proof_bytes(shape.statement()) == shape.proof_bytes()
            pats[(name, n, n_bind)] = pat
    assert len(set(pats.values())) == len(pats)
    head = pats[("plonk", MIDDLE, 2)].split(b"\0")
    assert head[0] == b"provekit-hip/sumcheck-wide/v1/n5/m8/T5/tau1/terms0.5-1.6-2.5.6-3.7-4" and prodcheck_wide.LABEL == W.LABEL
    assert head[1:6] == [b"A2bind", b"A5tau", b"A5coefficients", b"A1sum", b"A4round_values"] and head[-1] == b"A8final_values"
    assert pats[("pow5", 1, 0)].split(b"\0") == [W.LABEL + b"/n1/m1/T1/tau0/terms0.0.0.0.0", b"A1coefficients", b"A1sum", b"A6round_values", b"S1challenge",
                                                 b"A1final_values"]
    # a statement both interfaces take: the same operations, another label -- the two are not interchangeable on the wire
    for wide, name in W.TRANSLATED.items():
        a, b = pats[(wide, MIDDLE, 2)].split(b"\0"), prodcheck.io_pattern(K.Shape(name, MIDDLE, 2).statement()).split(b"\0")
        assert a[1:] == b[1:] and a[0] != b[0] and a[0].startswith(W.LABEL + b"/") and not b[0].startswith(W.LABEL)


def test_arena_bytes_is_the_folded_copies_the_wide_scratch_and_the_split_eq_tables():
    from provekit_amd import prodcheck_wide

    for name, n in (("plonk", 20), ("pow5", 1), ("wide16", 28), ("lin16", 9)):
        shape = W.Shape(name, n)
        R = n - 1
        eq = (2 << (R - R // 2)) + (2 << (R // 2)) - 2
        assert prodcheck_wide.arena_bytes(shape.statement()) == 32 * (shape.m * (1 << (n - 1)) + 6 * 1024 + 8 + eq)


BIG = [(P >> (64 * i)) & (2**64 - 1) for i in range(4)]


@pytest.mark.parametrize("stmt, reason", [
    ((0, 2, [(1, [0, 1])]), "n must be"), ((29, 2, [(1, [0, 1])]), "n must be"),
    ((4, 0, [(1, [0])]), "m must be"), ((4, 17, [(1, [j]) for j in range(16)]), "m must be"),
    ((4, 2, []), "T must be"), ((4, 2, [(1, [0, 1])] * 17), "T must be"),
    ((4, 2, [(1, [0, 1])], False, 17), "n_bind must be"),
    ((4, 2, [(1, [0, 1])], 2), "has_tau must be"),
    ((4, 2, [(1, [1, 0])]), "not non-decreasing"), ((4, 3, [(1, [0, 2, 1])]), "not non-decreasing"),
    ((4, 2, [(1, [0, 1]), (1, [])]), "empty list"),
    ((4, 2, [(1, [0, 0, 0, 1, 1, 1])]), "more than 5 factors"),
    ((4, 2, [(1, [0, 2])]), "names a table >= m"), ((4, 2, [(1, [0, 1, 2**31])]), "names a table >= m"),
    ((4, 3, [(1, [0, 1])]), "used by no term"), ((4, 16, [(1, [j]) for j in range(15)]), "used by no term"),
    ((4, 2, [(BIG, [0, 1])]), "not below p"), ((4, 2, [(1, [0]), ([2**64 - 1] * 4, [1])]), "not below p"),
])
def test_every_refusal_is_made_with_a_reason(stmt, reason):
    from provekit_amd import prodcheck_wide
    from provekit_amd._lib import ProveKitHipError

    s = prodcheck_wide.Statement(*stmt)
    if reason == "has_tau must be":
        s.has_tau = 2
    for call in (prodcheck_wide.io_pattern, prodcheck_wide.proof_bytes, prodcheck_wide.arena_bytes):
        with pytest.raises(ProveKitHipError, match=reason) as e:
            call(s)
        assert e.value.code == -1
    st, r = s.struct(), prodcheck_wide.ResultStruct()  # the verifier refuses the statement before it looks at anything else
    assert prodcheck_wide.lib.pksw_verify(ctypes.addressof(st), None, 0, None, None, None, None, 0, None, None, ctypes.byref(r)) == -1
    assert re.search(reason, prodcheck_wide.lib.pksw_create_error().decode())


def test_verify_refuses_a_tau_or_bind_that_does_not_match_the_statement():
    from provekit_amd import prodcheck_wide
    from provekit_amd._lib import ProveKitHipError

    s = prodcheck_wide.Statement(3, 1, [(1, [0, 0])], has_tau=True, n_bind=1)
    st, r = s.struct(), prodcheck_wide.ResultStruct()
    one = W.mont([1, 1, 1])
    for tau, bind, reason in ((None, one.ctypes.data, b"has a tau"), (one.ctypes.data, None, b"binds elements")):
        assert prodcheck_wide.lib.pksw_verify(ctypes.addressof(st), None, 0, tau, bind, None, None, 0, None, None, ctypes.byref(r)) == -1
        assert reason in prodcheck_wide.lib.pksw_create_error()
    with pytest.raises(ProveKitHipError, match="not below p"):
        prodcheck_wide.verify(s, b"", tau=np.array([[2**64 - 1] * 4] * 3, dtype=np.uint64), bind=one[:1])


class Case:
    def __init__(self, name):
        self.shape = W.Shape(name, MIDDLE, n_bind=2)
        self.stmt = self.shape.statement()
        self.tables = W.random_tables(self.shape.m, self.shape.n, seed=len(name))
        self.tau = W.random_elements(self.shape.n, seed=7) if self.shape.has_tau else None
        self.bind = W.random_elements(2, seed=9)
        self.proof, self.point, self.finals, self.s = W.prove(self.shape, self.tables, self.tau, self.bind)

    def both(self, proof=None, tau="own", bind=None, expected_sum=None, pattern=None):
        """the library's verdict, after asserting that the reference's is the same check"""
        from provekit_amd import prodcheck_wide

        proof = self.proof if proof is None else proof
        tau = self.tau if tau == "own" else tau
        bind = self.bind if bind is None else bind
        ref, _, _ = W.verify(self.shape, proof, tau, bind, expected_sum, pattern)
        res, point, finals = prodcheck_wide.verify(self.stmt, proof, W.mont(tau) if tau is not None else None, W.mont(bind),
                                                   W.mont([expected_sum]) if expected_sum is not None else None, pattern)
        assert res.check == ref and res.accepted == (ref == "NONE"), (res, ref)
        return res, point, finals


@pytest.fixture(scope="module")
def cases():
    return {name: Case(name) for name in EVERY}


@pytest.mark.parametrize("name", EVERY)
def test_reference_proofs_are_accepted_with_the_references_point_and_finals(cases, name):
    c = cases[name]
    assert len(c.proof) == c.shape.proof_bytes() and int.from_bytes(c.proof[:32], "little") == c.s
    # the reference proves what it says: s is the sum, the finals are the tables' extensions at the point
    w = W.pr.eq_table(c.tau) if c.tau is not None else [1] * (1 << c.shape.n)
    assert c.s == sum(w[x] * c.shape.terms_at([t[x] for t in c.tables]) for x in range(1 << c.shape.n)) % P
    eq_r = W.pr.eq_table(c.point)
    assert c.finals == [sum(e * v for e, v in zip(eq_r, t)) % P for t in c.tables]
    for kw in ({}, {"pattern": c.shape.pattern()}, {"expected_sum": c.s}):
        res, point, finals = c.both(**kw)
        assert res.accepted and res.check == "NONE" and res.offset == len(c.proof) and res.message == ""
        assert W.unmont(point) == c.point and W.unmont(finals) == c.finals


@pytest.mark.parametrize("wide", list(W.TRANSLATED))
def test_a_translated_statement_has_the_round_0_of_the_product_sumchecks_reference(wide):
    """prodcheck_refs.prove is written apart from round_values; under the two labels the challenges differ, round 0 and s do not"""
    name = W.TRANSLATED[wide]
    a, b = W.Shape(wide, MIDDLE), K.Shape(name, MIDDLE)
    assert (a.m, a.D, a.has_tau, [c for c, _ in a.terms]) == (b.m, b.D, b.has_tau, [c for c, _ in b.terms])
    tables = W.random_tables(a.m, MIDDLE, seed=3)
    tau = W.random_elements(MIDDLE, seed=4) if a.has_tau else None
    pa, pb = W.prove(a, tables, tau)[0], K.prove(b, tables, tau)[0]
    assert pa[: 32 * (2 + a.D)] == pb[: 32 * (2 + a.D)] and pa != pb
    v = W.random_elements(a.m, seed=5)
    assert a.terms_at(v) == b.terms_at(v)
    # ... and pksw_verify accepts the wide reference's proof of it, with the sum pks_verify accepts for the other
    from provekit_amd import prodcheck, prodcheck_wide

    s = W.mont([int.from_bytes(pa[:32], "little")])
    tau_a = W.mont(tau) if tau is not None else None
    assert prodcheck_wide.verify(a.statement(), pa, tau_a, expected_sum=s)[0].accepted and prodcheck.verify(b.statement(), pb, tau_a, expected_sum=s)[0].accepted
    assert prodcheck_wide.verify(a.statement(), pb, tau_a)[0].check == "ROUND"  # the other label's proof: other challenges


def _bump(proof, element, delta=1):
    t = bytearray(proof)
    v = (int.from_bytes(t[32 * element : 32 * element + 32], "little") + delta) % P
    t[32 * element : 32 * element + 32] = v.to_bytes(32, "little")
    return bytes(t)


@pytest.mark.parametrize("name", EVERY)
def test_every_tampering_is_rejected_at_the_named_check_and_offset(cases, name):
    c = cases[name]
    n, D, m = c.shape.n, c.shape.D, c.shape.m
    for i in (0, n - 1):  # a changed h_i(0) enters round i's own check: the first and the last round
        res, _, _ = c.both(_bump(c.proof, 1 + i * (D + 1)))
        assert res.check == "ROUND" and f"round {i}:" in res.message and res.offset == 32 * (1 + (i + 1) * (D + 1))
    if D > 1:  # h_i(D) enters only the next claim: the round after it, or the final check after the last round
        res, _, _ = c.both(_bump(c.proof, 1 + D))
        assert res.check == "ROUND" and "round 1:" in res.message and res.offset == 32 * (1 + 2 * (D + 1))
        res, _, _ = c.both(_bump(c.proof, 1 + (n - 1) * (D + 1) + D))
        assert res.check == "FINAL" and res.offset == len(c.proof)
    for j in range(m):  # a final value the terms do not depend on is no tampering with the claim, by the statement's own terms
        changed = [(v + 1) % P if k == j else v for k, v in enumerate(c.finals)]
        cancelled = c.shape.terms_at(changed) == c.shape.terms_at(c.finals)
        assert cancelled == (name == "pks_lin2rep" and j == 0)
        res, _, _ = c.both(_bump(c.proof, 1 + n * (D + 1) + j))
        assert res.check == ("NONE" if cancelled else "FINAL") and res.offset == len(c.proof)
    res, _, _ = c.both(expected_sum=(c.s + 1) % P)
    assert res.check == "SUM" and res.offset == 32
    res, _, _ = c.both(_bump(c.proof, 0))
    assert res.check == "ROUND" and "round 0:" in res.message and res.offset == 32 * (2 + D)
    assert c.both(_bump(c.proof, 0), expected_sum=c.s)[0].check == "SUM"
    for cut in (0, 31, 32, 32 * (2 + D), len(c.proof) - 1):
        assert c.both(c.proof[:cut])[0].check == "TRANSCRIPT_SHORT"
    res, _, _ = c.both(c.proof + b"\0")
    assert res.check == "TRAILING_BYTES" and res.offset == len(c.proof)
    other = W.Shape("pow5" if name != "pow5" else "plonk", n, 2)
    assert c.both(pattern=other.pattern())[0].check in ("IO_PATTERN", "ROUND")  # as the reference says: absorbs may run across operations
    assert c.both(pattern=c.shape.pattern().replace(b"/v1/", b"/v2/"))[0].check == "ROUND"


def _hex(v):
    return "%064x" % v


def _lane(shape, lo, hi, weighted, w, repeats, env):
    terms = [a for c, factors in shape.terms for a in (".".join(map(str, factors)), _hex(c * K.R % P))]
    pairs = [_hex(v) for lh in zip(lo, hi) for v in lh]
    p = subprocess.run([ASAN, "wide", "lane", str(shape.D), str(shape.m), str(len(shape.terms)), str(int(weighted)), _hex(w), str(repeats)] + terms + pairs,
                       capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = [int(line, 16) for line in p.stdout.split()]
    # an image x stands for x R^-1; the sums come back as images
    weight = w * K.R_INV % P if weighted else 1
    want = [repeats * weight * shape.terms_at([(a + X * (b - a)) * K.R_INV % P for a, b in zip(lo, hi)]) * K.R % P for X in range(shape.D + 1)]
    assert got == want, (shape.name, lo[0], hi[0], weighted, repeats)


@pytest.mark.parametrize("name", EVERY)
def test_the_wide_lane_arithmetic_on_the_host_for_every_entry_with_0_and_p_minus_1_in_every_position(name):
    """wide_lane_accumulate<D> (pks_verify_asan wide lane) on each entry's own lists and coefficients, their kinds and packing taken
    by wide_terms as wide.hip's launch takes them, weighted and not, against Python ints: random values, and the value bound -- every lo,
    hi and the weight 0 and p - 1 in turn, so that every stepped value wraps both ways"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    shape = W.Shape(name, 1)
    m = shape.m
    rnd = W.random_elements(2 * m + 1, seed=50 + len(name))
    _lane(shape, rnd[:m], rnd[m : 2 * m], True, rnd[2 * m], 3, env)
    _lane(shape, rnd[:m], rnd[m : 2 * m], False, rnd[2 * m], 1, env)
    for lo, hi, w in ((P - 1, 0, P - 1), (0, P - 1, P - 1), (P - 1, P - 1, P - 1), (0, 0, P - 1), (P - 1, 0, 0)):
        _lane(shape, [lo] * m, [hi] * m, True, w, 3, env)
    alternating = [(P - 1, 0)[j % 2] for j in range(m)]  # neighbouring tables at opposite ends
    _lane(shape, alternating, alternating[::-1] if m % 2 == 0 else [P - 1 - v for v in alternating], False, 0, 1, env)


def test_the_wide_lane_arithmetic_with_coefficients_0_and_p_minus_1_at_the_value_bound():
    """x^5, a^2 b^3 and a five-table product at lo, hi in {0, p - 1, p - 2}, coefficient and weight p - 1 and 0"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}

    class Own(W.Shape):
        def __init__(self, m, terms):
            self.name, self.n, self.n_bind, self.m, self.terms, self.has_tau, self.D = "own", 1, 0, m, terms, True, max(len(f) for _, f in terms)

    for coeff in (P - 1, 0):
        for shape in (Own(1, [(coeff, [0] * 5)]), Own(2, [(coeff, [0, 0, 1, 1, 1])]), Own(5, [(coeff, [0, 1, 2, 3, 4])])):
            for lo, hi in ((P - 1, P - 1), (P - 1, 0), (0, P - 1), (P - 2, 5)):
                for w in (P - 1, 0):
                    _lane(shape, [lo] * shape.m, [hi] * shape.m, True, w, 3, env)


def test_hostile_framing_and_counts_of_the_wide_verifier_under_the_sanitizers(cases, tmp_path):
    """pksw_verify alone, built with -fsanitize=address,undefined as a program of its own: proofs cut at every kind of place and grown,
    from exact-size heap blocks; statements whose counts would size buffers or index tables if they were believed"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    for name in ("plonk", "a2b3c"):
        c = cases[name]
        sh = c.shape
        honest = bytes(sh.statement().struct())
        hostile = {"honest": c.proof, "zero length": b"", "one byte": b"\1", "all ones": b"\xff" * len(c.proof), "extended": c.proof + bytes(64),
                   "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes()}
        for cut in (1, 31, 33, 32 * (1 + sh.D), len(c.proof) - 32 * sh.m, len(c.proof) - 1):
            hostile[f"cut at {cut}"] = c.proof[:cut]
        for pattern in (b"", sh.pattern()):
            rest = struct.pack("<II", 1, len(pattern)) + pattern + W.mont(c.tau).tobytes() + W.mont(c.bind).tobytes() + W.mont([c.s]).tobytes()
            rest += struct.pack("<I", len(hostile)) + b"".join(struct.pack("<Q", len(p)) + p for p in hostile.values())
            f = tmp_path / "cases.bin"
            f.write_bytes(honest[:404] + honest[408:] + rest)  # the struct's fields without its padding
            p = subprocess.run([ASAN, "wide", "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            lines = p.stdout.splitlines()
            assert len(lines) == len(hostile)
            for (what, proof), line in zip(hostile.items(), lines):
                rc, accepted, check, offset = line.split()[:4]
                want = W.verify(sh, proof, c.tau, c.bind, c.s)[0]
                assert (rc, check, accepted) == ("0", want, "1" if want == "NONE" else "0"), (what, line)
                assert int(offset) <= len(proof)
    words = list(struct.unpack("<101I", honest[:404]))
    for at, value in ((0, 2**31), (1, 2**32 - 1), (2, 2**30), (3, 7), (4, 2**32 - 1), (5, 2**32 - 1), (5, 0), (6, 6), (21, 2**32 - 1), (22, 16)):
        bad = list(words)
        bad[at] = value
        f = tmp_path / "refused.bin"
        f.write_bytes(struct.pack("<101I", *bad) + honest[408:])  # nothing after the statement: a count that was believed would read past the block
        p = subprocess.run([ASAN, "wide", "verify", str(f)], capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0 and p.stdout.startswith("-1 0 REFUSED"), (at, value, p.stdout, p.stderr[-2000:])
