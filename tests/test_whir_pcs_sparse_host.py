"""CPU: sparse weights (index/value lists) on the host.  The symbols; pkw_verify_sparse on openings
the ORACLE prover builds over the DENSIFIED weights -- same bytes, same sums, fold point and deferred values as pkw_verify_linear
with the dense tables given; every tampering with the verdict it must give; the refusals of offsets, indexes and values that break
the representation's rules; the host's chunked eq tables against Python ints at every chunk boundary; the sums kernel's lane
arithmetic on the host at the column bound; hostile lists and truncated proofs through the sanitizer build (a program of its own,
run as a subprocess)."""
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
SPARSE_HEADER = os.path.join(ROOT, "include", "provekit_whir_sparse.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pkw_verify_asan")

import whir_pcs_cases as K  # noqa: E402
import whir_pcs_linear_cases as L  # noqa: E402
import whir_pcs_sparse_cases as S  # noqa: E402

SPARSE = ["pkw_open_sparse", "pkw_sparse_accumulate", "pkw_sparse_evaluate", "pkw_sparse_sums", "pkw_verify_sparse"]
LINEAR = ["pkw_io_pattern_linear", "pkw_open_linear", "pkw_verify_linear", "pkw_weighted_sums"]
NAMES_BOTH = re.compile(r"weight \d+.*entry \d+", re.S)


def test_the_sparse_header_declares_five_names_the_library_exports_and_the_binding_binds():
    from provekit_amd import whir_pcs

    def declared_in(path):
        return sorted(set(re.findall(r"\b(pkw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))))

    def exported_by(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return sorted(set(re.findall(r" [A-Za-z] (pkw_[a-z0-9_]+)$", nm, flags=re.M)))

    assert declared_in(SPARSE_HEADER) == sorted(SPARSE) and len(SPARSE) == 5
    assert set(SPARSE) <= set(exported_by(whir_pcs.WHIR_LIB_PATH)) and set(SPARSE) <= set(whir_pcs.SIGNATURES)
    # the linear names stay what they were, and provekit_whir.h does not pull the sparse header in
    assert declared_in(os.path.join(ROOT, "include", "provekit_whir_linear.h")) == sorted(LINEAR) and set(LINEAR) <= set(whir_pcs.SIGNATURES)
    assert exported_by(whir_pcs.WHIR_LIB_PATH) == sorted(whir_pcs.SIGNATURES)
    assert "provekit_whir_sparse.h" not in open(os.path.join(ROOT, "include", "provekit_whir.h")).read()
    assert ctypes.CDLL(whir_pcs.WHIR_LIB_PATH).pkw_abi_version() == 1
    assert whir_pcs.CHECKS[-3:] == ("POINTS", "ROOT", "DEFERRED") and whir_pcs.lib.pkw_check_name(len(whir_pcs.CHECKS)) == b"UNKNOWN"


class Case:
    def __init__(self, oracle, n_vars, batch, q, l):
        from provekit_amd import whir_pcs

        self.cfg = K.small_config(n_vars, batch)
        self.n, self.batch, self.q, self.l = n_vars, batch, q, l
        self.polys = K.polynomials(n_vars, batch)
        self.pts = K.points(n_vars, q) if q else []
        self.mpts = K.mont_points(oracle, self.pts) if q else None
        self.ws = S.weights(n_vars, l)
        self.dense = [S.densify(n_vars, w) for w in self.ws]
        self.mdense = [L.mont(oracle, w) for w in self.dense]
        self.tags = L.tags(l)
        self.mtags = L.mont(oracle, self.tags)
        self.pattern = whir_pcs.io_pattern_linear(self.cfg, q, l)
        self.proof, self.root, self.vals, self.sums = L.oracle_linear_opening(oracle, self.cfg, self.polys, self.pts, self.dense, self.tags, self.pattern)
        self.tag_offset = 32 + 32 * self.cfg.commitment_ood_samples * batch + 32 * q * n_vars
        self.sum_offset = self.tag_offset + 32 * l + 32 * q * batch
        self.oracle = oracle

    def verify(self, proof=None, ws=None, tags=None, **kw):
        from provekit_amd import whir_pcs

        kw.setdefault("expected_root", self.root)
        return whir_pcs.verify_sparse(self.cfg, self.mpts, self.mtags if tags is None else tags, S.pack(self.oracle, self.ws if ws is None else ws),
                                      self.proof if proof is None else proof, **kw)


@pytest.fixture(scope="module")
def cases(oracle):
    return {s: Case(oracle, *s) for s in L.SHAPES}


@pytest.mark.parametrize("shape", L.SHAPES)
def test_oracle_built_openings_over_the_densified_weights_are_accepted(oracle, cases, shape):
    from provekit_amd import whir_pcs

    c = cases[shape]
    assert c.sums == S.sums(c.polys, c.ws) == L.expected_sums(c.polys, c.dense)  # the lists and the tables state the same sums
    if c.l == 16:  # the widest set holds every kind of weight
        nnz = [len(idx) for idx, _ in c.ws]
        assert nnz[1] == 0 and c.ws[2][0] == [0] and c.ws[3][0] == [(1 << c.n) - 1] and nnz[4] == 1 << c.n and c.ws[5][0] == c.ws[0][0]
        assert c.ws[0][1][:3] == [0, 1, K.P - 1]
    dense = whir_pcs.verify_linear(c.cfg, c.mpts, c.mtags, c.mdense, c.proof, expected_root=c.root)
    assert dense.result.accepted and dense.unchecked == 0
    for kw in ({}, {"io_pattern": c.pattern}, {"expected_root": None}):
        v = c.verify(**kw)
        assert v.result.accepted and v.result.check == "NONE" and v.result.offset == len(c.proof), v.result
        assert oracle.limbs_to_ints(oracle.from_mont(v.sums.reshape(-1, 4))) == [s for row in c.sums for s in row]
        for got, want in ((v.sums, dense.sums), (v.evals, dense.evals), (v.fold_point, dense.fold_point), (v.deferred, dense.deferred)):
            assert np.array_equal(got, want)
    fold = oracle.limbs_to_ints(oracle.from_mont(v.fold_point))
    assert oracle.limbs_to_ints(oracle.from_mont(v.deferred)) == S.evaluate(c.n, c.ws, fold)


def test_every_tampering_is_rejected_with_its_check_and_the_deferred_check_names_the_weight(oracle, cases):
    c = cases[(8, 2, 2, 3)]
    assert c.verify().result.accepted

    def flipped(off):
        t = bytearray(c.proof)
        t[off] ^= 1
        return bytes(t)

    other_value = [(list(i), list(v)) for i, v in c.ws]
    other_value[2][1][0] = (other_value[2][1][0] + 1) % K.P
    other_index = [(list(i), list(v)) for i, v in c.ws]
    idx = other_index[0][0]
    k = next(k for k in range(3, len(idx) - 1) if idx[k] + 1 < idx[k + 1])  # past the planted values: entry 0's is 0, and may sit anywhere
    idx[k] += 1  # still strictly increasing, still in range: a well-formed list of another weight
    other_tags = c.mtags.copy()
    other_tags[c.l - 1] = L.mont(oracle, [424242])[0]
    expect = {
        "one value changed in the call": (dict(ws=other_value), "DEFERRED", "weight 2"),
        "one index changed in the call": (dict(ws=other_index), "DEFERRED", "weight 0"),
        "one tag changed in the call": (dict(tags=other_tags), "POINTS", f"tag {c.l - 1}"),
        "one tag changed in the proof": (dict(proof=flipped(c.tag_offset + 32 * (c.l - 1))), "POINTS", "tag"),
        "one sum changed in the proof": (dict(proof=flipped(c.sum_offset + 32 * (c.l * c.batch - 1))), "WHIR_SUMCHECK", ""),
        "truncated by 1 byte": (dict(proof=c.proof[:-1]), "TRANSCRIPT_SHORT", ""),
        "one appended byte": (dict(proof=c.proof + b"\0"), "TRAILING_BYTES", ""),
    }
    for name, (kw, check, says) in expect.items():
        v = c.verify(**kw)
        print(f"{name}: {v.result}")
        assert not v.result.accepted and v.result.check == check and says in v.result.message, (name, v.result)


def test_a_proof_run_over_other_weights_than_the_lists_stand_for_fails_the_deferred_check(oracle):
    """WHIR run honestly over ANOTHER table, with that table's true sums claimed: every WHIR relation holds; only the verifier's
    own evaluation of its entries at the folding point can tell, and with lists it always makes it"""
    from provekit_amd import whir_pcs

    n, batch, q, l = 8, 1, 0, 1
    cfg = K.small_config(n, batch)
    polys = K.polynomials(n, batch)
    mine, other = S.weights(n, 1), S.weights(n, 1, seed=99)
    d_mine, d_other = [S.densify(n, w) for w in mine], [S.densify(n, w) for w in other]
    tg = L.tags(l)
    proof, root, _, _ = L.oracle_linear_opening(oracle, cfg, polys, [], d_mine, tg, whir_pcs.io_pattern_linear(cfg, q, l), prove_weights=d_other,
                                                claimed_sums=L.expected_sums(polys, d_other))
    v = whir_pcs.verify_sparse(cfg, None, L.mont(oracle, tg), S.pack(oracle, mine), proof, expected_root=root)
    assert not v.result.accepted and v.result.check == "DEFERRED" and "weight 0" in v.result.message, v.result
    assert whir_pcs.verify_sparse(cfg, None, L.mont(oracle, tg), S.pack(oracle, other), proof, expected_root=root).result.accepted


def test_lists_that_break_the_rules_are_refused_with_a_reason_naming_weight_and_entry(oracle, cases):
    from provekit_amd import whir_pcs
    from provekit_amd._lib import ProveKitHipError

    c = cases[(8, 2, 2, 3)]
    good = S.pack(oracle, c.ws)
    nnz0 = len(c.ws[0][0])
    assert nnz0 >= 4

    def variant(offsets=None, index=None, value=None):
        return whir_pcs.SparseWeights(offsets=good.offsets.copy() if offsets is None else offsets, index=good.index.copy() if index is None else index,
                                      value=good.value.copy() if value is None else value)

    def with_index(k, x):
        idx = good.index.copy()
        idx[k] = x
        return variant(index=idx)

    shifted = good.offsets.copy()
    shifted[0] = 1
    decreasing = good.offsets.copy()
    decreasing[1], decreasing[2] = decreasing[2] + 1, decreasing[1]  # weight 0 grows by one, weight 1 ends before it starts
    too_long = np.array([0, 257, 257, 257], dtype=np.uint64)
    val_p = good.value.copy()
    val_p[2] = np.frombuffer(K.P.to_bytes(32, "little"), dtype="<u8")
    bad = {
        "offsets[0] = 1": (variant(offsets=shifted), "offsets[0]"),
        "decreasing offsets": (variant(offsets=decreasing), "weight 1"),
        "a weight longer than 2^n": (variant(offsets=too_long, index=np.zeros(257, dtype=np.uint32), value=np.zeros((257, 4), dtype=np.uint64)), "weight 0"),
        "an equal index pair": (with_index(2, int(good.index[1])), "weight 0, entry 2"),
        "a decreasing index pair": (with_index(3, int(good.index[2]) - 1), "weight 0, entry 3"),
        "an index = 2^n": (with_index(nnz0 - 1, 1 << c.n), f"weight 0, entry {nnz0 - 1}"),
        "an index = 2^n in the last weight": (with_index(len(good.index) - 1, 1 << c.n), "weight 2, entry 0"),
        "a value = p": (variant(value=val_p), "weight 0, entry 2"),
    }
    for name, (w, says) in bad.items():
        with pytest.raises(ProveKitHipError) as e:
            whir_pcs.verify_sparse(c.cfg, c.mpts, c.mtags, w, c.proof, expected_root=c.root)
        print(f"{name}: {e.value}")
        assert e.value.code == -1 and says in str(e.value) and NAMES_BOTH.search(str(e.value)), (name, str(e.value))
    assert c.verify().result.accepted  # the thread's error slot does not stick
    # the counts are pkw_verify_linear's
    for tags, why in ((np.zeros((0, 4), dtype=np.uint64), "1..16"), (np.zeros((17, 4), dtype=np.uint64), "1..16")):
        with pytest.raises(ProveKitHipError, match=why):
            whir_pcs.verify_sparse(c.cfg, c.mpts, tags, whir_pcs.SparseWeights(offsets=np.zeros(len(tags) + 1, dtype=np.uint64), index=[], value=[]), c.proof)


def chunk_edges():
    import pk_probes

    b = pk_probes.lib.pk_probe_whir_sparse_chunk_bits()
    assert b == 8  # the sizes below straddle its multiples
    return sorted({0, 1, 30} | {m * b + d for m in (1, 2, 3) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 30])
def test_the_hosts_chunked_eq_tables_agree_with_python_ints(oracle, n):
    """sparse.hpp's SparseEqTables, the code pkw_verify_sparse judges the deferred values with: n_vars 0, 1, every chunk boundary
    and its neighbours, 30; random points and points with coordinates 0, 1 and -1; entries at 0, 2^n - 1 and on both sides of every
    chunk boundary bit"""
    import pk_probes

    assert n in chunk_edges()
    N = 1 << n
    idx = {0, N - 1} | {x for b in range(0, n + 1, 8) for x in ((1 << b) - 1, 1 << b, (1 << b) + 1) if 0 <= x < N}
    idx |= {int(x) for x in np.random.default_rng(n).integers(0, N, size=20)}
    idx = sorted(idx)
    val = K.random_ints(len(idx), 70 + n)
    val[0], val[-1] = K.P - 1, 1
    rnd = K.random_ints(max(n, 1), 80 + n)[:n]
    corner = [(0, 1, K.P - 1)[j % 3] for j in range(n)]
    mixed = [corner[j] if j % 2 else rnd[j] for j in range(n)]
    index = np.array(idx, dtype=np.uint32)
    mval = L.mont(oracle, val)
    for point in (rnd, corner, mixed):
        mpt = L.mont(oracle, point) if n else np.zeros((1, 4), dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        assert pk_probes.lib.pk_probe_sparse_eq_host(n, mpt.ctypes.data, index.ctypes.data, mval.ctypes.data, len(idx), out.ctypes.data) == 0
        assert oracle.limbs_to_ints(oracle.from_mont(out.reshape(1, 4))) == S.evaluate(n, [(idx, val)], point)
    # a 0/1 point makes eq an indicator: the weight's value at that position, or nothing
    for at in (idx[0], idx[-1], idx[len(idx) // 2]):
        point = [(at >> (n - 1 - j)) & 1 for j in range(n)]
        mpt = L.mont(oracle, point) if n else np.zeros((1, 4), dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        assert pk_probes.lib.pk_probe_sparse_eq_host(n, mpt.ctypes.data, index.ctypes.data, mval.ctypes.data, len(idx), out.ctypes.data) == 0
        assert oracle.limbs_to_ints(oracle.from_mont(out.reshape(1, 4))) == [val[idx.index(at)]]
    out = np.zeros(4, dtype=np.uint64)
    bad = np.array([N if n < 32 else 0], dtype=np.uint32)
    assert pk_probes.lib.pk_probe_sparse_eq_host(n, mpt.ctypes.data, bad.ctypes.data, mval.ctypes.data, 1, out.ctypes.data) == -1


@pytest.mark.parametrize("top", [K.P - 1, (1 << 256) - 1], ids=["p-1", "2^256-1"])
@pytest.mark.parametrize("terms", range(1, 10))
def test_the_sums_kernels_lane_on_the_host_at_the_column_bound(terms, top):
    """the sums kernel's accumulate / flush / result code (sparse.hpp's sparse_tile_step over linear_tile.hpp's tile, 4 polynomials
    x 1 value as two slices of 2 x 1, which is how sparse.hip instantiates it), compiled for the host, for 1 to 9 entries: every phase of a DOT29_GROUP = 4
    reduction group.  Every value is p - 1; the gathered elements are p - 1 -- the largest reduced element: the columns at their
    bound -- or 2^256 - 1, every limb at its maximum, which the step reduces first (eight in a row are beyond what dot29's running
    sum takes unreduced)"""
    import pk_probes

    R_INV = pow(1 << 256, -1, K.P)
    f = np.frombuffer(top.to_bytes(32, "little") * (4 * terms), dtype="<u8").copy()
    w = np.frombuffer((K.P - 1).to_bytes(32, "little") * terms, dtype="<u8").copy()
    out = np.zeros(16, dtype=np.uint64)
    assert pk_probes.lib.pk_probe_sparse_tile_host(f.ctypes.data, w.ctypes.data, terms, out.ctypes.data) == 0
    got = [int.from_bytes(out[4 * i : 4 * i + 4].tobytes(), "little") for i in range(4)]
    assert got == [terms * top * (K.P - 1) * R_INV % K.P] * 4


def test_the_sums_kernels_lane_on_the_host_with_distinct_operands():
    import pk_probes

    terms, R_INV = 7, pow(1 << 256, -1, K.P)
    f = [K.random_ints(terms, 50 + u) for u in range(4)]
    w = K.random_ints(terms, 60)
    w[0], w[1], w[2] = 0, 1, K.P - 1
    f[0][2], f[3][6] = (1 << 256) - 1, K.P  # a gathered element may be any 256-bit value
    pack = lambda rows: np.frombuffer(b"".join(x.to_bytes(32, "little") for r in rows for x in r), dtype="<u8").copy()  # noqa: E731
    out = np.zeros(16, dtype=np.uint64)
    assert pk_probes.lib.pk_probe_sparse_tile_host(pack(f).ctypes.data, pack([w]).ctypes.data, terms, out.ctypes.data) == 0
    got = [int.from_bytes(out[4 * i : 4 * i + 4].tobytes(), "little") for i in range(4)]
    assert got == [sum(a * b for a, b in zip(f[u], w)) * R_INV % K.P for u in range(4)]


def test_hostile_lists_and_truncated_proofs_under_the_sanitizers(oracle, cases, tmp_path):
    """pkw_verify_sparse alone, built with -fsanitize=address,undefined as a program of its own (make -C provekit_amd/csrc asan):
    index, value and proof live in exact-size heap blocks there, so a read past any of them is a report, not a wrong answer"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pkw_verify_asan is missing: make -C provekit_amd/csrc asan"
    from provekit_amd import whir_pcs

    c = cases[(8, 2, 2, 3)]
    good = S.pack(oracle, c.ws)
    d0 = L.deferred_offset(c.proof, c.q + c.l)
    proofs = {"honest": c.proof, "zero length": b"", "truncated inside the sums": c.proof[: c.sum_offset + 40], "truncated inside the tags": c.proof[: c.tag_offset + 7],
              "truncated inside the deferred hint": c.proof[: d0 + 33], "truncated by 1 byte": c.proof[:-1],
              "random bytes": np.random.default_rng(1).integers(0, 256, size=len(c.proof), dtype=np.uint8).tobytes()}
    t = bytearray(c.proof)
    struct.pack_into("<Q", t, d0 - 8, 1 << 63)
    proofs["deferred count = 2^63"] = bytes(t)

    def lists(offsets=None, index=None, value=None):
        return (good.offsets if offsets is None else np.asarray(offsets, dtype=np.uint64), good.index if index is None else np.asarray(index, dtype=np.uint32),
                good.value if value is None else value)

    def idx_with(k, x):
        i = good.index.copy()
        i[k] = x
        return i

    total = len(good.index)
    hostile = {
        "honest": lists(),
        "offsets[0] = 2^63": lists(offsets=[1 << 63] + list(good.offsets[1:])),
        "offsets decrease to 0": lists(offsets=[0, total, 0, 0]),
        "a weight of 2^64 - 1 entries": lists(offsets=[0, (1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1]),
        "a weight of 2^n + 1 entries": lists(offsets=[0, 257, 257, 257], index=np.arange(257), value=np.zeros((257, 4), dtype=np.uint64)),
        "index = 2^n": lists(index=idx_with(total - 1, 1 << c.n)),
        "index = 2^32 - 1": lists(index=idx_with(0, 0xFFFFFFFF)),
        "equal pair": lists(index=idx_with(1, int(good.index[0]))),
        "value = 2^256 - 1": lists(value=np.concatenate([good.value[:-1], np.full((1, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)])),
        "every weight empty, no lists": lists(offsets=[0, 0, 0, 0], index=np.zeros(0), value=np.zeros((0, 4), dtype=np.uint64)),
    }
    cs = whir_pcs._cfg_struct(c.cfg)
    blob = struct.pack("<4I", 2, c.q, c.l, 0) + bytes(cs) + struct.pack("<I", len(c.pattern)) + c.pattern + c.mpts.tobytes() + c.mtags.tobytes()
    blob += struct.pack("<I", len(proofs)) + b"".join(struct.pack("<Q", len(p)) + p for p in proofs.values())
    blob += struct.pack("<I", len(hostile))
    for off, idx, val in hostile.values():
        blob += off.tobytes() + struct.pack("<Q", len(idx)) + idx.tobytes() + struct.pack("<Q", len(val)) + np.ascontiguousarray(val, dtype=np.uint64).tobytes()
    f = tmp_path / "cases.bin"
    f.write_bytes(blob)
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    p = subprocess.run([ASAN, "sparse", str(f)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(proofs) + len(hostile) - 1
    structural = {"TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT"}
    for (name, proof), line in zip(proofs.items(), lines):
        rc, accepted, check, offset = line.split()[:4]
        if name == "honest":
            assert (rc, accepted, check, int(offset)) == ("0", "1", "NONE", len(proof)), line
        else:
            assert rc == "0" and accepted == "0" and check in structural, (name, line)
        v = c.verify(proof=proof, expected_root=None)  # the library loaded into this process gives the same verdict
        assert (str(int(v.result.accepted)), v.result.check, v.result.offset) == (accepted, check, int(offset)), (name, line, v.result)
    for name, line in zip(list(hostile)[1:], lines[len(proofs) :]):
        if name == "every weight empty, no lists":  # well-formed: the zero weights, which this proof was not made for
            assert line.split()[:3] == ["0", "0", "DEFERRED"], (name, line)
        else:
            assert line.startswith("-1 0 REFUSED") and ("weight" in line or "offsets" in line), (name, line)
