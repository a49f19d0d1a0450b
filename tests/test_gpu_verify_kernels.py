"""GPU: the three kernels of the verifier's device path (csrc/verify/verify.hip) at their edges and on off-canonical bytes, and the
device path's parity with the host core.  openings_kernel against the definition (leaf fold, path walk by index bits, fold value
sum_j leaf[j] w[j]) for every width / depth / hash version it has a path for and for operands >= p; mat_eval_kernel and
sum_partials_kernel against the bilinear form at the edges of the entry guard, of the 16-proof tile and of the partial-sum loop;
pkv_verify_many against pkv_verify on proofs in which one element v was replaced by v + p.  The references are the C oracle
(tests/oracle_lib.py) for bulk work and Python ints (oracle/pyref.py) on a sample; every comparison is exact."""
import functools
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import oracle_lib as O  # noqa: E402
import pyref as pr  # noqa: E402

P = pr.P
M256 = (1 << 256) - 1


# ---- 1. openings_kernel -----------------------------------------------------------------------------------------------------------
def compress_all(pairs, version):
    """[(l, r)] canonical ints -> digests, by the C oracle"""
    if not pairs:
        return []
    out = O.compress_many(b"".join(l.to_bytes(32, "little") + r.to_bytes(32, "little") for l, r in pairs), version)
    return [int.from_bytes(out[32 * i : 32 * i + 32], "little") for i in range(len(pairs))]


def roots_of(leaves, sibs, paths, idx, version):
    """the definition, top-down from leaves / sibling / path (root -> leaf) / index, on the RESIDUES of what it is given: the hash
    takes any 256-bit value mod p.  Only the low depth + 1 bits of an index are consumed."""
    k, depth = len(leaves), len(paths[0]) if paths else 0
    h = [l[0] % P for l in leaves]
    for j in range(1, len(leaves[0]) if k else 0):
        h = compress_all([(h[q], leaves[q][j] % P) for q in range(k)], version)
    for t in range(depth + 1):
        node = [(sibs[q] if t == 0 else paths[q][depth - t]) % P for q in range(k)]
        h = compress_all([(node[q], h[q]) if (idx[q] >> t) & 1 else (h[q], node[q]) for q in range(k)], version)
    return h


def root_by_python_ints(leaf, sib, path, index, version):
    c = pr.compress if version == 2 else pr.compress_v1
    h = leaf[0] % P
    for x in leaf[1:]:
        h = c(h, x % P)
    for node in [sib] + list(reversed(path)):
        h = c(node % P, h) if index & 1 else c(h, node % P)
        index >>= 1
    return h


def folds_of(leaves, w):
    return [sum((x % P) * wj for x, wj in zip(l, w)) % P for l in leaves]


def limbs(xs, *shape):
    return O.ints_to_limbs(xs).reshape(*shape, 4)


class Openings:
    """one case: Python ints and the arrays pkv_openings_check takes"""

    def __init__(self, leaves, sibs, paths, idx, w, version, roots=None):
        self.k, self.width, self.depth, self.version = len(leaves), len(leaves[0]), len(paths[0]), version
        self.leaves, self.sibs, self.paths, self.idx, self.w = leaves, sibs, paths, idx, w
        self.roots = roots_of(leaves, sibs, paths, idx, version) if roots is None else roots
        self.folds = folds_of(leaves, w)
        k = self.k
        self.a_leaves = limbs([x for l in leaves for x in l], k, self.width)
        self.a_sibs = limbs(sibs, k)
        self.a_paths = limbs([x for p in paths for x in p], k, self.depth)
        self.a_idx = np.array(idx, dtype=np.uint64)
        self.a_roots = limbs(self.roots, k)
        self.a_w = O.to_mont(O.ints_to_limbs(w))  # the kernel's weights are Montgomery, its leaves and folds canonical

    def run(self, ctx, version=None, n=None, **replace):
        from provekit_amd.verify import openings_check

        a = dict(leaves=self.a_leaves, sibs=self.a_sibs, paths=self.a_paths, idx=self.a_idx, roots=self.a_roots)
        a.update(replace)
        n = self.k if n is None else n
        reached, folds = openings_check(ctx, a["leaves"][:n], a["sibs"][:n], a["paths"][:n], a["idx"][:n], a["roots"][:n], weights=self.a_w,
                                        hash_version=version or self.version)
        return reached, O.limbs_to_ints(folds)


def indices_for(depth, k, rng):
    """all-zero, all-one, both alternations, one with bits above bit `depth` (ignored: the path has depth + 1 steps), then random"""
    mask = (1 << (depth + 1)) - 1
    idx = [0, mask, 0xAAAAAAAAAAAAAAAA & mask, 0x5555555555555555 & mask, (rng.randrange(mask + 1) | (1 << (depth + 1)) | (1 << 63))]
    return idx + [rng.randrange(mask + 1) for _ in range(k - len(idx))]


HIGH_BITS = 4  # the opening of indices_for whose index has bits set above bit `depth`


@functools.lru_cache(maxsize=None)
def opening_case(width, depth, version, k=70):
    rng = random.Random(1000 * width + 10 * depth + version)
    f = lambda: rng.randrange(P)  # noqa: E731
    case = Openings([[f() for _ in range(width)] for _ in range(k)], [f() for _ in range(k)], [[f() for _ in range(depth)] for _ in range(k)],
                    indices_for(depth, k, rng), [f() for _ in range(width)], version)
    for q in (0, 1, HIGH_BITS, k - 1):  # the C oracle's chain against Python ints
        assert case.roots[q] == root_by_python_ints(case.leaves[q], case.sibs[q], case.paths[q], case.idx[q], version)
    return case


def flip(arr, where, bit):
    out = arr.copy()
    out[where] ^= np.uint64(1 << bit)
    return out


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("depth", [0, 1, 7, 25])
@pytest.mark.parametrize("width", [1, 2, 16, 32, 64])
def test_openings_reach_their_roots_and_fold_as_defined(ctx, width, depth, version):
    """k = 70: one full 64-lane workgroup and a partial one.  Every opening is reached and folds to sum_j leaf[j] w[j]; under the other
    hash version nothing is reached; one limb of one leaf / sibling / path digest / root altered: exactly that opening fails, and the
    folds change for the altered leaf only."""
    c = opening_case(width, depth, version)
    reached, folds = c.run(ctx)
    assert reached.all(), np.flatnonzero(~reached)
    assert folds == c.folds
    other, folds = c.run(ctx, version=3 - version)
    assert not other.any() and folds == c.folds
    k = c.k

    def only(q, **replace):
        reached, folds = c.run(ctx, **replace)
        assert [int(i) for i in np.flatnonzero(~reached)] == [q], replace.keys()
        return folds

    q, j, limb = 65, width // 2, (width + depth) % 4
    folds = only(q, leaves=flip(c.a_leaves, (q, j, limb), 7))
    altered = list(c.leaves[q])
    altered[j] ^= 1 << (64 * limb + 7)
    assert folds[:q] + folds[q + 1 :] == c.folds[:q] + c.folds[q + 1 :]
    assert folds[q] == folds_of([altered], c.w)[0] != c.folds[q]
    assert only(HIGH_BITS, sibs=flip(c.a_sibs, (HIGH_BITS, 3), 63)) == c.folds
    assert only(k - 1, roots=flip(c.a_roots, (k - 1, 0), 0)) == c.folds
    if depth:
        for q, t in ((63, 0), (64, depth - 1), (1, depth // 2)):  # the digest under the root, the one above the sibling, one between
            assert only(q, paths=flip(c.a_paths, (q, t, (q + t) % 4), 31)) == c.folds


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65])
def test_openings_at_the_workgroup_boundary(ctx, k):
    c = opening_case(16, 7, 2)
    reached, folds = c.run(ctx, n=k)
    assert reached.shape == (k,) and reached.all() and folds == c.folds[:k]
    if k:
        reached, _ = c.run(ctx, n=k, roots=flip(c.a_roots, (k - 1, 2), 5))
        assert [int(i) for i in np.flatnonzero(~reached)] == [k - 1]


def off_canonical_values(rng):
    """multiples of p, powers of two, the end of the 256-bit range and the overflow seam of unpack29<5> (32 x just below 2^261), each
    -2 .. +2 (mod 2^256) -- the operands tests/test_gpu_hash.py::test_compress_structured_inputs aims at the scaled-domain helpers"""
    base = [P, P + 1, 2 * P, 2 * P + 1, 5 * P, 1 << 255, M256, (1 << 256) - P, (1 << 261) // 32 // 5]
    return sorted({(v + d) & M256 for v in base for d in (-2, -1, 0, 1, 2)}) + [rng.randrange(P) + P for _ in range(5)]


PLACES = ("leaf first", "leaf middle", "leaf last", "sibling", "path bottom", "path top")


@functools.lru_cache(maxsize=None)
def off_canonical_case(version, width=16, depth=7):
    """one opening per (value, place): the value stands at that place, everything else is random and canonical.  -> (the case as
    given, the same case on residues); the roots of both are the residues' roots"""
    rng = random.Random(77 + version)
    f = lambda: rng.randrange(P)  # noqa: E731
    vals = off_canonical_values(rng)
    assert sum(v >= P for v in vals) >= 36  # the rest are the canonical neighbours: p - 2, p - 1 and, past 2^256 - 1, 0 and 1
    leaves, sibs, paths = [], [], []
    for v in vals:
        for place in PLACES:
            leaf, sib, path = [f() for _ in range(width)], f(), [f() for _ in range(depth)]
            if place.startswith("leaf"):
                leaf[{"leaf first": 0, "leaf middle": width // 2, "leaf last": width - 1}[place]] = v
            elif place == "sibling":
                sib = v
            else:
                path[depth - 1 if place == "path bottom" else 0] = v  # paths are stored root -> leaf
            leaves.append(leaf)
            sibs.append(sib)
            paths.append(path)
    idx, w = indices_for(depth, len(leaves), rng), [f() for _ in range(width)]
    residues = Openings([[x % P for x in l] for l in leaves], [s % P for s in sibs], [[x % P for x in p] for p in paths], idx, w, version)
    raw = Openings(leaves, sibs, paths, idx, w, version, roots=residues.roots)
    for q in range(0, raw.k, 7):
        assert raw.roots[q] == root_by_python_ints(residues.leaves[q], residues.sibs[q], residues.paths[q], idx[q], version)
    return raw, residues


@pytest.mark.parametrize("version", [1, 2])
def test_openings_take_operands_above_p_as_their_residues(ctx, version):
    """leaf elements, the sibling and path digests >= p: the hash and the fold take them mod p, so the results are those of the
    residues.  The root is compared as bytes (fe_eq(h, root) in the host core): root + p is another root."""
    raw, residues = off_canonical_case(version)
    assert raw.folds == residues.folds  # by construction: folds_of reduces before it multiplies
    want_reached, want_folds = residues.run(ctx)
    assert want_reached.all() and want_folds == residues.folds
    reached, folds = raw.run(ctx)
    assert reached.all(), [(int(q), PLACES[q % len(PLACES)]) for q in np.flatnonzero(~reached)]
    assert folds == residues.folds
    reached, folds = raw.run(ctx, roots=limbs([r + P for r in raw.roots], raw.k))
    assert not reached.any() and folds == residues.folds


# ---- 2. mat_eval_kernel + sum_partials_kernel ---------------------------------------------------------------------------------------
# name -> m, m_0, constraints, witnesses, entries of A, B, C.  A workgroup covers 1024 entries: 0, 1, 1023, 1024, 1025 and 4 * 1024 + 3
# are the edges of its guard; within and across the statements a large matrix is followed by a small one and a small by a large
# (the partial-sum buffer is re-ensured per matrix).  "wide rows" has m_0 > m - 1: the eq(alpha) tables are the longer ones there, in
# the other two the eq(point) tables.  "long" has more than 256 * 1024 entries in A: more than 256 partials, sum_partials_kernel loops.
STATEMENTS = {
    "edges": (12, 9, 500, 2000, (4 * 1024 + 3, 1, 1024)),
    "wide rows": (11, 11, 2000, 1000, (0, 1025, 1023)),
    "long": (13, 10, 1000, 4000, ((1 << 18) + 1500, 1023, 1025)),
}
K_MAX = 33
SPECIAL = (0, 1, P - 1)


def build_matrix(nc, nw, nnz, n_interned, rng):
    rows, cols, vals = (rng.integers(0, hi, size=nnz, dtype=np.int64) for hi in (nc, nw, n_interned))
    corners = [(nc - 1, nw - 1), (0, 0), (0, nw - 1), (nc - 1, 0)][: min(nnz, 4)]
    for e, (r, c) in enumerate(corners):
        rows[e], cols[e], vals[e] = r, c, 3 + e  # a random coefficient: the corner terms are not annihilated by the interner's 0
    if nnz >= 1023:
        vals[10:13] = (0, 1, 2)  # the interner's 0, 1 and p - 1
        rows[100:200], cols[100:200] = rows[200:300], cols[200:300]  # duplicate positions: their terms add up
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    return rows, cols.astype(np.uint32), vals.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def matrix_case(name):
    """the statement, K_MAX (alpha, point) pairs and the C oracle's bilinear forms for them, computed once; the pairs at slots 0, 16
    and 32 are equal; some coordinates are 0, 1 and p - 1.  Two (pair, matrix) values are recomputed on Python ints."""
    from provekit_amd.sparse_matrix import SparseMatrix

    m, m_0, nc, nw, entries = STATEMENTS[name]
    assert nc < 1 << m_0 and nw < 1 << (m - 1)
    rng = np.random.default_rng(len(name))
    pyrng = random.Random(name)
    interner = [0, 1, P - 1] + [pyrng.randrange(P) for _ in range(29)]
    trips = [build_matrix(nc, nw, nnz, len(interner), rng) for nnz in entries]
    for (rows, cols, _), nnz in zip(trips, entries):
        assert len(rows) == nnz
        if nnz >= 4:
            assert {0, nc - 1} <= set(rows.tolist()) and {0, nw - 1} <= set(cols.tolist())
        if nnz >= 1023:
            assert len(set(zip(rows.tolist(), cols.tolist()))) < nnz  # duplicates are present
    sparse = [SparseMatrix(nc, nw, np.searchsorted(r, np.arange(nc)).astype(np.uint32), c, v) for r, c, v in trips]
    interner_mont = O.to_mont(O.ints_to_limbs(interner))
    alphas = [[pyrng.randrange(P) for _ in range(m_0)] for _ in range(K_MAX)]
    points = [[pyrng.randrange(P) for _ in range(m - 1)] for _ in range(K_MAX)]
    for i, s in enumerate(SPECIAL):  # pairs 1..3 and 17..19; pair 0 stays random
        alphas[1 + i][(2 * i) % m_0] = s
        alphas[17 + i][m_0 - 1 - i] = s
        points[1 + i][m - 2 - 3 * i] = s
        points[17 + i][i] = s
    alphas[16], points[16], alphas[32], points[32] = alphas[0], points[0], alphas[0], points[0]
    ev = O.matrix_evaluator(nc, nw, [(s.new_row_indices, s.col_indices, s.values) for s in sparse], interner_mont)
    want = [ev(a, y) for a, y in zip(alphas, points)]
    assert want[0] == want[16] == want[32]
    if 0 in entries:
        assert all(w[entries.index(0)] == 0 for w in want)
    for k, mat in ((2, 0 if entries[0] else 1), (K_MAX - 2, 2)):
        eq_a, eq_y = pr.eq_table(alphas[k]), pr.eq_table(points[k])
        rows, cols, vals = (x.tolist() for x in trips[mat])
        assert want[k][mat] == sum(interner[v] * eq_a[r] * eq_y[c] for r, c, v in zip(rows, cols, vals)) % P, (name, k, mat)
    to_arr = lambda pts, n: O.to_mont(O.ints_to_limbs([x for p in pts for x in p])).reshape(K_MAX, n, 4)  # noqa: E731
    return dict(m=m, m_0=m_0, sparse=sparse, interner=interner_mont, alphas=to_arr(alphas, m_0), points=to_arr(points, m - 1), want=want,
                entries=entries)


@pytest.fixture(scope="module")
def matrix_verifiers(ctx):
    """one attached Verifier per statement, made on first use and kept for the module: its device buffers live across the tests"""
    from provekit_amd.scheme import WhirConfig, blinding_config_for
    from provekit_amd.verify import Verifier

    made = {}

    def get(name):
        if name not in made:
            c = matrix_case(name)
            v = Verifier(c["m"], c["m_0"], WhirConfig.for_size(c["m"], 4.0), blinding_config_for(c["m_0"], 4.0))
            v.set_r1cs(*c["sparse"], c["interner"])
            v.attach(ctx)
            made[name] = v
        return made[name]

    yield get
    for v in made.values():
        v.close()


def evaluations(ver, case, K):
    got = ver.matrix_evaluations(case["alphas"][:K], case["points"][:K])
    assert got.shape == (K, 3, 4)
    ints = O.limbs_to_ints(O.from_mont(got.reshape(-1, 4)))
    return [ints[3 * k : 3 * k + 3] for k in range(K)]


@pytest.mark.parametrize("K", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("name", list(STATEMENTS))
def test_matrix_evaluations_equal_the_bilinear_form(matrix_verifiers, name, K):
    """K around the 16-proof tile: every value equals eq(alpha_k)^T M eq(point_k) of the C oracle; equal pairs in different tiles
    give equal values; an empty matrix evaluates to 0; the first pair alone gives row 0 of every larger call"""
    case, ver = matrix_case(name), matrix_verifiers(name)
    got = evaluations(ver, case, K)
    bad = [(k, mat) for k in range(K) for mat in range(3) if got[k][mat] != case["want"][k][mat]]
    assert not bad, bad
    for k in (16, 32):
        if k < K:
            assert got[k] == got[0]
    if 0 in case["entries"]:
        assert all(g[case["entries"].index(0)] == 0 for g in got)
    assert evaluations(ver, case, 1)[0] == got[0]


@pytest.mark.parametrize("name", list(STATEMENTS))
def test_matrix_evaluations_reuse_their_buffers_across_calls(matrix_verifiers, name):
    """33 pairs, then 1, then 17 on one attached verifier: the device buffers are neither shrunk nor cleared in between"""
    case, ver = matrix_case(name), matrix_verifiers(name)
    for K in (33, 1, 17):
        assert evaluations(ver, case, K) == case["want"][:K], K


# ---- 3. the device path against the host core ----------------------------------------------------------------------------------------
SCALARS = ("root_0", "cubic_message", "final_coefficient")  # absorbed by the sponge: refused unless canonical
HASHED = ("leaf_element", "sibling_digest", "path_digest")  # hint bytes that are only hashed (and folded): taken mod p


def plus_p(proof, off):
    """the 32-byte little-endian element v at `off` replaced by v + p (< 2^256: p < 2^254)"""
    v = int.from_bytes(proof[off : off + 32], "little")
    assert v < P
    return proof[:off] + (v + P).to_bytes(32, "little") + proof[off + 32 :]


@pytest.fixture(scope="module")
def proved(ctx, oracle):
    """the small statement of test_gpu_verify.py (m = 9, m_0 = 7), its verifier and 32 accepted proofs"""
    from test_gpu_verify import small_statement

    scheme, r1cs, d_z, ver, _ = small_statement(ctx, oracle, 9, 7, 100, 60, 3, 6.0)
    proofs = [scheme.prove(d_z, seed=500 + i) for i in range(32)]
    assert len(set(proofs)) == 32
    yield scheme, ver, proofs
    for x in (ver, scheme, r1cs):
        x.close()


def same_as_the_host_core(ver, batch):
    got = ver.verify_many(batch)
    host = [ver.verify(p) for p in batch]
    for i, (g, h) in enumerate(zip(got, host)):
        assert (g.accepted, g.check, g.offset) == (h.accepted, h.check, h.offset), (i, g, h)
    return got


def test_proofs_with_one_element_plus_p_get_the_host_cores_verdict(proved):
    """one proof per region with v replaced by v + p, in a batch of 16 with untouched ones: element for element the host core's
    verdict.  Scalars are refused as NON_CANONICAL on both paths; leaf elements and digests count as their residues."""
    from test_verify_host import walk_layout

    scheme, ver, proofs = proved
    batch, tampered = list(proofs[:16]), {}
    for n, region in enumerate(SCALARS + HASHED):
        i = (5 * n + 1) % 16
        pos = walk_layout(batch[i], scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan)
        batch[i] = plus_p(batch[i], pos[region])
        tampered[i] = region
    assert len(tampered) == 6
    got = same_as_the_host_core(ver, batch)
    for i, g in enumerate(got):
        region = tampered.get(i)
        print(i, region or "-", g)
        if region in SCALARS:
            assert not g.accepted and g.check == "NON_CANONICAL", (i, region, g)
        else:
            assert g.accepted and g.check == "NONE" and g.offset == len(batch[i]), (i, region, g)


def test_verify_many_reuses_its_buffers_across_batches(proved):
    """32 proofs, then 1, then 32 others on one verifier: the flat device arrays are grown once and reused; each time the host core's
    verdicts, and what the short batch left behind disturbs nothing"""
    from test_verify_host import walk_layout

    scheme, ver, proofs = proved
    assert all(r.accepted for r in same_as_the_host_core(ver, proofs))
    assert same_as_the_host_core(ver, proofs[7:8])[0].accepted
    again = list(reversed(proofs))
    pos = walk_layout(again[3], scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan)
    again[3] = plus_p(again[3], pos["leaf_element"])
    t = bytearray(again[20])
    t[walk_layout(again[20], scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan)["sibling_digest"]] ^= 1
    again[20] = bytes(t)
    got = same_as_the_host_core(ver, again)
    assert [i for i, r in enumerate(got) if not r.accepted] == [20] and got[20].check == "MERKLE"
