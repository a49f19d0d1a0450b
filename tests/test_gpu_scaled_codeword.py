"""GPU: the hash-ready codeword (PK_LEAVES_SCALED32, csrc/skyscraper29s.hpp "the hash-ready codeword") in front of every consumer on
the device, over the whole range the encoding allows -- the stored values of tests/scaled_codeword_cases.py, every edge at a fold's
seed, at a later element and in an opened row -- and the producer held to its bound.  With it the index edges of the opening kernel
and the Montgomery-form leaf hash at the same sizes.  Everything is bit-exact against Python integers and the oracle's hash.
tests/test_scaled_codeword_host.py is the CPU half (the host build of the same source)."""
import ctypes as C

import numpy as np
import pytest

import scaled_codeword_cases as sc

pytestmark = pytest.mark.gpu

P = sc.P


def sentinel(n):
    return np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)


def ref_paths(heap, n, idx):
    """authentication paths of the leaves idx in the heap (2n digests), root -> leaf, without the leaf's sibling"""
    logn = n.bit_length() - 1
    plen = max(logn - 1, 0)
    out = np.zeros((len(idx), plen, 4), dtype=np.uint64)
    for q, i in enumerate(idx):
        for d in range(plen):
            out[q, d] = heap[((n + int(i)) >> (logn - (d + 1))) ^ 1]
    return out


def ref_siblings(heap, n, idx):
    return heap[(n + np.asarray(idx, dtype=np.int64)) ^ 1]


# ---- the self-test ops 39 .. 43 on the device --------------------------------------------------------------------------------------
def host_and_device(ctx, op, xs, ys):
    from provekit_amd._lib import lib
    from tools.pk_probes import lib as probes

    a, b = sc.to_limbs(xs), sc.to_limbs(ys)
    n = a.shape[0]
    host = np.empty_like(a)
    assert lib.pk_selftest_arith(op, a.ctypes.data, b.ctypes.data, host.ctypes.data, n) == 0
    da, db, do = ctx.upload(a), ctx.upload(b), ctx.alloc_fe(n)
    ctx._check(probes.pk_probe_arith_device(ctx.handle, op, da.ptr, db.ptr, do.ptr, n))
    return sc.from_limbs(host), sc.from_limbs(ctx.download_fe(do, n))


@pytest.mark.parametrize("op", [39, 40, 41, 42, 43])
def test_consumer_ops_device_host_and_ints_agree(ctx, oracle, op):
    import test_scaled_codeword_host as H

    if op in (42, 43):
        xs = ys = list(sc.CASES)
        want = [(sc.canonical_opening if op == 42 else sc.montgomery_opening)(x) for x in xs]
    else:
        xs, ys = sc.pair_operands()
        want = (H.fold_of_three(oracle, xs, ys) if op == 41 else
                sc.compress(oracle, [sc.value(x) for x in xs], [sc.value(y) for y in ys], 2 if op == 39 else 1))
    host, dev = host_and_device(ctx, op, xs, ys)
    assert H.mismatches(dev, want, xs, ys) == [], "the device build differs from the definition"
    assert H.mismatches(host, want, xs, ys) == [], "the host build differs from the definition"
    assert dev == host


# ---- (a) the leaf hash of constructed hash-ready leaves -----------------------------------------------------------------------------
@pytest.mark.parametrize("width", sc.LEAF_WIDTHS)
@pytest.mark.parametrize("version", [2, 1])
def test_leaf_hash_of_constructed_hash_ready_leaves(ctx, oracle, version, width):
    """leaf_hash_kernel<version, PK_COL_MAJOR, SCALED_IN> through the lab's pk_probe_leaf_hash_scaled: the last lane of a workgroup,
    one lane of a second and a third (63 .. 513 leaves), every edge value as some leaf's seed and as some leaf's later element
    (tests/test_scaled_codeword_host.py asserts that of the matrices), every digest, nothing written behind the digests"""
    from tools.pk_probes import lib as probes

    rows = sc.leaf_matrix(max(sc.LEAF_COUNTS), width, salt=width)
    want = sc.to_limbs(sc.leaf_digests(oracle, rows, version))
    ctx.set_hash_version(version)
    try:
        for n in sc.LEAF_COUNTS:
            d_l, d_out = ctx.upload(sc.column_major(rows[:n])), ctx.upload(sentinel(n + 1))
            ctx._check(probes.pk_probe_leaf_hash_scaled(ctx.handle, d_l.ptr, n, width, d_out.ptr))
            got = ctx.download_fe(d_out, n + 1)
            assert np.array_equal(got[:n], want[:n]), (n, [i for i in range(n) if not np.array_equal(got[i], want[i])][:4])
            assert np.array_equal(got[n], sentinel(1)[0]), n
    finally:
        ctx.set_hash_version(2)


# ---- (b) openings of constructed buffers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 3, 32])
@pytest.mark.parametrize("n", [2, 256])
def test_openings_of_constructed_hash_ready_buffers(ctx, oracle, n, width):
    """pk_gather_leaves_enc (both layouts) and pk_commit_open over a buffer the test built in PK_LEAVES_SCALED32, every leaf opened
    (at 256 leaves every column holds every edge value), canonical and Montgomery; the heap under pk_commit_open is the lab's digests
    of that buffer and pk_merkle_inner above them: every node equals the reference tree's"""
    from provekit_amd._lib import LEAVES_SCALED32, PK_COL_MAJOR, PK_LEAF_MAJOR, CommitLayout, lib
    from tools.pk_probes import lib as probes

    rows = sc.leaf_matrix(n, width, salt=3 * width)
    if n == 256:
        assert all(set(sc.EDGES) <= {row[j] for row in rows} for j in range(width))
    want = {1: sc.to_limbs(sc.canonical_opening(x) for row in rows for x in row).reshape(n, width, 4),
            0: sc.to_limbs(sc.montgomery_opening(x) for row in rows for x in row).reshape(n, width, 4)}
    heap = oracle.merkle_inner(sc.to_limbs(sc.leaf_digests(oracle, rows, 2)))
    d_col, d_row = ctx.upload(sc.column_major(rows)), ctx.upload(sc.leaf_major(rows))
    d_nodes = ctx.upload(sentinel(2 * n))
    ctx._check(probes.pk_probe_leaf_hash_scaled(ctx.handle, d_col.ptr, n, width, d_nodes.view_fe(n)))
    ctx._check(lib.pk_merkle_inner(ctx.handle, d_nodes.ptr, n))
    assert np.array_equal(ctx.download_fe(d_nodes.view_fe(1), 2 * n - 1), heap[1:])  # root, inner nodes and leaf digests
    idx = np.arange(n, dtype=np.uint64)[::-1].copy()  # every leaf, last first
    plen = max(n.bit_length() - 2, 0)
    lay = CommitLayout()
    lay.n_shards, lay.shard, lay.encoding = 1, 0, LEAVES_SCALED32
    for canon in (1, 0):
        for layout, buf in ((PK_COL_MAJOR, d_col), (PK_LEAF_MAJOR, d_row)):
            got = np.zeros((n, width, 4), dtype=np.uint64)
            ctx._check(lib.pk_gather_leaves_enc(ctx.handle, buf.ptr, n, width, layout, LEAVES_SCALED32, idx.ctypes.data, n, canon, got.ctypes.data))
            assert np.array_equal(got, want[canon][::-1]), (canon, layout)
        lo, so, po = np.zeros((n, width, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64), np.zeros((n, max(plen, 1), 4), dtype=np.uint64)
        ctx._check(lib.pk_commit_open(ctx.handle, d_col.ptr, d_nodes.ptr, n, width, C.byref(lay), idx.ctypes.data, n, canon, lo.ctypes.data,
                                      so.ctypes.data, po.ctypes.data))
        assert np.array_equal(lo, want[canon][::-1]), canon
        assert np.array_equal(so, ref_siblings(heap, n, idx))
        assert np.array_equal(po[:, :plen], ref_paths(heap, n, idx))


# ---- (c) the producer keeps the contract --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,n_vars,fold", [pytest.param(3, 10, 0, id="b3-rows2^11"), pytest.param(1, 18, 0, id="b1-rows2^19")])
def test_the_commit_stores_what_the_encoding_promises(ctx, oracle, batch, n_vars, fold):
    """pk_commit_into at 2^11 rows (two passes, both in the register-radix kernel) and at 2^19 rows (three: two register-radix passes
    before the last -- the smallest size with three passes), rate 1/2: every stored element is at most p + (p >> 10) (the producer
    bound: what reduce_almost29 leaves) and decodes, x / 32 mod p, to the oracle's codeword.
    Measured on an MI355X: 3 of the 6144 elements at 2^11 rows and 256 of the 524288 at 2^19 rows are stored at or above p, the
    largest of them 0.6 of p >> 10 above it (a count, printed on every run, not a bound: nothing is asserted of it)."""
    from provekit_amd._lib import LEAVES_SCALED32, CommitLayout, lib
    from provekit_amd.field import random_field

    polys = [random_field(1 << n_vars, 1900 + b + n_vars) for b in range(batch)]
    bufs = [ctx.upload(p) for p in polys]
    code = oracle.rs_encode(np.concatenate(polys), batch, n_vars, 1, fold)  # (rows, width) Montgomery images
    n, w = code.shape[0], code.shape[1]
    szs = [C.c_size_t() for _ in range(3)]
    ctx._check(lib.pk_commit_sizes(ctx.handle, batch, n_vars, 1, fold, *[C.byref(x) for x in szs]))
    assert szs[0].value == n * w
    d_l, d_n, d_s = (ctx.alloc_fe(x.value) for x in szs)
    ptrs = (C.c_void_p * batch)(*[b.ptr for b in bufs])
    root, lay = (C.c_uint8 * 32)(), CommitLayout()
    ctx._check(lib.pk_commit_into(ctx.handle, ptrs, batch, n_vars, 1, fold, d_l.ptr, d_n.ptr, d_s.ptr, root, C.byref(lay)))
    assert (lay.n_shards, lay.shard, lay.encoding) == (1, 0, LEAVES_SCALED32)
    stored = sc.from_limbs(ctx.download_fe(d_l, n * w))  # column-major
    values = sc.from_limbs(oracle.from_mont(np.ascontiguousarray(code.transpose(1, 0, 2))))
    above = sum(x >= P for x in stored)
    print(f"hash-ready codeword of {w} x 2^{n.bit_length() - 1}: {above} of {n * w} elements stored at or above p, largest excess "
          f"{max(stored) - P if above else 0:#x} (p >> 10 = {P >> 10:#x})")
    assert max(stored) <= sc.PRODUCER_MAX
    bad = [(t % n, t // n, hex(x)) for t, (x, v) in enumerate(zip(stored, values)) if sc.value(x) != v]
    assert bad[:4] == []


# ---- (d) the index edges of the opening kernel, in either encoding --------------------------------------------------------------------
OPEN_N, OPEN_W = 1 << 10, 3
# k * width and k * (width + log2 n) one below, at and one above a multiple of 256 (the opening kernel's workgroup): 3 k = 255, 768, 513
# and 13 k = 767, 3328, 2561
OPEN_KS = (1, 59, 85, 171, 197, 256)


@pytest.fixture(scope="module")
def open_trees(ctx, oracle):
    """three trees of 2^10 leaves of width 3 with their reference heaps and rows: a constructed hash-ready buffer (column-major, opened
    with pk_commit_open) and Montgomery leaves in both layouts (pk_tree_from_leaves, opened with pk_tree_open)"""
    from provekit_amd._lib import LEAVES_SCALED32, PK_COL_MAJOR, PK_LEAF_MAJOR, CommitLayout, lib
    from provekit_amd.field import random_field
    from tools.pk_probes import lib as probes

    n, w = OPEN_N, OPEN_W
    assert [k * w % 256 for k in (85, 256, 171)] == [255, 0, 1] and [k * (w + 10) % 256 for k in (59, 256, 197)] == [255, 0, 1]
    trees, keep = [], []
    rows = sc.leaf_matrix(n, w, salt=5)
    heap = oracle.merkle_inner(sc.to_limbs(sc.leaf_digests(oracle, rows, 2)))
    d_col, d_nodes = ctx.upload(sc.column_major(rows)), ctx.alloc_fe(2 * n)
    ctx._check(probes.pk_probe_leaf_hash_scaled(ctx.handle, d_col.ptr, n, w, d_nodes.view_fe(n)))
    ctx._check(lib.pk_merkle_inner(ctx.handle, d_nodes.ptr, n))
    lay = CommitLayout()
    lay.n_shards, lay.shard, lay.encoding = 1, 0, LEAVES_SCALED32
    keep += [d_col, d_nodes, lay]

    def open_raw(idx, k, canon, lo, so, po):
        return lib.pk_commit_open(ctx.handle, d_col.ptr, d_nodes.ptr, n, w, C.byref(lay), idx, k, canon, lo, so, po)

    trees.append(("hash-ready", open_raw, heap,
                  {1: sc.to_limbs(sc.canonical_opening(x) for row in rows for x in row).reshape(n, w, 4),
                   0: sc.to_limbs(sc.montgomery_opening(x) for row in rows for x in row).reshape(n, w, 4)}))
    leaves = random_field(n * w, 77).reshape(n, w, 4)
    leaves[0, 0], leaves[n - 1, w - 1] = 0, sc.to_limbs([P - 1])[0]
    mheap = oracle.merkle_commit(leaves)
    mrows = {1: oracle.from_mont(leaves).reshape(n, w, 4), 0: leaves}
    handles = []
    for name, layout, arr in (("montgomery-col", PK_COL_MAJOR, leaves.transpose(1, 0, 2)), ("montgomery-leaf", PK_LEAF_MAJOR, leaves)):
        d = ctx.upload(arr)
        h, root = C.c_void_p(), (C.c_uint8 * 32)()
        ctx._check(lib.pk_tree_from_leaves(ctx.handle, d.ptr, n, w, layout, root, C.byref(h)))
        assert bytes(root) == mheap[1].tobytes()
        keep.append(d)
        handles.append(h)
        trees.append((name, (lambda hh: lambda idx, k, canon, lo, so, po: lib.pk_tree_open(ctx.handle, hh, idx, k, canon, lo, so, po))(h), mheap, mrows))
    yield {t[0]: t[1:] for t in trees}
    for h in handles:
        lib.pk_tree_destroy(ctx.handle, h)


def open_at(ctx, opener, idx, canon):
    k, plen = len(idx), OPEN_N.bit_length() - 2
    lo, so, po = np.zeros((k, OPEN_W, 4), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64), np.zeros((k, plen, 4), dtype=np.uint64)
    ctx._check(opener(idx.ctypes.data, k, canon, lo.ctypes.data, so.ctypes.data, po.ctypes.data))
    return lo, so, po


@pytest.mark.parametrize("k", OPEN_KS)
@pytest.mark.parametrize("tree", ["hash-ready", "montgomery-col", "montgomery-leaf"])
def test_opening_index_edges(ctx, open_trees, tree, k):
    """unsorted indices with duplicates: every position holds its own leaf's row, sibling and path -- what the reference tree holds
    and, bit for bit, what an opening at the sorted unique indices returns for that leaf; k at the edges of the kernel's two lane
    ranges (rows, then digests)"""
    opener, heap, rows = open_trees[tree]
    n = OPEN_N
    idx = np.random.default_rng(1000 + k).integers(0, n, size=k).astype(np.uint64)
    if k >= 4:
        idx[1], idx[2], idx[3], idx[k // 2], idx[k - 1] = n - 1, 0, idx[0], n - 1, idx[0]  # the ends, and duplicates far apart
        assert len(np.unique(idx)) < k and list(idx) != sorted(idx)
    uniq = np.unique(idx)
    where = np.searchsorted(uniq, idx)
    for canon in (1, 0):
        lo, so, po = open_at(ctx, opener, idx, canon)
        ii = idx.astype(np.int64)
        assert np.array_equal(lo, rows[canon][ii]), canon
        assert np.array_equal(so, ref_siblings(heap, n, idx)) and np.array_equal(po, ref_paths(heap, n, idx))
        ulo, uso, upo = open_at(ctx, opener, uniq, canon)
        assert np.array_equal(lo, ulo[where]) and np.array_equal(so, uso[where]) and np.array_equal(po, upo[where])


@pytest.mark.parametrize("tree", ["hash-ready", "montgomery-col", "montgomery-leaf"])
def test_an_index_equal_to_n_leaves_is_refused_and_the_context_stays_usable(ctx, open_trees, tree):
    from provekit_amd import ProveKitHipError
    from provekit_amd._lib import LEAVES_MONTGOMERY, LEAVES_SCALED32, PK_COL_MAJOR, lib

    opener, heap, rows = open_trees[tree]
    n = OPEN_N
    for bad in ([n], [0, n, 1], [5, 6, n]):
        with pytest.raises(ProveKitHipError, match="out of range"):
            open_at(ctx, opener, np.array(bad, dtype=np.uint64), 1)
    good = np.array([n - 1, 0], dtype=np.uint64)
    lo, so, po = open_at(ctx, opener, good, 1)
    assert np.array_equal(lo, rows[1][[n - 1, 0]]) and np.array_equal(so, ref_siblings(heap, n, good)) and np.array_equal(po, ref_paths(heap, n, good))
    # the row gather on its own refuses it too (a two-leaf buffer of its own: the index one past its end)
    enc = LEAVES_SCALED32 if tree == "hash-ready" else LEAVES_MONTGOMERY
    d = ctx.upload(sc.to_limbs([1, 2, 3, 4, 5, 6]))
    out = np.zeros((1, 3, 4), dtype=np.uint64)
    two = np.array([2], dtype=np.uint64)
    with pytest.raises(ProveKitHipError, match="out of range"):
        ctx._check(lib.pk_gather_leaves_enc(ctx.handle, d.ptr, 2, 3, PK_COL_MAJOR, enc, two.ctypes.data, 1, 1, out.ctypes.data))
    one = np.array([1], dtype=np.uint64)
    ctx._check(lib.pk_gather_leaves_enc(ctx.handle, d.ptr, 2, 3, PK_COL_MAJOR, enc, one.ctypes.data, 1, 1, out.ctypes.data))
    conv = sc.canonical_opening if tree == "hash-ready" else (lambda x: x * pow(sc.R, -1, P) % P)
    assert sc.from_limbs(out) == [conv(x) for x in (2, 4, 6)]


# ---- (e) the Montgomery-form leaf hash at the same edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [3, 31, 33, 64])
@pytest.mark.parametrize("version", [2, 1])
def test_montgomery_leaf_hash_at_the_lane_edges_with_planted_elements(ctx, oracle, version, width):
    """pk_leaf_hash (Montgomery images in, mont_to_scaled29 in front of the fold) at 1, 255, 256, 257 leaves, both layouts, with the
    images 0, 1, p - 1 and R mod p (the image of one) planted as seeds and as later elements"""
    from provekit_amd._lib import PK_COL_MAJOR, PK_LEAF_MAJOR, lib
    from provekit_amd.field import random_field

    planted = sc.to_limbs([0, 1, P - 1, sc.R % P])
    leaves = random_field(257 * width, 2500 + width).reshape(257, width, 4)
    for t in range(4):
        leaves[t, 0] = planted[t]                      # a seed
        leaves[4 + t, 1 + t % (width - 1)] = planted[t]  # a later element
        leaves[253 + t, width - 1] = planted[t]        # the last element, on either side of the workgroup's edge
    leaves[0, width - 1], leaves[256, 0] = planted[3], planted[2]
    want = oracle.leaf_hash(leaves, version)
    ctx.set_hash_version(version)
    try:
        for n in (1, 255, 256, 257):
            for layout, arr in ((PK_LEAF_MAJOR, leaves[:n]), (PK_COL_MAJOR, leaves[:n].transpose(1, 0, 2))):
                d_l, d_out = ctx.upload(arr), ctx.upload(sentinel(n + 1))
                ctx._check(lib.pk_leaf_hash(ctx.handle, d_l.ptr, n, width, layout, d_out.ptr))
                got = ctx.download_fe(d_out, n + 1)
                assert np.array_equal(got[:n], want[:n]) and np.array_equal(got[n], sentinel(1)[0]), (n, layout)
    finally:
        ctx.set_hash_version(2)
