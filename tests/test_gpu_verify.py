"""GPU: the compiled verifier's device path (libprovekit_verify.so, pkv_verify_many) on pk_prove's own proofs: acceptance at the sizes
of test_gpu_prove.py, agreement with the host core (verdict and failing check) on a batch with tampered members, the openings kernel
against the reference's own Merkle data, the batched matrix evaluation against the product's kernels, and proofs made by the
engine.  Field values throughout: every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
G = os.path.join(ROOT, "tests", "golden")


def small_statement(ctx, oracle, m, m_0, nc, n_in, seed, pow_bits):
    """the instance tests/test_gpu_prove.py::run_case proves -> (scheme, r1cs, device witness, verifier, oracle arguments)"""
    import verifier as V
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
    from provekit_amd.sparse_matrix import R1CS
    from provekit_amd.verify import Verifier
    from test_gpu_prove import satisfiable_r1cs, to_sparse

    nw, z, coeffs, trips = satisfiable_r1cs(nc, n_in, seed)
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    sparse = [to_sparse(nc, nw, t) for t in trips]
    r1cs = R1CS(ctx, *sparse, interner)
    cfg_w = WhirConfig.for_size(m, pow_bits)
    cfg_w.num_queries = [20, 12, 9, 8][: cfg_w.n_rounds]
    cfg_b = blinding_config_for(m_0, pow_bits)
    scheme = WhirR1CSScheme(ctx, r1cs, m, m_0, cfg_w, cfg_b)
    d_z = ctx.upload(oracle.to_mont(oracle.ints_to_limbs(z)))
    ver = Verifier.for_scheme(scheme, sparse, interner)

    def vcfg(c):
        return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, c.num_queries, c.ood_samples, c.pow_bits,
                            c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)

    mats = [(t[0], t[1], [coeffs[v] for v in t[2]]) for t in trips]
    oracle_args = dict(args=(scheme.domain_separator, m, m_0, vcfg(cfg_w), vcfg(cfg_b)), r1cs=(nc, nw, mats))
    return scheme, r1cs, d_z, ver, oracle_args


@pytest.mark.parametrize("m,m_0,nc,n_in,seed,pow_bits", [(9, 7, 100, 60, 3, 6.0), (12, 9, 500, 700, 5, 4.0), (17, 16, 60000, 5000, 17, 10.0)])
def test_pk_prove_proofs_are_accepted(ctx, oracle, m, m_0, nc, n_in, seed, pow_bits):
    import verifier as V

    scheme, r1cs, d_z, ver, o = small_statement(ctx, oracle, m, m_0, nc, n_in, seed, pow_bits)
    proofs = [scheme.prove(d_z, seed=seed), scheme.prove(d_z, seed=seed + 1), scheme.prove(d_z)]
    got = ver.verify_many(proofs)
    print([str(r) for r in got])
    assert all(r.accepted and r.check == "NONE" and r.offset == len(p) for r, p in zip(got, proofs)), got
    assert [ver.verify(p) for p in proofs] == got  # the host core: same verdicts
    if m <= 16:
        assert V.verify(proofs[0], *o["args"], r1cs=o["r1cs"])
    ver.close()
    scheme.close()
    r1cs.close()


def test_the_bench_statement_is_accepted(ctx, oracle):
    """m = 21, m_0 = 20: bench.py's statement under the reference's derived schedule (queries 109/28/16/11, final 9)"""
    sys.path.insert(0, ROOT)
    import bench
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
    from provekit_amd.verify import Verifier

    m, m_0 = 21, 20
    n_wit = (1 << (m - 1)) - 5
    r1cs, mats, interner, nc, n_in = bench.synth_r1cs(ctx, m_0, n_wit, seed=1234)
    d_z, _ = bench.satisfying_witness(ctx, r1cs, n_wit, nc, n_in, 99)
    scheme = WhirR1CSScheme(ctx, r1cs, m, m_0, WhirConfig.derive(m), blinding_config_for(m_0))
    ver = Verifier.for_scheme(scheme, mats, interner)
    proofs = [scheme.prove(d_z), scheme.prove(d_z, seed=5)]
    bad = bytearray(proofs[1])
    bad[len(bad) // 2] ^= 1
    got = ver.verify_many(proofs + [bytes(bad)])
    print([str(r) for r in got])
    assert got[0].accepted and got[1].accepted and not got[2].accepted
    host = ver.verify(proofs[0])
    assert host == got[0] and ver.verify(bytes(bad)) == got[2]
    # the matrix check bites: the same proof under a statement with one coefficient changed
    other = Verifier.for_scheme(scheme, mats, interner, attach=False)
    from provekit_amd.sparse_matrix import SparseMatrix

    vals = mats[1].values.copy()
    vals[len(vals) // 2] ^= 1
    other.set_r1cs(mats[0], SparseMatrix(mats[1].num_rows, mats[1].num_cols, mats[1].new_row_indices, mats[1].col_indices, vals), mats[2], interner)
    other.attach(ctx)
    r = other.verify_many([proofs[0]])[0]
    assert not r.accepted and r.check == "MATRIX_EVAL", r
    for x in (ver, other, scheme, r1cs):
        x.close()


def test_a_batch_with_tampered_members(ctx, oracle):
    """32 proofs from different seeds, a known subset tampered in different regions: verdicts and failing checks equal the host
    core's, the untampered ones still pass"""
    from test_verify_host import walk_layout

    scheme, r1cs, d_z, ver, _ = small_statement(ctx, oracle, 9, 7, 100, 60, 3, 6.0)
    proofs = [scheme.prove(d_z, seed=100 + i) for i in range(32)]
    assert len(set(proofs)) == 32
    regions = ["root_0", "cubic_message", "quadratic_message", "nonce", "leaf_element", "sibling_digest", "path_digest", "leaf_index", "final_coefficient",
               "deferred_blinding_0", "deferred_witness_1", "claimed_evaluations_g", "hint_length_prefix_high"]
    tampered = {}
    for n, region in enumerate(regions):
        i = (5 * n + 2) % 32
        pos = walk_layout(proofs[i], scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan)
        t = bytearray(proofs[i])
        t[pos[region]] ^= 1
        proofs[i] = bytes(t)
        tampered[i] = region
    proofs[31] = proofs[31][:-7]
    tampered[31] = "truncated"
    assert len(tampered) == len(regions) + 1
    got = ver.verify_many(proofs)
    host = [ver.verify(p) for p in proofs]
    for i, (g, h) in enumerate(zip(got, host)):
        print(i, tampered.get(i, "-"), g)
        assert g == h, (i, tampered.get(i), g, h)
        assert g.accepted == (i not in tampered), (i, tampered.get(i), g)
    assert len({g.check for g in got}) >= 6  # the tampering reached different checks
    ver.close()
    scheme.close()
    r1cs.close()


def reference_openings(oracle):
    """every Merkle opening of the reference's own proof, per tree: (name, root, leaves, siblings, root-to-leaf paths, leaf indexes).
    fixture_merkle.json records the seven trees and their 218 openings but, for size, keeps a prefix of each tree's openings only; the
    rest is read from the proof the fixture was minted from (poseidon-1000.np next to it, by the minting script's own parsers at
    the offsets it uses), and the kept prefix is compared so that the two cannot drift apart."""
    sys.path.insert(0, G)
    import gen_golden as gg
    from provekit_amd.file import read_np

    fix = json.load(open(os.path.join(G, "fixture_merkle.json")))
    assert fix["hash_version"] == 1
    t = read_np(os.path.join(G, "poseidon-1000.np"))
    assert [h[0] for h in gg.HINT_SETS] == [tree["name"] for tree in fix["trees"]]
    out = []
    for (name, off, root_off), tree in zip(gg.HINT_SETS, fix["trees"]):
        pay, nxt = gg.parse_hint(t, off)
        leaves = gg.parse_stir_answers(pay)
        sib, pre, suf, idx = gg.parse_multipath(gg.parse_hint(t, nxt)[0])
        paths = gg.decode_paths(pre, suf)
        assert len(leaves) == len(sib) == len(paths) == len(idx) == tree["n_openings_in_fixture"], name
        assert {len(p) for p in paths} == {tree["height"] - 1} and {len(l) for l in leaves} == {tree["leaf_width"]}, name
        mp, kept = tree["multipath"], len(tree["leaves"])
        assert idx[:kept] == mp["leaf_indexes"] and [gg.hx(x) for x in sib[:kept]] == mp["leaf_sibling_hashes"], name
        assert [[gg.hx(x) for x in p] for p in paths[:kept]] == mp["auth_paths_root_to_leaf"], name
        assert [[gg.hx(x) for x in l] for l in leaves[:kept]] == tree["leaves"], name
        assert gg.hx(int.from_bytes(t[root_off : root_off + 32], "little")) == tree["root"], name
        k, depth = len(idx), tree["height"] - 1
        out.append((name, oracle.hex_to_limbs([tree["root"]]),
                    oracle.ints_to_limbs([x for l in leaves for x in l]).reshape(k, tree["leaf_width"], 4), oracle.ints_to_limbs(sib),
                    oracle.ints_to_limbs([x for p in paths for x in p]).reshape(k, depth, 4), np.array(idx, dtype=np.uint64)))
    return out


def test_openings_kernel_on_the_reference_proofs_merkle_data(ctx, oracle):
    """all 218 openings of the reference's proof fixture reach their roots under Skyscraper v1; one digest altered: exactly that one fails"""
    from provekit_amd.verify import openings_check

    total = 0
    for name, root, leaves, sibs, paths, idx in reference_openings(oracle):
        k = len(idx)
        roots = np.repeat(root, k, axis=0)
        reached, _ = openings_check(ctx, leaves, sibs, paths, idx, roots, hash_version=1)
        assert reached.all(), (name, reached)
        assert not openings_check(ctx, leaves, sibs, paths, idx, roots, hash_version=2)[0].any()
        total += k
        # one digest altered, a path digest and then the sibling: that opening fails, the others do not.  (Neighbours may share a
        # path digest in the proof's prefix compression, not here: every opening has its own copy.)
        q = k // 2
        bad = paths.copy()
        bad[q, paths.shape[1] // 2, 0] ^= np.uint64(1)
        reached, _ = openings_check(ctx, leaves, sibs, bad, idx, roots, hash_version=1)
        assert [int(i) for i in np.flatnonzero(~reached)] == [q], name
        bad = sibs.copy()
        bad[k - 1, 0] ^= np.uint64(1)
        reached, _ = openings_check(ctx, leaves, bad, paths, idx, roots, hash_version=1)
        assert [int(i) for i in np.flatnonzero(~reached)] == [k - 1], name
    assert total == 218


def test_fold_values_equal_the_definition(ctx, oracle):
    """the opening's fold value: MultivarPoly(leaf combined by beta, r) (utilities.go:15-22, mtUtilities.go:98-114) on Python ints"""
    import pyref as pr
    from provekit_amd.field import random_field
    from provekit_amd.verify import openings_check

    rng = np.random.default_rng(4)
    k, width, depth = 7, 32, 3
    leaves_c = oracle.from_mont(random_field(k * width, 9)).reshape(k, width, 4)
    ints = [oracle.limbs_to_ints(l) for l in leaves_c]
    beta, rs = 0x1234567 * 987654321987654321 % pr.P, [int(x) * 1000003 % pr.P for x in rng.integers(1, 2**62, size=4)]
    w = []
    for b in range(2):
        for j in range(16):
            v = pow(beta, b, pr.P)
            for t in range(4):
                if (j >> t) & 1:
                    v = v * rs[t] % pr.P
            w.append(v)
    zeros = np.zeros((k, 4), dtype=np.uint64)
    _, folds = openings_check(ctx, leaves_c, zeros, np.zeros((k, depth, 4), dtype=np.uint64), np.arange(k, dtype=np.uint64), zeros,
                              weights=oracle.to_mont(oracle.ints_to_limbs(w)))
    want = [pr.multivar_poly([(l[j] + beta * l[16 + j]) % pr.P for j in range(16)], rs) for l in ints]
    assert oracle.limbs_to_ints(folds) == want


def test_batched_matrix_evaluation_equals_the_products_kernels(ctx, oracle):
    """K = 1 and K = 5 on a statement with a dense column and a long row: value for value pk_r1cs_external_row then pk_dot against
    pk_eq_table(y); and the C oracle's evaluator"""
    import ctypes as C

    from provekit_amd._lib import lib
    from provekit_amd.field import random_field
    from provekit_amd.scheme import WhirConfig, blinding_config_for
    from provekit_amd.sparse_matrix import R1CS, SparseMatrix
    from provekit_amd.verify import Verifier
    from test_gpu_prove import satisfiable_r1cs

    m, m_0, nc, n_in = 12, 9, 500, 700
    nw, _, coeffs, trips = satisfiable_r1cs(nc, n_in, 5)
    A, B, Cm = ([list(x) for x in t] for t in trips)
    for i in range(nc):  # the constant-one witness' column: every row of C reads it
        Cm[0].append(i); Cm[1].append(0); Cm[2].append(3)
    keep = [i for i, r in enumerate(B[0]) if r != nc - 1]
    B = [[x[i] for i in keep] for x in B]
    for c in range(nw):  # a grand sum: the last row of B reads every witness
        B[0].append(nc - 1); B[1].append(c); B[2].append(int(c % len(coeffs)))
    sparse = []
    for rows, cols, vals in (A, B, Cm):
        order = np.lexsort((np.array(cols), np.array(rows)))
        r, c, v = (np.array(x, dtype=np.int64)[order] for x in (rows, cols, vals))
        sparse.append(SparseMatrix(nc, nw, np.searchsorted(r, np.arange(nc)).astype(np.uint32), c.astype(np.uint32), v.astype(np.uint32)))
    assert max(np.bincount(sparse[2].col_indices)) == nc and np.diff(np.append(sparse[1].new_row_indices, sparse[1].nnz)).max() >= nw
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    r1cs = R1CS(ctx, *sparse, interner)
    ver = Verifier(m, m_0, WhirConfig.for_size(m, 4.0), blinding_config_for(m_0, 4.0))
    ver.set_r1cs(*sparse, interner)
    ver.attach(ctx)
    alphas, points = random_field(5 * m_0, 21).reshape(5, m_0, 4), random_field(5 * (m - 1), 22).reshape(5, m - 1, 4)
    want = np.zeros((5, 3, 4), dtype=np.uint64)
    eq_a, eq_y, out = ctx.alloc_fe(1 << m_0), ctx.alloc_fe(1 << (m - 1)), np.zeros(4, dtype=np.uint64)
    for k in range(5):
        ctx._check(lib.pk_eq_table(ctx.handle, np.ascontiguousarray(alphas[k]).ctypes.data, m_0, eq_a.ptr))
        ctx._check(lib.pk_eq_table(ctx.handle, np.ascontiguousarray(points[k]).ctypes.data, m - 1, eq_y.ptr))
        ext = r1cs.calculate_external_row_of_r1cs_matrices(eq_a)
        for mat in range(3):
            ctx._check(lib.pk_dot(ctx.handle, ext.view_fe(mat * nw), eq_y.ptr, nw, out.ctypes.data))
            want[k, mat] = out
    assert np.array_equal(ver.matrix_evaluations(alphas[:1], points[:1]), want[:1])
    assert np.array_equal(ver.matrix_evaluations(alphas, points), want)
    # the C oracle's bilinear form (tests/oracle_lib.matrix_evaluator) on canonical ints
    csr = [(s.new_row_indices, s.col_indices, s.values) for s in sparse]
    ev = oracle.matrix_evaluator(nc, nw, csr, interner)
    for k in (0, 4):
        a, y = oracle.limbs_to_ints(oracle.from_mont(alphas[k])), oracle.limbs_to_ints(oracle.from_mont(points[k]))
        assert ev(a, y) == oracle.limbs_to_ints(oracle.from_mont(want[k]))
    ver.close()
    r1cs.close()


def test_engine_proofs_verify_in_one_call(ctx, oracle):
    import provekit_amd

    scheme, r1cs, d_z, ver, _ = small_statement(ctx, oracle, 12, 9, 500, 700, 5, 4.0)
    with provekit_amd.ProofEngine(r1cs, scheme.m, scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan, lanes=4) as eng:
        proofs = eng.prove_many([d_z] * 12, list(range(40, 52)))
    assert len(set(proofs)) == 12
    got = ver.verify_many(proofs)
    assert all(r.accepted for r in got), got
    ver.close()
    scheme.close()
    r1cs.close()
