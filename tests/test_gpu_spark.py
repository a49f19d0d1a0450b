"""GPU: libprovekit_spark.so on the device.  The matrix's columns and a query's gathered columns bit for bit against Python ints
(tests/spark_refs.py) at shapes that cross the kernels' seams, for every entry pattern and several grids, with nothing written past an
output's end, the inputs unchanged and an index outside the matrix refused with the smallest entry and nothing written; the proof bytes
and claims against the Python reference; a prover reused, a short buffer, the refusals with their reasons; one larger size against
pkw_evaluate; the composition with libprovekit_whir.so; the one stacked query of an R1CS against pkv_matrix_evaluations; the C++
example."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import prodcheck_refs as K  # noqa: E402
import spark_refs as X  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(2, seed=47)
GRIDS = (1, 3, 0)  # workgroups (0: the library's rule)
PATTERNS = ("random", "one column", "distinct", "duplicates", "padding")
SENTINEL = 0xA5
ENTRY_COLUMNS = ("row", "col", "val", "e_row", "e_col")


def rows_of(stmt, name):
    return 1 << (stmt[0] if name in ENTRY_COLUMNS else stmt[1] if name == "m_row" else stmt[2])


def sentinel_fe(ctx, rows):
    """rows + 1 elements of sentinel bytes on the device: what a kernel does not write stays"""
    return ctx.upload(np.full((rows + 1, 4), int.from_bytes(bytes([SENTINEL]) * 8, "little"), dtype=np.uint64))


def untouched(ctx, buf, rows, first=None):
    """the element behind the end is the sentinel; first=0: the whole buffer is"""
    start = rows if first is None else first
    return ctx.download_fe(buf, rows + 1)[start:].tobytes() == bytes([SENTINEL]) * 32 * (rows + 1 - start)


def point(kind, count, seed):
    """`count` coordinates: "random", or with 0, 1 and -1 among them, so that the eq table holds zeros"""
    r = K.random_elements(count, seed)
    if kind == "edges":
        for i, v in zip(range(count), (0, 1, P - 1)):
            r[i] = v
    return r


class Device:
    """a query's columns on the device"""

    def __init__(self, ctx, stmt):
        self.ctx, self.stmt, self.bufs = ctx, stmt, {}

    def put(self, Q, names=X.COLUMNS):
        for name in names:
            if name in self.bufs:
                self.bufs[name].free()
            self.bufs[name] = self.ctx.upload(K.mont(Q[name]))
        return self

    def outputs(self, names):
        for name in names:
            if name in self.bufs:
                self.bufs[name].free()
            self.bufs[name] = sentinel_fe(self.ctx, rows_of(self.stmt, name))
        return self

    def get(self, name):
        return K.unmont(self.ctx.download_fe(self.bufs[name], rows_of(self.stmt, name)))

    def free(self):
        for buf in self.bufs.values():
            buf.free()
        self.bufs = {}


def indices(ctx, M):
    images = [np.asarray(M[c], dtype=np.uint32) for c in ("row_idx", "col_idx")]
    return images, [ctx.upload(a) for a in images]


def columns_case(ctx, prover, stmt, kind):
    """every pattern at one statement: pkx_matrix and pkx_begin against the reference"""
    from tools.pk_probes import lib as probes
    from provekit_amd import spark as sp

    n, s, t = stmt
    dev = Device(ctx, stmt)
    for number, name in enumerate(PATTERNS):
        M = X.matrix(n, s, t, *X.random_entries(n, s, t, seed=1000 * n + 10 * s + t + number, pattern_name=name))
        if name == "one column":
            assert M["m_col"][0] == 1 << n
        if name == "padding":
            assert M["m_row"][0] == M["m_col"][0] == 1 << n and not any(M["val"])
        rx, ry = point(kind, s, 7 * number + 1), point(kind, t, 7 * number + 2)
        Q = X.query(M, rx, ry)
        if kind == "edges" and s > 1:
            assert 0 in X.eq_table(rx)
        images, (d_row_idx, d_col_idx) = indices(ctx, M)
        for grid in GRIDS if name in ("random", "one column") else (0,):
            assert probes.pk_probe_spark_set_grid(prover.handle, grid) == 0
            dev.outputs(("row", "col", "m_row", "m_col", "e_row", "e_col"))
            b = dev.bufs
            prover.matrix(d_row_idx, d_col_idx, b["row"], b["col"], b["m_row"], b["m_col"])
            assert prover.first_bad == sp.NO_BAD_ENTRY
            prover.begin(d_row_idx, d_col_idx, K.mont(rx), K.mont(ry), b["e_row"], b["e_col"])
            assert prover.first_bad == sp.NO_BAD_ENTRY
            for col in ("row", "col", "m_row", "m_col", "e_row", "e_col"):
                assert dev.get(col) == Q[col], (name, grid, col)
                assert untouched(ctx, b[col], rows_of(stmt, col)), (name, grid, col)  # nothing past the end
        # the inputs are unchanged
        for image, d in zip(images, (d_row_idx, d_col_idx)):
            assert ctx.download(d, (1 << n,), np.uint32).tobytes() == image.tobytes()
            d.free()
    dev.free()


def shapes():
    from provekit_amd import spark as sp

    L = sp.count_lds_max()
    out = [(1, 1, 1), (3, 2, 5), (3, L - 1, L + 1), (9, L, 2), (10, 3, L), (8, L + 1, L - 1)]
    return out


@pytest.mark.parametrize("which", range(6))
def test_the_columns_are_the_references_for_every_pattern_and_grid(ctx, which):
    """n = 1, 3 and around one workgroup's sweep of the gather (2^9 entries); s and t at the LDS histogram's threshold, below and above
    it; the points' kinds go round"""
    from provekit_amd import spark as sp

    stmt = shapes()[which]
    prover = sp.Prover(ctx, sp.Statement(*stmt))
    columns_case(ctx, prover, stmt, ("random", "edges")[which % 2])
    prover.close()


def test_the_eq_tables_hold_zeros_for_points_with_coordinates_0_1_and_minus_1(ctx):
    from provekit_amd import spark as sp

    stmt = (5, 3, 4)
    prover = sp.Prover(ctx, sp.Statement(*stmt))
    columns_case(ctx, prover, stmt, "edges")
    prover.close()


@pytest.mark.parametrize("where", ["entry 0", "the last entry", "two entries", "2^32 - 1"])
@pytest.mark.parametrize("stmt", [(1, 1, 1), (5, 3, 2), (11, 4, 13)])
def test_an_index_outside_the_matrix_is_refused_with_the_smallest_entry_and_nothing_is_written(ctx, stmt, where):
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    n, s, t = stmt
    row_idx, col_idx, val = X.random_entries(n, s, t, seed=3)
    good = X.matrix(n, s, t, row_idx, col_idx, val)
    row_idx, col_idx = list(row_idx), list(col_idx)
    entries = 1 << n
    if where == "entry 0":
        row_idx[0], want = 1 << s, 0
    elif where == "the last entry":
        col_idx[entries - 1], want = 1 << t, entries - 1
    elif where == "two entries":
        row_idx[entries - 1], col_idx[entries // 2], want = 1 << s, (1 << t) + 7, entries // 2
    else:
        row_idx[entries // 2], want = 2**32 - 1, entries // 2
    prover = sp.Prover(ctx, sp.Statement(*stmt))
    names = ("row", "col", "m_row", "m_col", "e_row", "e_col")
    dev = Device(ctx, stmt).outputs(names)
    b = dev.bufs
    d_row_idx, d_col_idx = ctx.upload(np.asarray(row_idx, dtype=np.uint32)), ctx.upload(np.asarray(col_idx, dtype=np.uint32))
    rx, ry = K.random_elements(s, 1), K.random_elements(t, 2)
    with pytest.raises(ProveKitHipError, match="entry %d: its row is outside" % want) as e:
        prover.matrix(d_row_idx, d_col_idx, b["row"], b["col"], b["m_row"], b["m_col"])
    assert e.value.code == sp.ERR_BAD_ARG and prover.first_bad == want
    for col in ("row", "col", "m_row", "m_col"):  # every entry is validated before anything of the caller's is written: nothing was
        assert untouched(ctx, b[col], rows_of(stmt, col), first=0), col
    with pytest.raises(ProveKitHipError, match="entry %d: its row is outside" % want) as e:
        prover.begin(d_row_idx, d_col_idx, K.mont(rx), K.mont(ry), b["e_row"], b["e_col"])
    assert e.value.code == sp.ERR_BAD_ARG and prover.first_bad == want
    for col in ("e_row", "e_col"):  # the bad index was followed nowhere past a table's end, and nothing is written past the outputs'
        assert untouched(ctx, b[col], rows_of(stmt, col)), col
    # the prover stays usable
    ctx.upload_into(d_row_idx.ptr, np.asarray(good["row_idx"], dtype=np.uint32))
    ctx.upload_into(d_col_idx.ptr, np.asarray(good["col_idx"], dtype=np.uint32))
    prover.matrix(d_row_idx, d_col_idx, b["row"], b["col"], b["m_row"], b["m_col"])
    prover.begin(d_row_idx, d_col_idx, K.mont(rx), K.mont(ry), b["e_row"], b["e_col"])
    Q = X.query(good, rx, ry)
    assert prover.first_bad == sp.NO_BAD_ENTRY and all(dev.get(col) == Q[col] for col in names)
    d_row_idx.free(), d_col_idx.free()
    dev.free()
    prover.close()


def test_arena_bytes_states_the_tables_the_counts_and_the_three_inner_provers(ctx):
    from provekit_amd import spark as sp, tuplelookup as tl

    def up(b):
        return (b + 63) // 64 * 64

    for n, s, t in ((1, 1, 1), (12, 7, 9), (5, 13, 3)):
        lookups = tl.arena_bytes(tl.Statement(n, s, 2, 1, 1)) + tl.arena_bytes(tl.Statement(n, t, 2, 1, 1))
        # the two eq tables and the index column; the counts; the cell of the first bad entry -- every part rounded up to 64 bytes
        own = up(32 << s) + up(32 << t) + up(32 << max(s, t)) + up(4 << s) + up(4 << t) + 64
        # ... and the sumcheck prover's arena: three folded copies of half length, one round's scratch (four partials a workgroup of up to
        # 1024, and 8 results), the split eq weights of n - 1 variables
        low = (n - 1) // 2
        val = 32 * (3 * (1 << (n - 1)) + 4 * 1024 + 8 + (2 << (n - 1 - low)) + (2 << low) - 2)
        assert sp.arena_bytes(sp.Statement(n, s, t)) == lookups + own + val
        prover = sp.Prover(ctx, sp.Statement(n, s, t))  # and a prover of it is made and given back
        prover.close()


def same_claims(claims, ref):
    assert K.unmont(claims.value) == [ref["value"]]
    assert K.unmont(claims.z_val) == ref["z_val"] and K.unmont(claims.val_values) == ref["val_values"]
    for side in range(2):
        assert K.unmont(claims.beta[side]) == [ref["beta"][side]] and K.unmont(claims.f_value[side]) == [ref["f_value"][side]]
        assert K.unmont(claims.m_value[side]) == [ref["m_value"][side]]
        for name in ("z_f", "f_coeff", "z_m"):
            assert K.unmont(getattr(claims, name)[side]) == ref[name][side], (name, side)


@pytest.mark.parametrize("size", [(1, 1, 1), (2, 3, 1), (3, 1, 2), (4, 3, 3)])
def test_proof_bytes_and_claims_are_the_references_and_a_prover_proves_two_queries(ctx, size):
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    n, s, t = size
    stmt, bind = sp.Statement(n, s, t, 2), K.mont(BIND)
    prover = sp.Prover(ctx, stmt)
    M = X.matrix(n, s, t, *X.random_entries(n, s, t, seed=100 * n + 10 * s + t))
    _, (d_row_idx, d_col_idx) = indices(ctx, M)
    dev = Device(ctx, size).put(M, ("val",)).outputs(("row", "col", "m_row", "m_col", "e_row", "e_col"))
    b = dev.bufs
    prover.matrix(d_row_idx, d_col_idx, b["row"], b["col"], b["m_row"], b["m_col"])  # once: the matrix
    proofs = []
    for seed, kind in ((1, "random"), (2, "edges")):  # the same prover and matrix, two queries
        rx, ry = point(kind, s, 10 * seed), point(kind, t, 10 * seed + 1)
        Q = X.query(M, rx, ry)
        ref = X.prove(n, s, t, Q, rx, ry, BIND)
        prover.begin(d_row_idx, d_col_idx, K.mont(rx), K.mont(ry), b["e_row"], b["e_col"])
        proof, value, claims = prover.prove(b, K.mont(rx), K.mont(ry), bind)
        assert proof == ref["proof"] and len(proof) == sp.proof_bytes(stmt)
        assert K.unmont(value) == [ref["value"]] == [X.dense_value(M, s, t, rx, ry)]
        same_claims(claims, ref)
        res, side, layer, seen = sp.verify(stmt, proof, K.mont(rx), K.mont(ry), bind, expected_value=value)
        assert res.accepted and res.offset == len(proof), res
        same_claims(seen, ref)
        assert prover.prove(b, K.mont(rx), K.mont(ry), bind)[0] == proof  # again: the same bytes
        proofs.append(proof)
    assert proofs[0] != proofs[1]
    # a short buffer: the length is told, nothing is proved or written, the prover stays usable
    prover.fill = SENTINEL
    with pytest.raises(ProveKitHipError, match="the proof buffer holds") as e:
        prover.prove(b, K.mont(rx), K.mont(ry), bind, capacity=len(proof) - 1)
    assert e.value.code == -1 and prover.last_len == len(proof) and bytes(prover.buffer) == bytes([SENTINEL]) * (len(proof) - 1)
    assert prover.prove(b, K.mont(rx), K.mont(ry), bind)[0] == proof
    for name in X.COLUMNS:  # the caller's columns are unchanged
        assert dev.get(name) == Q[name]
    d_row_idx.free(), d_col_idx.free()
    dev.free()
    prover.close()


def test_columns_that_are_no_read_of_the_eq_tables_are_refused_with_the_sides_reason_and_nothing_is_written(ctx):
    from provekit_amd import spark as sp
    from provekit_amd._lib import ProveKitHipError

    n, s, t = 4, 3, 2
    stmt, bind = sp.Statement(n, s, t, 2), K.mont(BIND)
    M = X.matrix(n, s, t, *X.random_entries(n, s, t, seed=12))
    rx, ry = K.random_elements(s, 1), K.random_elements(t, 2)
    Q = X.query(M, rx, ry)
    honest_ref = X.prove(n, s, t, Q, rx, ry, BIND)
    prover = sp.Prover(ctx, stmt)
    prover.fill = SENTINEL
    good = Device(ctx, (n, s, t)).put(Q)
    honest = prover.prove(good.bufs, K.mont(rx), K.mont(ry), bind)[0]
    assert honest == honest_ref["proof"]

    def refused(column, index, reason, value=None):
        changed = {c: list(v) for c, v in Q.items()}
        changed[column][index] = (changed[column][index] + 1) % P if value is None else value
        bad = Device(ctx, (n, s, t)).put(changed)
        with pytest.raises(ProveKitHipError, match=reason) as e:
            prover.prove(bad.bufs, K.mont(rx), K.mont(ry), bind)
        assert e.value.code == sp.ERR_UNSATISFIED
        assert bytes(prover.buffer) == bytes([SENTINEL]) * len(honest)  # nothing is written
        assert prover.prove(good.bufs, K.mont(rx), K.mont(ry), bind)[0] == honest  # and the same prover then proves the good columns
        bad.free()

    refused("e_row", 5, r"side ROW: \(row, e_row\) is not a read of eq\(rx, \.\) under m_row: .*a row is not in t: stacked index 5 ")
    refused("e_col", 9, r"side COL: \(col, e_col\) is not a read of eq\(ry, \.\) under m_col: .*a row is not in t: stacked index 9 ")
    refused("m_row", 1, r"side ROW: .*m is wrong")
    refused("m_col", 0, r"side COL: .*m is wrong")
    refused("row", 3, r"side ROW: .*a row is not in t: stacked index 3 ", value=1 << s)  # no index of the matrix
    # a wrong val is no refusal: it is another matrix, with another value
    changed = dict(Q, val=[(Q["val"][0] + 1) % P] + Q["val"][1:])
    other = Device(ctx, (n, s, t)).put(changed)
    proof, value, _ = prover.prove(other.bufs, K.mont(rx), K.mont(ry), bind)
    assert K.unmont(value) == [X.value(changed, rx, ry)] != [honest_ref["value"]]
    assert sp.verify(stmt, proof, K.mont(rx), K.mont(ry), bind, expected_value=K.mont([honest_ref["value"]])[0])[0].check == "SUM"
    other.free()
    good.free()
    prover.close()


def evaluations(ctx, whir_pcs, b, stmt, claims):
    """the nine evaluations of the claims from the device columns (pkw_evaluate)"""
    n, s, t = stmt
    three = np.stack([claims.z_val, claims.z_f[0], claims.z_f[1]])  # the two batches a caller commits, each at the three points
    at = np.concatenate([whir_pcs.evaluate(ctx, [b[c] for c in ("val", "row", "col")], n, three), whir_pcs.evaluate(ctx, [b[c] for c in ("e_row", "e_col")], n, three)])
    m_row = whir_pcs.evaluate(ctx, [b["m_row"]], s, claims.z_m[0][None])[0, 0]
    m_col = whir_pcs.evaluate(ctx, [b["m_col"]], t, claims.z_m[1][None])[0, 0]
    return np.stack([at[0, 0], at[3, 0], at[4, 0]]), np.stack([at[1, 1], at[3, 1]]), m_row, np.stack([at[2, 2], at[4, 2]]), m_col


def test_one_larger_query_is_verified_and_its_nine_claims_hold_of_the_columns_evaluations(ctx):
    """n = 12, s = 10, t = 11: nothing is proved in Python at this size"""
    from provekit_amd import spark as sp, whir_pcs

    stmt3 = (12, 10, 11)
    n, s, t = stmt3
    M = X.matrix(n, s, t, *X.random_entries(n, s, t, seed=1210))
    rx, ry = K.random_elements(s, 5), K.random_elements(t, 6)
    Q = X.query(M, rx, ry)
    stmt = sp.Statement(n, s, t)
    prover = sp.Prover(ctx, stmt)
    _, (d_row_idx, d_col_idx) = indices(ctx, M)
    dev = Device(ctx, stmt3).put(M, ("val",)).outputs(("row", "col", "m_row", "m_col", "e_row", "e_col"))
    b = dev.bufs
    prover.matrix(d_row_idx, d_col_idx, b["row"], b["col"], b["m_row"], b["m_col"])
    prover.begin(d_row_idx, d_col_idx, K.mont(rx), K.mont(ry), b["e_row"], b["e_col"])
    assert all(dev.get(col) == Q[col] for col in ("row", "col", "m_row", "m_col", "e_row", "e_col"))
    proof, value, claims = prover.prove(b, K.mont(rx), K.mont(ry))
    assert len(proof) == sp.proof_bytes(stmt) and K.unmont(value) == [X.value(M, rx, ry)]
    res, side, layer, seen = sp.verify(stmt, proof, K.mont(rx), K.mont(ry), expected_value=value)
    assert res.accepted and res.offset == len(proof), res
    assert np.array_equal(seen.value, claims.value) and np.array_equal(seen.z_val, claims.z_val) and np.array_equal(seen.val_values, claims.val_values)
    for name in ("beta", "z_f", "f_coeff", "f_value", "z_m", "m_value"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(seen, name), getattr(claims, name))), name
    evs = evaluations(ctx, whir_pcs, b, stmt3, seen)
    assert sp.check_claims(stmt, seen, *evs) == "NONE"
    for group, index, which in ((0, 0, "VAL"), (0, 2, "E_COL"), (1, 1, "ROW"), (3, 0, "COL")):
        bad = [e.copy() for e in evs]
        bad[group][index] = K.mont([(K.unmont(bad[group][index])[0] + 1) % P])[0]
        assert sp.check_claims(stmt, seen, *bad) == which
    assert sp.check_claims(stmt, seen, evs[0], evs[1], evs[4], evs[3], evs[4]) == "M_ROW" and sp.check_claims(stmt, seen, evs[0], evs[1], evs[2], evs[3], evs[2]) == "M_COL"
    d_row_idx.free(), d_col_idx.free()
    dev.free()
    prover.close()


def test_composition_with_the_commitment_scheme(ctx):
    """commit the matrix's columns once -- {row, col, val} as one batch, m_row, m_col -- then for a query commit {e_row, e_col}, bind the
    four roots, prove, open both batches at z_val, z_f[0] and z_f[1] in one opening each and the multiplicities at their points, verify
    the openings, check the claims on the opened values; with one evaluation changed the claims fail"""
    import whir_pcs_cases as W
    from provekit_amd import spark as sp, whir_pcs

    stmt3 = (6, 4, 5)
    n, s, t = stmt3
    M = X.matrix(n, s, t, *X.random_entries(n, s, t, seed=64))
    rx, ry = K.random_elements(s, 1), K.random_elements(t, 2)
    dev = Device(ctx, stmt3).put(X.query(M, rx, ry))
    b = dev.bufs
    cfgs = [W.small_config(n, 3), W.small_config(s, 1), W.small_config(t, 1), W.small_config(n, 2)]
    schemes = [whir_pcs.Scheme(ctx, cfg) for cfg in cfgs]
    groups = [[b[c] for c in ("row", "col", "val")], [b["m_row"]], [b["m_col"]], [b["e_row"], b["e_col"]]]
    coms = [scheme.commit(group) for scheme, group in zip(schemes, groups)]
    bind = K.mont([int.from_bytes(com.root(), "little") for com in coms])
    stmt = sp.Statement(n, s, t, 4)
    prover = sp.Prover(ctx, stmt)
    proof, value, _ = prover.prove(b, K.mont(rx), K.mont(ry), bind)
    res, side, layer, seen = sp.verify(stmt, proof, K.mont(rx), K.mont(ry), bind, expected_value=value)
    assert res.accepted, res
    three = np.stack([seen.z_val, seen.z_f[0], seen.z_f[1]])
    opened = []
    for scheme, cfg, com, points in zip(schemes, cfgs, coms, (three, seen.z_m[0][None], seen.z_m[1][None], three)):
        _, opening = scheme.open(com, points)
        wres, wevals = whir_pcs.verify(cfg, points, opening, expected_root=com.root())
        assert wres.accepted, wres
        opened.append(wevals)
    mat, m_row, m_col, e = opened
    evs = [np.stack([mat[2, 0], e[0, 0], e[1, 0]]), np.stack([mat[0, 1], e[0, 1]]), m_row[0, 0], np.stack([mat[1, 2], e[1, 2]]), m_col[0, 0]]
    assert sp.check_claims(stmt, seen, *evs) == "NONE"
    changed = [x.copy() for x in evs]
    changed[3][1] = K.mont([(K.unmont(changed[3][1])[0] + 1) % P])[0]
    assert sp.check_claims(stmt, seen, *changed) == "COL"
    # other roots: other seeds, rejected on side VAL
    res, side, layer, _ = sp.verify(stmt, proof, K.mont(rx), K.mont(ry), K.mont([1, 2, 3, 4]))
    assert not res.accepted and side == "VAL"
    for closing in coms + [prover] + schemes:
        closing.close()
    dev.free()


def test_the_stacked_query_of_an_r1cs_is_the_eq_combination_of_the_verifiers_three_matrix_evaluations(ctx):
    """a small random R1CS: pkv_matrix_evaluations gives eq(alpha)^T {A, B, C} eq(point); the one stacked query at ((u, alpha), point)
    proves their eq(u, .) combination"""
    import oracle_lib as oracle
    from provekit_amd import spark as sp
    from provekit_amd.scheme import WhirConfig, blinding_config_for
    from provekit_amd.verify import Verifier
    from test_gpu_prove import satisfiable_r1cs, to_sparse

    nc, m, m_0 = 60, 8, 6
    nw, _, coeffs, trips = satisfiable_r1cs(nc, 40, 11)
    assert nw <= 1 << (m - 1)
    sparse = [to_sparse(nc, nw, trip) for trip in trips]
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    ver = Verifier(m, m_0, WhirConfig.for_size(m, 4.0), blinding_config_for(m_0, 4.0))
    ver.set_r1cs(*sparse, interner)
    ver.attach(ctx)
    alpha, pt, u = K.random_elements(m_0, 1), K.random_elements(m - 1, 2), K.random_elements(2, 3)
    three = K.unmont(ver.matrix_evaluations(K.mont(alpha)[None], K.mont(pt)[None])[0])
    want = sum(X.eq_hi(u, g) * three[g] for g in range(3)) % P

    s, t = m_0, m - 1
    n = max(1, (sum(sm.nnz for sm in sparse) - 1).bit_length())
    row_idx, col_idx, val = sp.entries_from_r1cs(nc, nw, [(sm.new_row_indices, sm.col_indices, sm.values) for sm in sparse], interner, n, s, t)
    stmt = sp.Statement(n, s + 2, t)
    prover = sp.Prover(ctx, stmt)
    d_row_idx, d_col_idx, d_val = ctx.upload(row_idx), ctx.upload(col_idx), ctx.upload(val)
    stmt3 = (n, s + 2, t)
    dev = Device(ctx, stmt3).outputs(("row", "col", "m_row", "m_col", "e_row", "e_col"))
    b = dict(dev.bufs, val=d_val)
    rx = u + alpha
    prover.matrix(d_row_idx, d_col_idx, b["row"], b["col"], b["m_row"], b["m_col"])
    prover.begin(d_row_idx, d_col_idx, K.mont(rx), K.mont(pt), b["e_row"], b["e_col"])
    proof, value, _ = prover.prove(b, K.mont(rx), K.mont(pt))
    assert K.unmont(value) == [want]
    res, side, layer, _ = sp.verify(stmt, proof, K.mont(rx), K.mont(pt), expected_value=K.mont([want])[0])
    assert res.accepted, res
    three[1] = (three[1] + 1) % P  # one deferred value off: the combination is another value, and the proof is not one of it
    off = sum(X.eq_hi(u, g) * three[g] for g in range(3)) % P
    assert sp.verify(stmt, proof, K.mont(rx), K.mont(pt), expected_value=K.mont([off])[0])[0].check == "SUM"
    for buf in (d_row_idx, d_col_idx, d_val):
        buf.free()
    dev.free()
    prover.close()
    ver.close()


def test_the_cpp_demo_commits_a_matrix_once_proves_a_query_opens_checks_the_claims_and_sees_the_refusals():
    demo = os.path.join(ROOT, "examples", "spark_pcs_demo")
    assert os.path.exists(demo), "examples/spark_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "5", "6"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n=9 s=7 t=6 ") and "proof_bytes=%d " % X.proof_bytes(9, 7, 6) in lines[0] and "claims=hold" in lines[0]
    assert lines[1].startswith("a wrong v: rejected check=SUM side=0 offset=32")
    assert lines[2].startswith("one e_row changed: refused rc=-6") and "side ROW" in lines[2] and "a row is not in t" in lines[2]
