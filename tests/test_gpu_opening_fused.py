"""GPU: the fused launches of the WHIR opening -- round 0 of a quadratic sumcheck in the launch that forms its tables
(csrc/mle.hip opening_first_launch: the opening's first kernel and a round's new weights) and the deferred hint without the equality
table (dot_rows_eq) -- each against the sequence of public calls it replaces, bit for bit, on junk-filled outputs so that anything left
unwritten shows; and whole proofs against the oracle's prover (oracle/prover_ref.py).

The whole proof at the bench size is test_gpu_prove.py::test_transcript_equals_the_oracle_provers_at_the_bench_size[21], which runs
the same code.

Not covered here, because not built: the six weighted sums out of the kernel that makes the external rows (EXPERIMENTS.md round 29)."""
import os
import sys

import numpy as np
import pytest

import mle_edge_refs as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
P = E.P
JUNK = 0xA5A5A5A5A5A5A5A5
SCALARS = {"zero": 0, "one": 1, "p-1": P - 1}  # stored values
# n_vars: odd and even splits of the half tables, nhi = 0 (1), more than one workgroup (9), and 2^12 pairs, which a capped grid strides over
N_VARS = [1, 2, 3, 8, 9, 13]
# points: none (overwrite: zeros plus rows), below, at and above a dot29 group of four, and the bench's 109 + 4
POINTS = [0, 1, 2, 4, 5, 113]
TOP = E.limbs([E.TOP])[0]


def row_lengths(N):
    """none, one, an odd length (a pair straddles the rows' end), 2^n - 5 and 2^n, as far as the table has them"""
    return sorted({x for x in (0, 1, N // 2 + 1, N - 5, N) if 0 <= x <= N})


class Tables:
    """the operands of one table size, uploaded once: two evaluation tables, three rows at a stride, an earlier w, and the points"""

    def __init__(self, ctx, n_vars):
        from provekit_amd.field import random_field

        self.ctx, self.n_vars, self.N = ctx, n_vars, 1 << n_vars
        N = self.N
        self.stride = N + 3
        e0, e1, rows, w = random_field(N, 900 + n_vars), random_field(N, 901 + n_vars), random_field(3 * self.stride, 902 + n_vars), random_field(N, 903 + n_vars)
        e0[0] = e1[0] = e1[N - 1] = rows[0] = rows[self.stride] = rows[2 * self.stride + N - 1] = w[0] = w[N - 1] = TOP  # the largest entries
        self.w = w
        self.d_e0, self.d_e1, self.d_rows = ctx.upload(e0), ctx.upload(e1), ctx.upload(rows)
        self.pts = np.ascontiguousarray(random_field(max(POINTS) * n_vars, 904 + n_vars))
        self.scales = np.ascontiguousarray(random_field(max(POINTS), 905 + n_vars))
        self.pts[:n_vars] = TOP
        self.scales[0] = TOP
        self.out = [ctx.alloc_fe(N) for _ in range(4)]  # fused p, w; reference p, w
        self.junk = np.full((N, 4), JUNK, dtype=np.uint64)

    def free(self):
        for b in [self.d_e0, self.d_e1, self.d_rows] + self.out:
            b.free()

    def run(self, q, overwrite, nrows, row_len, beta, g3, nsums, grid=0):
        """one fused launch against pk_eq_accumulate, pk_fe_axpy per row, lincomb2 and pk_sumcheck_quadratic_round.  nrows = 0: a
        round's new weights -- p stands (the reference's combination is made first and both read it), no rows"""
        from provekit_amd._lib import lib
        from tools.pk_probes import lib as probes

        ctx, N, n_vars = self.ctx, self.N, self.n_vars
        p, w, p_ref, w_ref = self.out
        combine = nrows > 0
        bl = E.limbs([beta])
        gl = E.limbs(g3)
        ctx._check(probes.pk_probe_lincomb2(ctx.handle, p_ref.ptr, self.d_e0.ptr, bl.ctypes.data, self.d_e1.ptr, N))
        if combine:
            ctx.upload_into(p.ptr, self.junk)
        else:
            ctx._check(probes.pk_probe_lincomb2(ctx.handle, p.ptr, self.d_e0.ptr, bl.ctypes.data, self.d_e1.ptr, N))
        for d in (w, w_ref):
            ctx.upload_into(d.ptr, self.junk if overwrite else self.w)
        pts, scales = (self.pts.ctypes.data, self.scales.ctypes.data) if q else (None, None)
        got = np.full((3, 4), JUNK, dtype=np.uint64)
        ctx._check(probes.pk_probe_opening_first(ctx.handle, self.d_e0.ptr if combine else None, self.d_e1.ptr if combine else None,
                                                 bl.ctypes.data if combine else None, p.ptr, w.ptr, n_vars, pts, scales, q, int(overwrite),
                                                 self.d_rows.ptr if combine else None, self.stride, nrows, row_len, gl.ctypes.data if combine else None,
                                                 nsums, grid, got.ctypes.data))
        ctx._check(lib.pk_eq_accumulate(ctx.handle, w_ref.ptr, n_vars, pts, scales, q, int(overwrite)))
        for k in range(nrows):
            ctx._check(lib.pk_fe_axpy(ctx.handle, w_ref.ptr, gl[k].ctypes.data, self.d_rows.ptr + 32 * k * self.stride, row_len))
        want = np.zeros((3, 4), dtype=np.uint64)
        ctx._check(lib.pk_sumcheck_quadratic_round(ctx.handle, p_ref.ptr, w_ref.ptr, N, None, None, None, want.ctypes.data))
        what = (n_vars, q, overwrite, nrows, row_len, nsums, grid)
        for name, a, b in (("p", p, p_ref), ("w", w, w_ref)):
            x, y = ctx.download_fe(a, N), ctx.download_fe(b, N)
            assert np.array_equal(x, y), (what, name, int(np.flatnonzero((x != y).any(axis=1))[0]))
        if nsums == 3:
            assert np.array_equal(got, want), (what, E.ints(got), E.ints(want))
        else:  # h(0), h(2); nothing written behind them
            assert np.array_equal(got[:2], want[[0, 2]]) and (got[2] == JUNK).all(), (what, E.ints(got), E.ints(want))


@pytest.fixture(scope="module", params=N_VARS)
def tables(ctx, request):
    t = Tables(ctx, request.param)
    yield t
    t.free()


def test_the_openings_first_launch_equals_the_unfused_sequence(tables):
    """p = e0 + beta e1, w = (0 | w) + the points' equality weights + the scaled rows, and the round's two or three sums"""
    from provekit_amd.field import random_field

    beta, g3 = E.ints(random_field(1, 910))[0], E.ints(random_field(3, 911))
    for q in POINTS:
        for nrows in (1, 3):
            for i, row_len in enumerate(row_lengths(tables.N)):
                for overwrite in (True, False):
                    tables.run(q, overwrite, nrows, row_len, beta, g3, nsums=2 + (i + q + nrows + overwrite) % 2)
    odd = row_lengths(tables.N)[-3] if tables.N > 2 else 1
    for name in SCALARS:  # the combination's and the rows' scalars at 0, 1 and p - 1
        s = SCALARS[name]
        tables.run(2, True, 3, odd, s, [s, s, s], 3)
        tables.run(5, False, 1, odd, s, [s, 0, 0], 2)
    tables.run(2, True, 3, odd, beta, [0, 1, P - 1], 3)
    if tables.n_vars == 13:  # three workgroups stride over 2^12 pairs
        tables.run(5, True, 3, tables.N - 5, beta, g3, 3, grid=3)
        tables.run(4, False, 1, tables.N // 2 + 1, beta, g3, 2, grid=3)


def test_a_rounds_new_weights_in_its_first_launch_equal_the_unfused_sequence(tables):
    """w += the points' equality weights (or, overwriting, = them) with p as it stands, and the round's three sums"""
    from provekit_amd.field import random_field

    beta = E.ints(random_field(1, 912))[0]
    for q in POINTS:
        for overwrite in (False, True):
            tables.run(q, overwrite, 0, 0, beta, [0, 0, 0], 3)
    if tables.n_vars == 13:
        tables.run(113, False, 0, 0, beta, [0, 0, 0], 3, grid=3)


def test_the_hint_without_the_table_equals_eq_table_and_dot(tables):
    """<row k, eq(point, .)> over the rows' leading entries against pk_eq_table and pk_dot per row; point coordinates at p - 1 too"""
    from provekit_amd._lib import lib
    from tools.pk_probes import lib as probes

    ctx, N, n_vars = tables.ctx, tables.N, tables.n_vars
    d_eq = tables.out[0]
    for point in (tables.pts[:n_vars], tables.pts[n_vars: 2 * n_vars]):
        point = np.ascontiguousarray(point)
        ctx.upload_into(d_eq.ptr, tables.junk)
        ctx._check(lib.pk_eq_table(ctx.handle, point.ctypes.data, n_vars, d_eq.ptr))
        for nrows in (1, 3):
            for n in row_lengths(N):
                got = np.full((3, 4), JUNK, dtype=np.uint64)
                ctx._check(probes.pk_probe_dot_rows_eq(ctx.handle, tables.d_rows.ptr, tables.stride, nrows, point.ctypes.data, n_vars, n, got.ctypes.data))
                for k in range(nrows):
                    want = np.zeros(4, dtype=np.uint64)
                    ctx._check(lib.pk_dot(ctx.handle, tables.d_rows.ptr + 32 * k * tables.stride, d_eq.ptr, n, want.ctypes.data))
                    assert np.array_equal(got[k], want), (n_vars, nrows, n, k)
                assert (got[nrows:] == JUNK).all()


def custom_config(n_vars, fold, queries):
    """a WHIR schedule by hand: `fold` variables per round, one round per entry of `queries`, cheap grinding"""
    from provekit_amd.scheme import WhirConfig

    return WhirConfig(n_vars, 2, fold, 1, list(queries), [1] * len(queries), [4.0] * len(queries), 3, 4.0, 1, 0.0)


# (m, m_0, witness length): one entry, an odd length and 2^(m-1) - 5 at both sizes
PROOFS = [(9, 7, 1), (9, 7, 161), (9, 7, (1 << 8) - 5), (12, 9, 1), (12, 9, (1 << 10) + 1), (12, 9, (1 << 11) - 5)]


def prove_both(ctx, oracle, m, m_0, nw, cfg_w, cfg_b):
    import prover_ref as PR
    from test_gpu_commit_fused import instance_of_length
    from test_gpu_prove import _vcfg, to_sparse

    from provekit_amd.scheme import WhirR1CSScheme
    from provekit_amd.sparse_matrix import R1CS

    nc, nw, z, coeffs, trips = instance_of_length(nw, m_0)
    mats = []
    for rows, cols, vals in trips:
        rows = np.array(rows, dtype=np.int64)
        mats.append((np.searchsorted(rows, np.arange(nc)).astype(np.uint32), np.array(cols, dtype=np.uint32), np.array(vals, dtype=np.uint32)))
    interner = oracle.to_mont(oracle.ints_to_limbs(coeffs))
    zm = oracle.to_mont(oracle.ints_to_limbs(z))
    r1cs = R1CS(ctx, *(to_sparse(nc, nw, t) for t in trips), interner)
    scheme = WhirR1CSScheme(ctx, r1cs, m, m_0, cfg_w, cfg_b)
    try:
        want = PR.prove(scheme.domain_separator, m, m_0, _vcfg(cfg_w), _vcfg(cfg_b), (nc, nw, mats, interner), zm, (5).to_bytes(32, "little"))
        got = scheme.prove(ctx.upload(zm), seed=5)
    finally:
        scheme.close()
        r1cs.close()
    assert len(got) == len(want)
    if got != want:
        first = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f"pk_prove's transcript differs from the oracle prover's from byte {first} of {len(got)}")


@pytest.mark.parametrize("m,m_0,nw", PROOFS)
def test_whole_proof_equals_the_oracle_provers(ctx, oracle, m, m_0, nw):
    from provekit_amd.scheme import WhirConfig, blinding_config_for

    prove_both(ctx, oracle, m, m_0, nw, WhirConfig.for_size(m, 4.0), blinding_config_for(m_0, 4.0))


def test_whole_proof_where_a_rounds_table_is_a_single_pair(ctx, oracle):
    """m = 5 at one variable per round and four rounds: the opening's first launch forms 2^5 entries and the rounds' first launches add
    their weights to tables of 16, 8, 4 and, in the last round, 2 entries -- one pair, nhi = 0"""
    from provekit_amd.scheme import blinding_config_for

    prove_both(ctx, oracle, 5, 4, 9, custom_config(5, 1, [6, 5, 4, 3]), blinding_config_for(4, 4.0))
