"""GPU: csrc/r1cs.hip at the places where it changes path -- lines of the largest values at every phase of a reduction group and on
both sides of the heavy threshold and of a chunk, the slot lookup of the pre-summed heavy lines through the six line sets and the
masks of the entry points, the shards of the sharded prover (witness_bounds_strided, external_row_range: reached through the lab,
tools/probes/r1cs.hip), the satisfaction check's first failing row, and degenerate shapes.  The systems are
tests/r1cs_edge_cases.py's (their shape is checked on the host by test_r1cs_edge_cases_host.py); every output is compared bit for
bit with the C oracle's row-by-row sums (oracle.spmv / oracle.hadamard)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import r1cs_edge_cases as E  # noqa: E402

SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def thresholds():
    """the cases straddle these values: a retune of csrc/r1cs_shape.hpp or fe29.hpp must fail here, not quietly un-aim them"""
    from tools.pk_probes import r1cs_thresholds

    th = r1cs_thresholds()
    assert (th["HEAVY_DEGREE"], th["HEAVY_CHUNK"], th["DOT29_GROUP"]) == (64, 2048, 4) and th == E.THRESHOLDS


def _sentinel(ctx, n):
    """n elements no kernel output equals: what a call leaves untouched shows"""
    return ctx.upload(np.full((max(int(n), 1), 4), SENTINEL, np.uint64))


class _Loaded:
    """a case on the device with the oracle's products: rows[k] = M_k z, cols[k] = eq^T M_k, c = (A z) o (B z), the first failing row"""

    def __init__(self, ctx, oracle, case):
        from provekit_amd.sparse_matrix import R1CS

        self.ctx, self.case = ctx, case
        nc, nw = case.nc, case.nw
        sp = lambda m, x, t: oracle.spmv(nc, nw, m.new_row_indices, m.col_indices, m.values, case.interner, x, transpose=t)  # noqa: E731
        self.rows = [sp(m, case.z, False) for m in case.mats]
        self.cols = [sp(m, case.eq[:nc], True) for m in case.mats]
        self.c = oracle.hadamard(self.rows[0], self.rows[1])
        self.first_bad = self.first_failing(oracle, case.z)
        self.r = R1CS(ctx, *case.mats, case.interner)
        self.d_z, self.d_eq = ctx.upload(case.z), ctx.upload(case.eq)

    def first_failing(self, oracle, z):
        case = self.case
        a, b, c = (oracle.spmv(case.nc, case.nw, m.new_row_indices, m.col_indices, m.values, case.interner, z) for m in case.mats)
        bad = np.nonzero((oracle.hadamard(a, b) != c).any(axis=1))[0]
        return int(bad[0]) if len(bad) else -1

    def close(self):
        self.r.close()

    # the entry points, each on outputs prefilled with the sentinel
    def bounds(self):
        ctx, case = self.ctx, self.case
        n = 1 << case.m0
        from provekit_amd._lib import lib

        bufs = [_sentinel(ctx, n) for _ in range(3)]
        ctx._check(lib.pk_r1cs_witness_bounds(ctx.handle, self.r.handle, self.d_z.ptr, case.m0, *[b.ptr for b in bufs]))
        pad = np.zeros((n - case.nc, 4), np.uint64)
        for name, buf, want in zip("abc", bufs, (self.rows[0], self.rows[1], self.c)):
            assert np.array_equal(ctx.download_fe(buf, n), np.concatenate([want, pad])), f"{case.name}: witness bounds {name}"

    def external(self):
        ctx, case = self.ctx, self.case
        from provekit_amd._lib import lib

        out = _sentinel(ctx, 3 * case.nw)
        ctx._check(lib.pk_r1cs_external_row(ctx.handle, self.r.handle, self.d_eq.ptr, out.ptr))
        got = ctx.download_fe(out, 3 * case.nw).reshape(3, case.nw, 4)
        for k in range(3):
            assert np.array_equal(got[k], self.cols[k]), f"{case.name}: external row of {'ABC'[k]}"

    def matvec(self, k, transpose):
        ctx, case = self.ctx, self.case
        from provekit_amd._lib import lib

        n = case.nw if transpose else case.nc
        out = _sentinel(ctx, n)
        ctx._check(lib.pk_r1cs_matvec(ctx.handle, self.r.handle, k, int(transpose), (self.d_eq if transpose else self.d_z).ptr, out.ptr))
        assert np.array_equal(ctx.download_fe(out, n), (self.cols if transpose else self.rows)[k]), f"{case.name}: matvec {'ABC'[k]} transpose={transpose}"

    def satisfaction(self, d_z=None, want=None):
        from provekit_amd import ProveKitHipError

        want = self.first_bad if want is None else want
        d_z = self.d_z if d_z is None else d_z
        if want < 0:
            self.r.test_witness_satisfaction(d_z)  # raises unless PK_OK
            return
        with pytest.raises(ProveKitHipError, match=f"Constraint {want} failed") as e:
            self.r.test_witness_satisfaction(d_z)
        assert e.value.code == -6 and e.value.row == want, self.case.name

    def entry_points(self):
        return [self.bounds, self.external] + [(lambda k=k, t=t: self.matvec(k, t)) for t in (False, True) for k in range(3)] + [self.satisfaction]


@pytest.mark.parametrize("name", list(E.PM1_CASES))
def test_lines_of_the_largest_values(ctx, oracle, name):
    """1. interner {p - 1, 0, R}, z and eq all p - 1, one line of each length 0..9, 63, 64, 65, 2047, 2048, 2049, 4097 and
    RED_THREADS -+ 1, 2 RED_THREADS -+ 1 in one line set (rows or columns of A, B or C): t (p-1)^2 / 2^256 in Python integers ==
    the oracle == witness bounds, external rows and the six single-matrix products"""
    case = E.PM1_CASES[name]()
    L = _Loaded(ctx, oracle, case)
    s = case.expect["set"]
    want = np.zeros(((case.nw if s >= 3 else case.nc), 4), np.uint64)
    for i, t in case.expect["lengths"].items():
        want[i] = E.limbs([E.pm1_value(t)])[0]
    assert np.array_equal((L.cols if s >= 3 else L.rows)[s % 3], want)  # the oracle is the Python integers' sum
    for call in L.entry_points():
        call()
    L.close()


@pytest.mark.parametrize("name", list(E.SLOT_CASES))
def test_heavy_lines_are_found_in_their_slots(ctx, oracle, name):
    """2. one heavy line; the first row only; the last row and column only; every row; heavy rows in A, in B, in C only; heavy columns
    in C only; heavy rows of A with heavy columns of C and nothing between; 64 entries next to 65.  Every entry point (each sums the
    heavy lines of its own sets only: rows of A and B; the three column sets; one set; the three row sets), then all of them again in
    the opposite order on the same context, so that each call finds the workspace as another one left it.  The heavy lines' sums
    differ pairwise (host test): a sum read from a neighbouring slot, or from a slot this call did not fill, is a wrong output"""
    case = E.SLOT_CASES[name]()
    L = _Loaded(ctx, oracle, case)
    calls = L.entry_points()
    for call in calls:
        call()
    for call in reversed(calls):
        call()
    L.close()


@pytest.mark.parametrize("nc", E.STRIDED_NCS)
def test_strided_witness_bounds(ctx, oracle, nc):
    """3. witness_bounds_strided(stride, offset) for stride 1, 2, 4, 8, 16 and every offset below it, m0 minimal and minimal + 2
    (workgroups of pure padding), on a system with heavy rows in A and B: output j is the oracle's row j * stride + offset, zero past
    the constraints, for a, b and c; nothing is written past 2^m0 / stride outputs; a shard without outputs (stride > 2^m0) is
    PK_OK and writes nothing"""
    from tools.pk_probes import lib as probes

    case = E.strided_case(nc)
    L = _Loaded(ctx, oracle, case)
    for m0 in (case.m0, case.m0 + 2):
        n = 1 << m0
        full = [np.concatenate([w, np.zeros((n - nc, 4), np.uint64)]) for w in (L.rows[0], L.rows[1], L.c)]
        for stride in E.STRIDES:
            padded = n // stride
            for offset in range(stride):
                bufs = [_sentinel(ctx, padded + 1) for _ in range(3)]
                rc = probes.pk_probe_r1cs_witness_bounds_strided(ctx.handle, L.r.handle, L.d_z.ptr, m0, stride, offset, *[b.ptr for b in bufs])
                assert rc == 0, (m0, stride, offset, ctx.last_error())
                idx = np.arange(padded) * stride + offset
                for name, buf, want in zip("abc", bufs, full):
                    got = ctx.download_fe(buf, padded + 1)
                    assert np.array_equal(got[:padded], want[idx]), f"nc={nc} m0={m0} stride={stride} offset={offset}: {name}"
                    assert (got[padded] == SENTINEL).all(), f"nc={nc} m0={m0} stride={stride} offset={offset}: {name} written past its end"
    # shards that do not exist, a table too small for the constraints
    bufs = [_sentinel(ctx, 1 << (case.m0 + 1)) for _ in range(3)]
    for m0, stride, offset in ((case.m0, 0, 0), (case.m0, 1, 1), (case.m0, 4, 4), (case.m0, 16, 17)) + (((case.m0 - 1, 1, 0),) if case.m0 else ()):
        assert probes.pk_probe_r1cs_witness_bounds_strided(ctx.handle, L.r.handle, L.d_z.ptr, m0, stride, offset, *[b.ptr for b in bufs]) == -1
    for buf in bufs:
        assert (ctx.download_fe(buf, 1 << (case.m0 + 1)) == SENTINEL).all()
    L.close()


def test_external_row_ranges(ctx, oracle):
    """4. external_row_range(first, last) on a system with heavy columns at both ends, around 256 and 512 and at the seams of four
    equal blocks: inside [first, min(last, num_witnesses)) the three planes are the oracle's, outside every byte is still the
    sentinel the output was filled with; empty ranges write nothing; the four blocks together are the whole"""
    from tools.pk_probes import lib as probes

    case = E.range_case()
    nw = case.nw
    assert nw % 4 == 0 and nw > 512 and (nw // 4) % 256 != 0
    L = _Loaded(ctx, oracle, case)
    whole = np.stack(L.cols)

    def run(out, first, last):
        rc = probes.pk_probe_r1cs_external_row_range(ctx.handle, L.r.handle, L.d_eq.ptr, first, last, out.ptr)
        assert rc == 0, (first, last, ctx.last_error())

    for first, last in E.ranges(nw):
        out = _sentinel(ctx, 3 * nw + 1)
        run(out, first, last)
        got = ctx.download_fe(out, 3 * nw + 1)
        want = np.full((3, nw, 4), SENTINEL, np.uint64)
        want[:, first : min(last, nw)] = whole[:, first : min(last, nw)]
        assert np.array_equal(got[: 3 * nw].reshape(3, nw, 4), want), (first, last)
        assert (got[3 * nw] == SENTINEL).all(), (first, last)
    out = _sentinel(ctx, 3 * nw)
    for q in range(4):
        run(out, q * nw // 4, (q + 1) * nw // 4)
    assert np.array_equal(ctx.download_fe(out, 3 * nw).reshape(3, nw, 4), whole)
    L.close()


def test_satisfaction_names_the_first_failing_row(ctx, oracle):
    """5. a satisfied system with heavy rows in A, B and C is PK_OK with row -1; one changed witness breaks exactly its row -- row 0,
    255 (the last lane of a workgroup), 256, the last row, a heavy row of C (through its output and through an input only that heavy
    line reads), a row whose only heavy matrix is A (through an input only that line reads); of failures in different workgroups the
    lowest row is named; a wrong witness count is PK_ERR_BAD_ARG; a satisfied witness right after a failing one is row -1 again"""
    from provekit_amd import ProveKitHipError

    case = E.satisfiable_case()
    L = _Loaded(ctx, oracle, case)
    x, nc, n_in = case.expect, case.nc, case.expect["n_in"]
    assert L.first_bad == -1 and nc == 600
    L.satisfaction(want=-1)
    singles = [(n_in + i, i) for i in (0, 255, 256, nc - 1, x["heavy_c_row"])] + [x["priv_c"], x["priv_a"]]
    assert x["priv_a"][1] == x["only_a_heavy_row"] and x["priv_c"][1] in case.heavy[2] and x["heavy_c_row"] in case.heavy[2]
    assert x["only_a_heavy_row"] in case.heavy[0] and x["only_a_heavy_row"] not in case.heavy[1] and x["only_a_heavy_row"] not in case.heavy[2]
    for column, row in singles:
        z = E.corrupt(case.z, column)
        assert L.first_failing(oracle, z) == row
        L.satisfaction(ctx.upload(z), want=row)
        L.satisfaction(want=-1)  # no failure carries over
    for rows in ((300, 40), (40, 300), (599, 300, 40), (511, 512), (256, 255)):
        z = case.z
        for i in rows:
            z = E.corrupt(z, n_in + i)
        L.satisfaction(ctx.upload(z), want=min(rows))
    for n in (case.nw - 1, case.nw + 1, 0):
        with pytest.raises(ProveKitHipError) as e:
            L.r.test_witness_satisfaction(L.d_z, n_witness=n)
        assert e.value.code == -1
    L.satisfaction(want=-1)
    L.close()


@pytest.mark.parametrize("name", list(E.DEGENERATE_CASES))
def test_degenerate_shapes(ctx, oracle, name):
    """6. three matrices without entries (zero outputs everywhere, satisfied); no constraints but witnesses (the external rows are
    zero, the padded table is one zero); no interned values and no entries; one constraint with m0 = 0 (a heavy row of B in it)"""
    case = E.DEGENERATE_CASES[name]()
    L = _Loaded(ctx, oracle, case)
    if name != "one_row_m0_zero":
        assert not any(w.any() for w in L.rows + L.cols) and L.first_bad == -1
    else:
        assert case.m0 == 0 and case.heavy == {1: {0: 65}}
    for call in L.entry_points():
        call()
    L.close()
