"""Sparse-matrix evaluation proofs over device tables (libprovekit_spark.so, include/provekit_spark.h): commit once to a sparse matrix
as dense columns, then prove M~(rx, ry) = v with one product sumcheck and two ROM lookups into eq tables (Spark), and verify such proofs
on the host in O(log).  `Prover.matrix` builds the committed columns row, col, m_row, m_col from the entries' indices on the device,
`Prover.begin` gathers the per-query columns e_row, e_col.

An accepted proof is accepted PROVIDED the nine values of `Claims`: whir_pcs.Scheme.open / whir_pcs.verify give the columns'
evaluations at z_val, z_f and z_m, `check_claims` forms the combinations.

An eleventh library above the product's C ABI, with its own loader and one signature table (as provekit_amd.memcheck).  `verify`,
`check_claims`, `entries_from_r1cs`, the pattern and the lengths are host only; the prover needs a Context.  A rejected proof is a
Result, not an exception; only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import tuplelookup  # loads libprovekit_tuplelookup.so (and the libraries under it), which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

SPARK_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_spark.so")
MAX_VARS, MAX_BIND, MAX_GRID = 28, 16, 1024
CHECKS = tuplelookup.CHECKS + ("TABLE",)
SIDES = ("VAL", "ROW", "COL")
WHICH = ("NONE", "VAL", "E_ROW", "E_COL", "ROW", "M_ROW", "COL", "M_COL")  # check_claims
COLUMNS = ("row", "col", "val", "m_row", "m_col", "e_row", "e_col")  # pkx_prove's order
LABEL = b"provekit-hip/spark/v1"
ERR_BAD_ARG, ERR_UNSATISFIED = -1, -6
NO_BAD_ENTRY = 2**64 - 1


class StatementStruct(C.Structure):
    """pkx_statement"""

    _fields_ = [("n", C.c_uint), ("s", C.c_uint), ("t", C.c_uint), ("n_bind", C.c_uint)]


class ClaimsStruct(C.Structure):
    """pkx_claims"""

    _fields_ = [("value", C.c_uint64 * 4), ("z_val", (C.c_uint64 * 4) * MAX_VARS), ("val_values", (C.c_uint64 * 4) * 3), ("beta", (C.c_uint64 * 4) * 2),
                ("z_f", ((C.c_uint64 * 4) * MAX_VARS) * 2), ("f_coeff", ((C.c_uint64 * 4) * 2) * 2), ("f_value", (C.c_uint64 * 4) * 2),
                ("z_m", ((C.c_uint64 * 4) * MAX_VARS) * 2), ("m_value", (C.c_uint64 * 4) * 2)]


class SparseMatrixStruct(C.Structure):
    """pk_sparse_matrix"""

    _fields_ = [("new_row_indices", vp), ("col_indices", vp), ("values", vp), ("nnz", sz)]


# name -> (restype, argtypes); kept in the same order as include/provekit_spark.h
SIGNATURES = {
    "pkx_abi_version": (C.c_int, []),
    "pkx_check_name": (C.c_char_p, [C.c_int]),
    "pkx_create_error": (C.c_char_p, []),
    "pkx_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkx_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkx_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkx_count_lds_max": (C.c_uint, []),
    "pkx_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkx_prover_destroy": (C.c_int, [vp]),
    "pkx_last_error": (C.c_char_p, [vp]),
    "pkx_matrix": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "pkx_begin": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "pkx_prove": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp, vp]),
    "pkx_verify": (C.c_int, [vp, vp, sz, vp, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(ResultStruct)]),
    "pkx_check_claims": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]),
    "pkx_entries_from_r1cs": (C.c_int, [sz, sz, vp, vp, sz, C.c_uint, C.c_uint, C.c_uint, vp, vp, vp]),
}


def _load():
    if not os.path.exists(SPARK_LIB_PATH):
        raise ImportError(
            f"{SPARK_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(SPARK_LIB_PATH)  # the libraries it links are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Statement:
    """2^n entries of a matrix of 2^s rows and 2^t columns; n_bind caller elements (the roots) are absorbed first"""

    def __init__(self, n: int, s: int, t: int, n_bind: int = 0):
        self.n, self.s, self.t, self.n_bind = n, s, t, n_bind

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.s, self.t, self.n_bind)


class Claims:
    """what an accepted proof is accepted PROVIDED of, Montgomery [.., 4] uint64: value [4]; z_val [n, 4] with val_values [3, 4] (val,
    e_row, e_col there); and per side ROW, COL: beta, z_f [n, 4], f_coeff [2, 4] = (1, beta), f_value, z_m [s or t, 4], m_value"""

    def __init__(self, stmt: Statement, c: ClaimsStruct):
        self.struct = c
        a = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
        self.value = a(c.value)
        self.z_val = a([list(c.z_val[i]) for i in range(stmt.n)])
        self.val_values = a([list(c.val_values[j]) for j in range(3)])
        self.beta = [a(c.beta[side]) for side in range(2)]
        self.z_f = [a([list(c.z_f[side][i]) for i in range(stmt.n)]) for side in range(2)]
        self.f_coeff = [a([list(c.f_coeff[side][j]) for j in range(2)]) for side in range(2)]
        self.f_value = [a(c.f_value[side]) for side in range(2)]
        self.z_m = [a([list(c.z_m[side][i]) for i in range((stmt.s, stmt.t)[side])]) for side in range(2)]
        self.m_value = [a(c.m_value[side]) for side in range(2)]


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkx_create_error().decode())


def _sized(call, stmt) -> int:
    s = stmt.struct()
    n = sz()
    rc = call(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of the outer transcript (host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pkx_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pkx_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    return _sized(lib.pkx_proof_bytes, stmt)


def arena_bytes(stmt: Statement) -> int:
    """the device memory a prover of this statement holds, its three inner provers included (host only)"""
    return _sized(lib.pkx_prover_arena_bytes, stmt)


def count_lds_max() -> int:
    return int(lib.pkx_count_lds_max())


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _bytes_arg(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def verify(stmt: Statement, proof: bytes, rx, ry, bind=None, expected_value=None, io_pattern: bytes | None = None):
    """(Result, side, layer, Claims or None): side is "VAL", "ROW" or "COL"; rx [s, 4], ry [t, 4], expected_value [4] or None, Montgomery
    (pkx_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    rx_a, ry_a = _fe(rx, stmt.s, "rx"), _fe(ry, stmt.t, "ry")
    want = _fe(expected_value, 1, "expected_value") if expected_value is not None else None
    claims, r, side, layer = ClaimsStruct(), ResultStruct(), C.c_int(0), C.c_uint(0)
    pat = _bytes_arg(io_pattern) if io_pattern else None
    pbuf = _bytes_arg(proof)
    rc = lib.pkx_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(rx_a), _ptr(ry_a), _ptr(bind_a),
                        _ptr(want), C.cast(pbuf, vp), len(proof), C.addressof(claims), C.byref(side), C.byref(layer), C.byref(r))
    if rc:
        _refused(rc)
    res = _result(r)
    return res, SIDES[side.value], layer.value, Claims(stmt, claims) if res.accepted else None


def check_claims(stmt: Statement, claims: Claims, val_evals, row_evals, m_row_eval, col_evals, m_col_eval) -> str:
    """val_evals [3, 4] = (val, e_row, e_col)(z_val), row_evals [2, 4] = (row, e_row)(z_f[0]), m_row_eval [4] = m_row(z_m[0]), col_evals
    [2, 4] = (col, e_col)(z_f[1]), m_col_eval [4] = m_col(z_m[1]), Montgomery -> "NONE" when all hold, else the first that does not, in
    WHICH's order (pkx_check_claims; host only)"""
    s = stmt.struct()
    arrs = [_fe(np.asarray(v, dtype=np.uint64).reshape(-1, 4), rows, what) for v, rows, what in
            ((val_evals, 3, "val_evals"), (row_evals, 2, "row_evals"), (m_row_eval, 1, "m_row_eval"), (col_evals, 2, "col_evals"), (m_col_eval, 1, "m_col_eval"))]
    which = C.c_int(-1)
    rc = lib.pkx_check_claims(C.addressof(s), C.addressof(claims.struct), *[_ptr(a) for a in arrs], C.byref(which))
    if rc:
        _refused(rc)
    return WHICH[which.value]


def entries_from_r1cs(num_constraints: int, num_witnesses: int, mats, interner, n: int, s: int, t: int):
    """mats: three (new_row_indices, col_indices, values) triples of uint32 arrays (CSR, values indexing the interner); interner
    [k, 4] Montgomery -> (row_idx [2^n] uint32, col_idx [2^n] uint32, val [2^n, 4]): the one stacked entry list of the statement
    (n, s + 2, t), stacked row = matrix 2^s + row (pkx_entries_from_r1cs; host only)"""
    keep, structs = [], (SparseMatrixStruct * 3)()
    for g, (rows, cols, vals) in enumerate(mats):
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (rows, cols, vals)]
        keep.append(arrs)
        structs[g] = SparseMatrixStruct(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, len(arrs[1]))
    table = np.ascontiguousarray(interner, dtype=np.uint64).reshape(-1, 4)
    size = 1 << n if 0 <= n <= MAX_VARS else 1
    row_idx, col_idx, val = np.zeros(size, dtype=np.uint32), np.zeros(size, dtype=np.uint32), np.zeros((size, 4), dtype=np.uint64)
    rc = lib.pkx_entries_from_r1cs(num_constraints, num_witnesses, C.addressof(structs), table.ctypes.data, table.shape[0], n, s, t, row_idx.ctypes.data,
                                   col_idx.ctypes.data, val.ctypes.data)
    if rc:
        _refused(rc)
    return row_idx, col_idx, val


def _dev(buf):
    return None if buf is None else buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


class Prover:
    """one statement's prover on a context: owns the two eq tables, the index column, the counts and the three inner provers, made at
    creation; a proof allocates no device memory and never writes the caller's tables"""

    fill = None  # a byte the proof buffer (`buffer`) is filled with before a proof, to see afterwards what a refused call wrote: nothing

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkx_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)
        self.first_bad = NO_BAD_ENTRY

    def close(self):
        if getattr(self, "handle", None):
            lib.pkx_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pkx_last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())

    def matrix(self, d_row_idx, d_col_idx, d_row, d_col, d_m_row, d_m_col) -> None:
        """d_row_idx, d_col_idx: 2^n uint32 -> the caller's tables row, col (2^n elements), m_row (2^s), m_col (2^t).  An index outside
        the matrix raises with code -1 (PK_ERR_BAD_ARG), `first_bad` is the smallest such entry (NO_BAD_ENTRY otherwise) and nothing is
        written"""
        bad = C.c_uint64(0)
        rc = lib.pkx_matrix(self.handle, _dev(d_row_idx), _dev(d_col_idx), _dev(d_row), _dev(d_col), _dev(d_m_row), _dev(d_m_col), C.byref(bad))
        self.first_bad = bad.value
        self._check(rc)

    def begin(self, d_row_idx, d_col_idx, rx, ry, d_e_row, d_e_col) -> None:
        """the per-query columns e_row[k] = eq(rx, row_idx[k]), e_col[k] = eq(ry, col_idx[k]); the indices are validated as `matrix` does"""
        rx_a, ry_a = _fe(rx, self.stmt.s, "rx"), _fe(ry, self.stmt.t, "ry")
        bad = C.c_uint64(0)
        rc = lib.pkx_begin(self.handle, _dev(d_row_idx), _dev(d_col_idx), _ptr(rx_a), _ptr(ry_a), _dev(d_e_row), _dev(d_e_col), C.byref(bad))
        self.first_bad = bad.value
        self._check(rc)

    def prove(self, cols, rx, ry, bind=None, capacity: int | None = None):
        """cols: a dict of the seven device columns (COLUMNS) -> (proof bytes, value [4], Claims).  Columns that are not a read of the eq
        tables raise with code -6 (PK_ERR_UNSATISFIED) and a reason that names the side; nothing is written then and the prover stays
        usable"""
        st = self.stmt
        bind_a = _fe(bind, st.n_bind, "bind") if (bind is not None or st.n_bind) else None
        rx_a, ry_a = _fe(rx, st.s, "rx"), _fe(ry, st.t, "ry")
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        if self.fill is not None:
            C.memset(buf, self.fill, max(cap, 1))
        self.buffer = buf
        n = sz()
        claims, value = ClaimsStruct(), np.zeros(4, dtype=np.uint64)
        ptrs = (vp * len(COLUMNS))(*[_dev(cols[name]) for name in COLUMNS])
        rc = lib.pkx_prove(self.handle, C.cast(ptrs, vp), _ptr(rx_a), _ptr(ry_a), _ptr(bind_a), C.cast(buf, vp), cap, C.byref(n), value.ctypes.data, C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), value, Claims(st, claims)
