"""LogUp lookup arguments over device tables (libprovekit_lookup.so, include/provekit_lookup.h): prove that every entry of a column f
of 2^n values occurs in a table t of 2^k values, and verify such a proof on the host.

An accepted proof is accepted PROVIDED the seven evaluation claims of `Claims` hold: whir_pcs.Scheme.open / whir_pcs.verify establish
them for committed tables (f and h_f at r_f, t, m and h_t at r_t, h_f and h_t at the all-halves points).

A sixth library above the product's C ABI, with its own loader and one signature table (as provekit_amd.prodcheck, whose library it
links).  `verify`, `io_pattern`, `proof_bytes` and `arena_bytes` are host only; `LookupProver` needs a Context.  A rejected proof is a
Result, not an exception; only a failed CALL raises.  There is no fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import prodcheck  # loads libprovekit_sumcheck.so, which this library links
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import CHECKS, _fe, _ptr
from .runtime import Context, DeviceBuffer
from .verify import Result, ResultStruct

LOOKUP_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_lookup.so")
MAX_VARS, MAX_BIND, MAX_GRID = 28, 16, 1024
SIDES = ("OUTER", "F", "T")
LABEL = b"provekit-hip/lookup/v1"
ERR_UNSATISFIED = -6
NO_BAD = (1 << 64) - 1


class StatementStruct(C.Structure):
    """pkl_statement"""

    _fields_ = [("n", C.c_uint), ("k", C.c_uint), ("n_bind", C.c_uint), ("n_bind2", C.c_uint)]


class ClaimsStruct(C.Structure):
    """pkl_claims"""

    _fields_ = [("alpha", C.c_uint64 * 4), ("s", C.c_uint64 * 4), ("r_f", (C.c_uint64 * 4) * MAX_VARS), ("r_t", (C.c_uint64 * 4) * MAX_VARS),
                ("hf_at_rf", C.c_uint64 * 4), ("f_at_rf", C.c_uint64 * 4), ("ht_at_rt", C.c_uint64 * 4), ("t_at_rt", C.c_uint64 * 4),
                ("m_at_rt", C.c_uint64 * 4), ("hf_at_half", C.c_uint64 * 4), ("ht_at_half", C.c_uint64 * 4)]


# name -> (restype, argtypes); kept in the same order as include/provekit_lookup.h
SIGNATURES = {
    "pkl_abi_version": (C.c_int, []),
    "pkl_create_error": (C.c_char_p, []),
    "pkl_io_pattern": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
    "pkl_proof_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkl_prover_arena_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "pkl_count_lds_max_k": (C.c_uint, []),
    "pkl_gather_lds_max_k": (C.c_uint, []),
    "pkl_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkl_prover_destroy": (C.c_int, [vp]),
    "pkl_last_error": (C.c_char_p, [vp]),
    "pkl_multiplicities": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "pkl_begin": (C.c_int, [vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]),
    "pkl_finish": (C.c_int, [vp, vp, vp, sz, C.POINTER(sz), vp]),
    "pkl_verify": (C.c_int, [vp, vp, sz, vp, vp, vp, sz, vp, C.POINTER(C.c_int), C.POINTER(ResultStruct)]),
}


def _load():
    if not os.path.exists(LOOKUP_LIB_PATH):
        raise ImportError(
            f"{LOOKUP_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(LOOKUP_LIB_PATH)  # its libprovekit_sumcheck.so and libprovekit_hip.so are the ones already loaded (same files, next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def gather_lds_max_k() -> int:
    """the largest k whose source tables the gather stages in LDS"""
    return int(lib.pkl_gather_lds_max_k())


class Statement:
    """a column of 2^n values against a table of 2^k; n_bind elements are absorbed before alpha, n_bind2 after the helper tables exist"""

    def __init__(self, n: int, k: int, n_bind: int = 0, n_bind2: int = 0):
        self.n, self.k, self.n_bind, self.n_bind2 = n, k, n_bind, n_bind2

    def struct(self) -> StatementStruct:
        return StatementStruct(self.n, self.k, self.n_bind, self.n_bind2)


class Claims:
    """what an accepted proof is accepted PROVIDED of, Montgomery [.., 4] uint64: alpha, s, the points r_f [n, 4] and r_t [k, 4], and the
    seven values hf_at_rf, f_at_rf, ht_at_rt, t_at_rt, m_at_rt, hf_at_half, ht_at_half"""

    VALUES = ("hf_at_rf", "f_at_rf", "ht_at_rt", "t_at_rt", "m_at_rt", "hf_at_half", "ht_at_half")

    def __init__(self, stmt: Statement, c: ClaimsStruct):
        self.alpha, self.s = np.array(c.alpha, dtype=np.uint64), np.array(c.s, dtype=np.uint64)
        self.r_f = np.array([list(c.r_f[i]) for i in range(stmt.n)], dtype=np.uint64)
        self.r_t = np.array([list(c.r_t[i]) for i in range(stmt.k)], dtype=np.uint64)
        for name in self.VALUES:
            setattr(self, name, np.array(getattr(c, name), dtype=np.uint64))


def _refused(rc: int):
    raise ProveKitHipError(rc, lib.pkl_create_error().decode())


def io_pattern(stmt: Statement) -> bytes:
    """the spongefish operation list (domain separator) of the outer transcript (pkl_io_pattern; host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pkl_io_pattern(C.addressof(s), None, 0, C.byref(n))
    if rc:
        _refused(rc)
    buf = (C.c_uint8 * n.value)()
    lib.pkl_io_pattern(C.addressof(s), buf, n.value, C.byref(n))
    return bytes(buf)


def proof_bytes(stmt: Statement) -> int:
    s = stmt.struct()
    n = sz()
    rc = lib.pkl_proof_bytes(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def arena_bytes(stmt: Statement) -> int:
    """the device memory a LookupProver of this statement holds, its two sumcheck provers included (host only)"""
    s = stmt.struct()
    n = sz()
    rc = lib.pkl_prover_arena_bytes(C.addressof(s), C.byref(n))
    if rc:
        _refused(rc)
    return n.value


def count_lds_max_k() -> int:
    """the largest k whose multiplicities are counted in LDS"""
    return int(lib.pkl_count_lds_max_k())


def verify(stmt: Statement, proof: bytes, bind=None, bind2=None, io_pattern: bytes | None = None):
    """(Result, side, Claims or None): side is "OUTER", "F" or "T"; the claims are given when the proof is accepted, and accepted means
    accepted provided they hold (pkl_verify; host only)"""
    s = stmt.struct()
    bind_a = _fe(bind, stmt.n_bind, "bind") if (bind is not None or stmt.n_bind) else None
    bind2_a = _fe(bind2, stmt.n_bind2, "bind2") if (bind2 is not None or stmt.n_bind2) else None
    claims, r, side = ClaimsStruct(), ResultStruct(), C.c_int(0)
    pat = (C.c_uint8 * len(io_pattern)).from_buffer_copy(io_pattern) if io_pattern else None
    pbuf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(bytes(proof) or b"\0")
    rc = lib.pkl_verify(C.addressof(s), C.cast(pat, vp) if pat is not None else None, len(io_pattern) if io_pattern else 0, _ptr(bind_a), _ptr(bind2_a),
                        C.cast(pbuf, vp), len(proof), C.addressof(claims), C.byref(side), C.byref(r))
    if rc:
        _refused(rc)
    res = Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))
    return res, SIDES[side.value], Claims(stmt, claims) if res.accepted else None


def _dev(buf) -> int:
    return buf.ptr if isinstance(buf, DeviceBuffer) else int(buf)


class LookupProver:
    """one statement's prover on a context: owns one device arena and two sumcheck provers, made at creation; a proof allocates no
    device memory and never writes the caller's f, t or idx.  The steps of a proof: multiplicities() -> commit f, t, m -> begin() ->
    commit h_f, h_t -> finish()."""

    def __init__(self, ctx: Context, stmt: Statement):
        self.ctx, self.stmt = ctx, stmt
        s = stmt.struct()
        h = vp()
        rc = lib.pkl_prover_create(ctx.handle, C.addressof(s), C.byref(h))
        if rc:
            _refused(rc)
        self.handle = h
        self.proof_bytes = proof_bytes(stmt)
        self.first_bad = None

    def close(self):
        if getattr(self, "handle", None):
            lib.pkl_prover_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return lib.pkl_last_error(self.handle).decode()

    def _check(self, rc: int):
        if rc:
            raise ProveKitHipError(rc, self.last_error())

    def multiplicities(self, d_f, d_t, d_idx, d_m_out):
        """step 1: validates every lookup and writes m (2^k elements) to d_m_out, which stays valid and unchanged until finish().  A failed
        validation raises with code -6 (PK_ERR_UNSATISFIED) and leaves the smallest bad x in self.first_bad"""
        bad = C.c_uint64(0)
        rc = lib.pkl_multiplicities(self.handle, _dev(d_f), _dev(d_t), _dev(d_idx), _dev(d_m_out), C.byref(bad))
        self.first_bad = None if bad.value == NO_BAD else bad.value
        self._check(rc)

    def begin(self, d_t, d_idx, bind=None):
        """steps 2 and 3 -> (alpha [4], device address of h_f, device address of h_t): the two helper tables to commit, in the prover's
        arena, valid until the next begin()"""
        bind_a = _fe(bind, self.stmt.n_bind, "bind") if (bind is not None or self.stmt.n_bind) else None
        alpha = np.zeros(4, dtype=np.uint64)
        hf, ht = vp(), vp()
        self._check(lib.pkl_begin(self.handle, _dev(d_t), _dev(d_idx), _ptr(bind_a), alpha.ctypes.data, C.byref(hf), C.byref(ht)))
        return alpha, hf.value, ht.value

    def finish(self, bind2=None, capacity: int | None = None):
        """steps 4 and 5 -> (proof bytes, Claims)"""
        bind2_a = _fe(bind2, self.stmt.n_bind2, "bind2") if (bind2 is not None or self.stmt.n_bind2) else None
        cap = self.proof_bytes if capacity is None else capacity
        buf = (C.c_uint8 * max(cap, 1))()
        n = sz()
        claims = ClaimsStruct()
        rc = lib.pkl_finish(self.handle, _ptr(bind2_a), C.cast(buf, vp), cap, C.byref(n), C.addressof(claims))
        self.last_len = n.value
        self._check(rc)
        return bytes(buf[: n.value]), Claims(self.stmt, claims)
