"""Verifier: WhirR1CSVerifier::verify for the proofs pk_prove writes (libprovekit_verify.so, include/provekit_verify.h).

A third library above the product's C ABI.  `verify(proof)` is the host core (one thread, no device); `verify_many(proofs)`
needs an attached Context and runs the Merkle openings and the R1CS matrix evaluations of the whole batch on the GPU.  Both
return Result objects: "rejected" is a verdict, not an exception; only a failed CALL raises.  This module has its own loader
and signature table (provekit_amd._lib's table is the product header's, nothing else).  There is no fallback: without the built
library the import raises, and verify_many without a device raises."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from ._lib import ProveKitHipError, SparseMatrixStruct, sz, vp
from .scheme import WhirConfig, _cfg_struct
from .sparse_matrix import SparseMatrix

VERIFY_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libprovekit_verify.so")

CHECKS = ("NONE", "TRANSCRIPT_SHORT", "NON_CANONICAL", "IO_PATTERN", "HINT_FORMAT", "OPENING_COUNT", "MERKLE", "ZK_SUMCHECK", "WHIR_SUMCHECK", "POW",
          "STIR_INDICES", "FINAL_POLY", "WHIR_FINAL", "BLINDING_WEIGHT", "TRAILING_BYTES", "SPARTAN", "WITNESS_FIT", "MATRIX_EVAL")


class ResultStruct(C.Structure):
    """pkv_result"""

    _fields_ = [("accepted", C.c_int), ("check", C.c_int), ("offset", C.c_uint64), ("message", C.c_char * 160)]


# name -> (restype, argtypes); kept in the same order as include/provekit_verify.h
SIGNATURES = {
    "pkv_abi_version": (C.c_int, []),
    "pkv_check_name": (C.c_char_p, [C.c_int]),
    "pkv_verifier_create": (C.c_int, [C.c_uint, C.c_uint, vp, vp, vp, sz, C.c_int, C.POINTER(vp)]),
    "pkv_create_error": (C.c_char_p, []),
    "pkv_verifier_destroy": (C.c_int, [vp]),
    "pkv_last_error": (C.c_char_p, [vp]),
    "pkv_verifier_set_r1cs": (C.c_int, [vp, sz, sz, vp, vp, sz]),
    "pkv_verify": (C.c_int, [vp, vp, sz, C.POINTER(ResultStruct)]),
    "pkv_verifier_attach_device": (C.c_int, [vp, vp]),
    "pkv_verify_many": (C.c_int, [vp, vp, vp, sz, vp]),
    "pkv_openings_check": (C.c_int, [vp, C.c_int, vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp]),
    "pkv_matrix_evaluations": (C.c_int, [vp, vp, vp, sz, vp]),
}


def _load():
    if not os.path.exists(VERIFY_LIB_PATH):
        raise ImportError(
            f"{VERIFY_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C provekit_amd/csrc`). provekit_amd has no CPU fallback."
        )
    return C.CDLL(VERIFY_LIB_PATH)  # its libprovekit_hip.so is the one _lib has loaded (same file, found next to it)


lib = _load()
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


@dataclass
class Result:
    accepted: bool
    check: str  # one of CHECKS: the first check that failed ("NONE" when accepted)
    offset: int  # bytes of the proof consumed when the verdict was reached
    message: str

    def __bool__(self):
        return self.accepted


def _result(r: ResultStruct) -> Result:
    return Result(bool(r.accepted), CHECKS[r.check] if 0 <= r.check < len(CHECKS) else str(r.check), int(r.offset), r.message.decode(errors="replace"))


def _fe_ptr(a, n_fe=None):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    if n_fe is not None and a.shape[0] != n_fe:
        raise ValueError(f"expected {n_fe} field elements, got {a.shape[0]}")
    return a


class Verifier:
    """The statement a proof is checked under: m, m_0, the two WhirConfigs, the IO-pattern bytes in force (None: the library's
    restatement, what a scheme uses unless set_io_pattern was called) and the Skyscraper version."""

    def __init__(self, m: int, m_0: int, whir_witness: WhirConfig, whir_for_hiding_spartan: WhirConfig, io_pattern: bytes | None = None,
                 hash_version: int = 2):
        self.handle = None
        self.ctx = None
        self.m, self.m_0 = m, m_0
        cw, cb = _cfg_struct(whir_witness), _cfg_struct(whir_for_hiding_spartan)
        h = vp()
        pat = bytes(io_pattern) if io_pattern else None
        rc = lib.pkv_verifier_create(m, m_0, C.addressof(cw), C.addressof(cb), pat, len(pat) if pat else 0, hash_version, C.byref(h))
        if rc:
            raise ProveKitHipError(rc, lib.pkv_create_error().decode())
        self.handle = h.value

    @classmethod
    def for_scheme(cls, scheme, matrices=None, interner_mont=None, hash_version: int = 2, attach: bool = True) -> "Verifier":
        """the verifier of a WhirR1CSScheme's proofs, under the IO pattern the scheme has in force.  matrices = (A, B, C) as
        SparseMatrix plus the interner (Montgomery) -- the host arrays the scheme's R1CS was uploaded from -- enable the
        matrix-evaluation check.  attach: bind the scheme's Context for verify_many."""
        v = cls(scheme.m, scheme.m_0, scheme.whir_witness, scheme.whir_for_hiding_spartan, scheme.domain_separator, hash_version)
        if matrices is not None:
            v.set_r1cs(*matrices, interner_mont)
        if attach:
            v.attach(scheme.ctx)
        return v

    def _check(self, rc):
        if rc:
            raise ProveKitHipError(rc, lib.pkv_last_error(self.handle).decode())

    def set_r1cs(self, a: SparseMatrix, b: SparseMatrix, c: SparseMatrix, interner_mont):
        mats = (SparseMatrixStruct * 3)()
        keep = []
        for k, m in enumerate((a, b, c)):
            if (m.num_rows, m.num_cols) != (a.num_rows, a.num_cols):
                raise ValueError("matrix shape mismatch")
            nri, ci, vv = (np.ascontiguousarray(x, dtype=np.uint32) for x in (m.new_row_indices, m.col_indices, m.values))
            keep += [nri, ci, vv]
            mats[k] = SparseMatrixStruct(nri.ctypes.data, ci.ctypes.data, vv.ctypes.data, ci.shape[0])
        it = _fe_ptr(interner_mont)
        self._check(lib.pkv_verifier_set_r1cs(self.handle, a.num_rows, a.num_cols, C.addressof(mats), it.ctypes.data, it.shape[0]))

    def attach(self, ctx):
        """bind a Context (or None) for verify_many; uploads the attached R1CS once"""
        self._check(lib.pkv_verifier_attach_device(self.handle, ctx.handle if ctx is not None else None))
        self.ctx = ctx

    def verify(self, proof: bytes) -> Result:
        """the host core"""
        r = ResultStruct()
        proof = bytes(proof)
        self._check(lib.pkv_verify(self.handle, proof, len(proof), C.byref(r)))
        return _result(r)

    def verify_many(self, proofs) -> list:
        """the device path: every proof's verdict, in order"""
        proofs = [bytes(p) for p in proofs]
        n = len(proofs)
        if not n:
            return []
        ptrs = (C.c_char_p * n)(*proofs)
        lens = (sz * n)(*(len(p) for p in proofs))
        res = (ResultStruct * n)()
        self._check(lib.pkv_verify_many(self.handle, C.cast(ptrs, vp), C.cast(lens, vp), n, C.cast(res, vp)))
        return [_result(r) for r in res]

    def matrix_evaluations(self, alphas, points) -> np.ndarray:
        """[K, 3, 4] Montgomery: eq(alpha_k)^T {A, B, C} eq(point_k) for K pairs (alphas [K, m_0, 4], points [K, m-1, 4])"""
        a = np.ascontiguousarray(alphas, dtype=np.uint64).reshape(-1, self.m_0, 4)
        y = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, self.m - 1, 4)
        if a.shape[0] != y.shape[0]:
            raise ValueError("as many alphas as points")
        out = np.zeros((a.shape[0], 3, 4), dtype=np.uint64)
        self._check(lib.pkv_matrix_evaluations(self.handle, a.ctypes.data, y.ctypes.data, a.shape[0], out.ctypes.data))
        return out

    def close(self):
        if self.handle is not None:
            lib.pkv_verifier_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def openings_check(ctx, leaves, siblings, paths, indices, roots, weights=None, hash_version: int = 2):
    """the openings kernel by itself (pkv_openings_check): leaves [k, width, 4] canonical, siblings [k, 4], paths [k, depth, 4]
    (root -> leaf), indices [k], roots [k, 4], weights [width, 4] Montgomery or None -> (reached [k] bool, folds [k, 4] canonical)"""
    lv = np.ascontiguousarray(leaves, dtype=np.uint64)
    k, width = lv.shape[0], lv.shape[1]
    pa = np.ascontiguousarray(paths, dtype=np.uint64)
    depth = pa.shape[1] if pa.ndim == 3 else (pa.size // (4 * k) if k else 0)  # k = 0 or depth = 0: nothing for reshape to infer from
    pa = pa.reshape(k, depth, 4)
    sb, rt = _fe_ptr(siblings, k), _fe_ptr(roots, k)
    ix = np.ascontiguousarray(indices, dtype=np.uint64)
    w = _fe_ptr(weights, width) if weights is not None else None
    reached = np.zeros(k, dtype=np.uint8)
    folds = np.zeros((k, 4), dtype=np.uint64)
    rc = lib.pkv_openings_check(ctx.handle, hash_version, lv.ctypes.data, k, width, sb.ctypes.data, pa.ctypes.data if depth else None, depth,
                                ix.ctypes.data, rt.ctypes.data, w.ctypes.data if w is not None else None, reached.ctypes.data, folds.ctypes.data)
    if rc:
        raise ProveKitHipError(rc, "pkv_openings_check failed")
    return reached.astype(bool), folds
