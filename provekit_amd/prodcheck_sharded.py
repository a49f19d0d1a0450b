"""Product sumchecks sharded over the ranks of a device set (libprovekit_sumcheck.so, include/provekit_sumcheck_sharded.h): the proof
of provekit_amd.prodcheck, byte for byte, with every rank reading 1/G of the tables in the sharded rounds and holding 1/G of the
folded copies.  provekit_amd.prodcheck.verify verifies it: it is the same proof.

`plan` is host only; `Prover` is collective -- create it and call prove() on every context of the set, one host thread per rank,
with the same statement, tau and bind (ranks that disagree all refuse); `round_shard` is one rank's slice of one round on a lone
context, for tests and tools.  Ranks handed different TABLES are not detected: the proof is then of no table.  There is no
fallback: without the built library the import raises."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import prodcheck as _lone
from ._lib import ProveKitHipError, sz, vp
from .prodcheck import Proof, Statement
from .runtime import Context

CHUNK_LOG2, MAX_WORLD_LOG2 = 8, 4


class PlanStruct(C.Structure):
    """struct pkss_plan"""

    _fields_ = [("g", C.c_uint), ("c", C.c_uint), ("S", C.c_uint), ("local_len", sz), ("handover_len", sz), ("arena_bytes", sz)]


class RoundProfileStruct(C.Structure):
    """pkss_round_profile"""

    _fields_ = [("sharded", C.c_uint), ("pairs", C.c_uint64), ("round_seconds", C.c_double), ("exchange_seconds", C.c_double)]


# name -> (restype, argtypes); kept in the same order as include/provekit_sumcheck_sharded.h
SIGNATURES = {
    "pkss_abi_version": (C.c_int, []),
    "pkss_plan": (C.c_int, [vp, C.c_uint, C.POINTER(PlanStruct)]),
    "pkss_prover_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "pkss_prove": (C.c_int, [vp, vp, vp, vp, vp, sz, C.POINTER(sz), vp, vp]),
    "pkss_last_profile": (C.c_int, [vp, C.POINTER(RoundProfileStruct), C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pkss_round_shard": (C.c_int, [vp, vp, vp, sz, vp, vp, vp, C.c_uint, C.c_uint, C.c_uint, vp]),
}

lib = _lone.lib  # the same library
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class Plan:
    """what a sharded proof takes on each of `world` ranks: g = log2(world), c = the chunk's log2, S sharded rounds (0 .. S-1), a
    rank's share of a table, the replicated tables' length and the bytes of the prover's arena"""

    def __init__(self, s: PlanStruct):
        self.g, self.c, self.S = int(s.g), int(s.c), int(s.S)
        self.local_len, self.handover_len, self.arena_bytes = int(s.local_len), int(s.handover_len), int(s.arena_bytes)

    def __repr__(self):
        return f"Plan(g={self.g}, c={self.c}, S={self.S}, local_len={self.local_len}, handover_len={self.handover_len}, arena_bytes={self.arena_bytes})"


def plan(stmt: Statement, world: int) -> Plan:
    """pkss_plan; host only.  Every refusal raises with its reason"""
    s, out = stmt.struct(), PlanStruct()
    rc = lib.pkss_plan(C.addressof(s), world, C.byref(out))
    if rc:
        _lone._refused(rc)
    return Plan(out)


class Prover(_lone.Prover):
    """one statement's sharded prover on ONE context of a device set.  Creation and prove() are collective: every rank makes the same
    calls.  prove() returns the lone prover's Proof on every rank, allocates no device memory and never writes the caller's tables"""

    _create = lib.pkss_prover_create

    def __init__(self, ctx: Context, stmt: Statement):
        super().__init__(ctx, stmt)
        self.rank, self.world, _ = ctx.comm_info()
        self.plan = plan(stmt, self.world)

    def prove(self, d_tables, tau=None, bind=None, capacity: int | None = None) -> Proof:
        return self._prove_with(lib.pkss_prove, d_tables, tau, bind, capacity)

    def last_profile(self) -> dict:
        """this rank's last proof, round by round (pkss_last_profile): {"rounds": [{"sharded", "pairs", "round_s", "exchange_s"}],
        "handover_s", "total_s"} -- host wall time of blocking steps"""
        rounds = (RoundProfileStruct * self.stmt.n)()
        hand, total = C.c_double(), C.c_double()
        rc = lib.pkss_last_profile(self.handle, rounds, self.stmt.n, C.byref(hand), C.byref(total))
        if rc:
            raise ProveKitHipError(rc, "pkss_last_profile")
        return {"rounds": [{"sharded": bool(r.sharded), "pairs": int(r.pairs), "round_s": r.round_seconds, "exchange_s": r.exchange_seconds} for r in rounds],
                "handover_s": hand.value, "total_s": total.value}


def round_shard(ctx: Context, stmt: Statement, d_tables, length: int, world: int, rank: int, tau_rest=None, fold=None, d_out_local=None,
                grid: int = 0) -> np.ndarray:
    """[D + 1, 4] Montgomery: rank `rank` of `world`'s partial sums of ONE sharded round on FULL tables of current length `length`,
    folded first by `fold` -- the rank's part, compacted -- into d_out_local if given (pkss_round_shard; a lone context)"""
    return _lone._round(lib.pkss_round_shard, ctx, stmt, d_tables, length, tau_rest, fold, d_out_local, world, rank, grid)
