"""GPU: the proof engine (include/provekit_engine.h, provekit_amd.ProofEngine) -- many proofs in flight from this test's single
thread.  The acceptance is byte identity: whatever lane ran a job and in whatever order the jobs finished, its proof is the one
WhirR1CSScheme.prove writes for the same (witness, seed) on a context of its own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
DEMO = os.path.join(ROOT, "examples", "prove_demo")
PK_ERR_BAD_ARG, PK_ERR_OOM = -1, -2


@pytest.fixture(autouse=True)
def spinning_waits_afterwards():
    """an engine puts the device in the polling wait; the rest of the suite runs in HIP's default, which may be restored at any time"""
    yield
    import provekit_amd

    provekit_amd.Context.set_host_wait(0, "spin")


def _vcfg(V, c):
    return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, c.num_queries, c.ood_samples, c.pow_bits,
                        c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)


def _second_witness(z, coeffs, trips, n_in, nc):
    """other inputs, outputs recomputed row by row (a row reads only entries before its own output)"""
    import pyref as pr

    z2 = [1] + [(v * 7 + 3) % pr.P for v in z[1 : 1 + n_in]] + [0] * nc
    rows = [([], []) for _ in range(nc)]
    for k in (0, 1):
        for r, c, v in zip(*trips[k]):
            rows[r][k].append((c, coeffs[v]))
    for r in range(nc):
        sa = sum(cf * z2[c] for c, cf in rows[r][0]) % pr.P
        sb = sum(cf * z2[c] for c, cf in rows[r][1]) % pr.P
        z2[1 + n_in + r] = sa * sb % pr.P
    return z2


class Small:
    """the m = 12 instance of tests/test_gpu_prove.py (two WHIR rounds), two witnesses, a lone prover on a context of its own"""

    m, m_0, nc, n_in = 12, 9, 500, 700

    def __init__(self, oracle):
        import provekit_amd
        from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
        from provekit_amd.sparse_matrix import R1CS
        from test_gpu_prove import satisfiable_r1cs, to_sparse

        self.nw, z, self.coeffs, self.trips = satisfiable_r1cs(self.nc, self.n_in, 5)
        z2 = _second_witness(z, self.coeffs, self.trips, self.n_in, self.nc)
        self.ctx = provekit_amd.Context(0)  # fresh: not the session's
        self.r1cs = R1CS(self.ctx, *(to_sparse(self.nc, self.nw, t) for t in self.trips), oracle.to_mont(oracle.ints_to_limbs(self.coeffs)))
        self.cfg_w = WhirConfig.for_size(self.m, 4.0)
        self.cfg_w.num_queries = [20, 12, 9, 8][: self.cfg_w.n_rounds]
        self.cfg_b = blinding_config_for(self.m_0, 4.0)
        self.scheme = WhirR1CSScheme(self.ctx, self.r1cs, self.m, self.m_0, self.cfg_w, self.cfg_b)
        self.d = [self.ctx.upload(oracle.to_mont(oracle.ints_to_limbs(w))) for w in (z, z2)]
        for d in self.d:
            self.r1cs.test_witness_satisfaction(d)

    def engine(self, lanes, **kw):
        import provekit_amd

        return provekit_amd.ProofEngine(self.r1cs, self.m, self.m_0, self.cfg_w, self.cfg_b, lanes=lanes, **kw)

    def single(self, w, seed):
        return self.scheme.prove(self.d[w], seed=seed)

    def verify(self, proof, ds=None):
        import verifier as V

        mats = [(t[0], t[1], [self.coeffs[v] for v in t[2]]) for t in self.trips]
        return V.verify(proof, ds or self.scheme.domain_separator, self.m, self.m_0, _vcfg(V, self.cfg_w), _vcfg(V, self.cfg_b), r1cs=(self.nc, self.nw, mats))

    def close(self):
        self.scheme.close()
        self.r1cs.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def small(oracle):
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first, as tests/conftest.py's ctx does
    s = Small(oracle)
    yield s
    s.close()


def test_byte_identity_m12_and_the_verifier_accepts(small):
    """24 jobs, distinct seeds, two witnesses, 6 lanes, one caller thread: every proof is the lone prover's, and verifies"""
    jobs = [(i % 2, 100 + i) for i in range(24)]
    with small.engine(6) as eng:
        assert eng.lanes == 6
        got = eng.prove_many([small.d[w] for w, _ in jobs], [s for _, s in jobs])
    assert eng.last_status == [0] * 24
    want = [small.single(w, s) for w, s in jobs]
    assert got == want
    assert len(set(got)) == 24
    for p in got:
        assert small.verify(p)


def test_byte_identity_at_the_bench_size(oracle):
    """m = 21 / m_0 = 20, the bench's size class under the reference's own WHIR schedule, built as tests/test_gpu_prove.py builds it"""
    import provekit_amd
    from provekit_amd.field import random_field
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
    from provekit_amd.sparse_matrix import R1CS, SparseMatrix
    from test_gpu_prove import size_class_instance

    m, m_0 = 21, 20
    nc, nw, mats, interner, z = size_class_instance(oracle, m)
    n_in = nw - 1 - nc
    z2 = z.copy()
    z2[1 : 1 + n_in] = random_field(n_in, 6)
    az, bz = (oracle.spmv(nc, nw, nri, ci, v, interner, z2) for nri, ci, v in mats[:2])
    z2[1 + n_in :] = oracle.hadamard(az, bz)
    ctx = provekit_amd.Context(0)
    r1cs = R1CS(ctx, *(SparseMatrix(nc, nw, *t) for t in mats), interner)
    d = [ctx.upload(z), ctx.upload(z2)]
    for dz in d:
        r1cs.test_witness_satisfaction(dz)
    cfg_w, cfg_b = WhirConfig.derive(m), blinding_config_for(m_0)
    jobs = [(i % 2, 500 + i) for i in range(24)]
    with provekit_amd.ProofEngine(r1cs, m, m_0, cfg_w, cfg_b, lanes=6) as eng:
        got = eng.prove_many([d[w] for w, _ in jobs], [s for _, s in jobs])
    scheme = WhirR1CSScheme(ctx, r1cs, m, m_0, cfg_w, cfg_b)
    want = [scheme.prove(d[w], seed=s) for w, s in jobs]
    assert [len(p) for p in got] == [len(p) for p in want] and all(260_000 < len(p) < 277_000 for p in got)
    assert got == want
    scheme.close()
    r1cs.close()
    ctx.close()


def test_job_counts_below_equal_and_above_the_lanes_and_a_second_call(small):
    lanes = 4
    with small.engine(lanes) as eng:
        assert eng.prove_many([]) == [] and eng.last_status == []
        seed = 1000
        for n in (lanes - 1, lanes, 5 * lanes, 1):  # every call after the first is "a second prove_many on the same engine"
            jobs = [((seed + i) % 2, seed + i) for i in range(n)]
            got = eng.prove_many([small.d[w] for w, _ in jobs], [s for _, s in jobs])
            assert got == [small.single(w, s) for w, s in jobs], f"n = {n}"
            seed += n
        # production form: no seeds -> fresh randomness per job, every proof different and valid
        fresh = eng.prove_many([small.d[0]] * 3)
        assert len(set(fresh)) == 3 and all(small.verify(p) for p in fresh)


def test_submit_and_wait_overlap_host_work_and_fill_the_right_slots(small):
    """ten jobs on three lanes finish in whatever order grinding luck and the hand-out give; they are fetched in an order unrelated to
    submission, with host and device work of the caller's own in between"""
    with small.engine(3) as eng:
        jobs = [eng.submit(small.d[i % 2], seed=2000 + i) for i in range(10)]
        host_work = sum(int(x) for x in np.arange(200000) % 7)  # the caller's thread is free while the lanes prove
        assert host_work > 0
        order = [7, 0, 9, 3, 1, 8, 2, 6, 4, 5]
        got = {}
        for k in order:
            got[k] = jobs[k].wait()
            more = small.single(k % 2, 2000 + k)  # host + device work of the caller's own between the waits
            assert got[k] == more, f"slot {k}"
        assert [j.ticket for j in jobs] == list(range(jobs[0].ticket, jobs[0].ticket + 10))
        eng.wait_all()
        assert jobs[4].wait() == got[4]  # waiting twice is harmless


def test_a_dropped_job_is_kept_alive_by_the_engine(small):
    """the buffers a lane writes belong to the Job object: the engine holds every submitted Job until it is final, so a caller that
    throws the result of submit() away (and only calls wait_all), or loses its list to an exception, corrupts nothing"""
    import gc

    with small.engine(2) as eng:
        for i in range(8):
            eng.submit(small.d[i % 2], seed=7000 + i)  # result dropped while a lane is, or will be, writing into it
        gc.collect()
        assert len(eng._outstanding) == 8
        eng.wait_all()
        assert eng._outstanding == {}
        assert eng.prove_many([small.d[0]], [7000]) == [small.single(0, 7000)]  # proves once more, correctly
        kept = eng.submit(small.d[1], seed=7001)
        eng.submit(small.d[0], seed=7002)
        assert kept.wait() == small.single(1, 7001) and kept.ticket not in eng._outstanding
    assert eng._outstanding == {}  # close() released the dropped one


def test_failed_jobs_do_not_stop_the_others_and_the_engine_stays_usable(small):
    import provekit_amd

    n, bad_len, bad_cap = 9, 2, 6
    n_witness = [small.nw] * n
    n_witness[bad_len] = small.nw - 1
    cap = [4 << 20] * n
    cap[bad_cap] = 16
    with small.engine(4) as eng:
        got = eng.prove_many([small.d[i % 2] for i in range(n)], [3000 + i for i in range(n)], n_witness=n_witness, cap=cap, raise_on_error=False)
        assert [i for i, s in enumerate(eng.last_status) if s != 0] == [bad_len, bad_cap]
        assert eng.last_status[bad_len] == PK_ERR_BAD_ARG and eng.last_status[bad_cap] == PK_ERR_BAD_ARG
        assert "witness length" in eng.last_error(eng.last_first_ticket + bad_len)
        assert "too small" in eng.last_error(eng.last_first_ticket + bad_cap)
        for i in range(n):
            assert got[i] == (None if i in (bad_len, bad_cap) else small.single(i % 2, 3000 + i))
        with pytest.raises(provekit_amd.ProveKitHipError, match="job 2: .*witness length") as ei:
            eng.prove_many([small.d[0]] * 3, [1, 2, 3], n_witness=[small.nw, small.nw, 5])
        assert ei.value.code == PK_ERR_BAD_ARG
        bad = eng.submit(small.d[0], seed=1, n_witness=3)
        with pytest.raises(provekit_amd.ProveKitHipError, match="witness length"):
            bad.wait()
        assert eng.prove_many([small.d[1]], [77]) == [small.single(1, 77)]  # usable afterwards


def test_the_c_call_returns_nonzero_iff_a_job_failed(small):
    """pke_prove_many at the C boundary: NULL seed array, per-job status and len, the call's own return"""
    from provekit_amd import engine

    with small.engine(2) as eng:
        n = 3
        bufs = [(C.c_uint8 * (1 << 20))() for _ in range(n)]
        d_w = (C.c_void_p * n)(*[small.d[0].ptr] * n)
        nw = (C.c_size_t * n)(small.nw, small.nw, small.nw)
        out = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        cap = (C.c_size_t * n)(*[1 << 20] * n)
        lens, status = (C.c_size_t * n)(), (C.c_int * n)()
        assert engine.lib.pke_prove_many(eng.handle, n, d_w, nw, None, out, cap, lens, status, None) == 0
        assert list(status) == [0, 0, 0] and all(small.verify(C.string_at(bufs[i], lens[i])) for i in range(n))
        nw[1] = 1
        assert engine.lib.pke_prove_many(eng.handle, n, d_w, nw, None, out, cap, lens, status, None) == PK_ERR_BAD_ARG
        assert list(status) == [0, PK_ERR_BAD_ARG, 0] and lens[1] == 0
        # a job the queue itself refuses (no buffer for a non-zero capacity) fails alone: the jobs after it still run
        nw[1] = small.nw
        out[0] = None
        lens[2] = 0
        assert engine.lib.pke_prove_many(eng.handle, n, d_w, nw, None, out, cap, lens, status, None) == PK_ERR_BAD_ARG
        assert list(status) == [PK_ERR_BAD_ARG, 0, 0] and lens[0] == 0 and all(small.verify(C.string_at(bufs[i], lens[i])) for i in (1, 2))
        assert engine.lib.pke_prove_many(eng.handle, 0, None, None, None, None, None, None, None, None) == 0
        assert engine.lib.pke_wait(eng.handle, 1 << 40) == PK_ERR_BAD_ARG


def test_lanes_zero_picks_a_count(small):
    with small.engine(0) as eng:
        assert 1 <= eng.lanes <= 16
        jobs = [(i % 2, 4000 + i) for i in range(eng.lanes + 1)]
        assert eng.prove_many([small.d[w] for w, _ in jobs], [s for _, s in jobs]) == [small.single(w, s) for w, s in jobs]


def test_a_lane_request_that_cannot_fit_fails_cleanly(small):
    """32 lanes at m = 25: the arenas alone exceed the device, so some lane k meets PK_ERR_OOM; the lanes before it are torn down"""
    import torch

    import provekit_amd
    from provekit_amd.scheme import WhirConfig, arena_bytes, blinding_config_for

    m = 25
    cfg_w, cfg_b = WhirConfig.derive(m), blinding_config_for(small.m_0)
    arena = arena_bytes(m, small.m_0, small.nw, cfg_w)
    free0, _ = torch.cuda.mem_get_info(0)
    if 32 * arena <= free0:
        pytest.skip("32 provers of m = 25 fit on this device")
    with pytest.raises(provekit_amd.ProveKitHipError) as ei:
        provekit_amd.ProofEngine(small.r1cs, m, small.m_0, cfg_w, cfg_b, lanes=32)
    assert ei.value.code == PK_ERR_OOM and "lane" in str(ei.value)
    free1, _ = torch.cuda.mem_get_info(0)
    assert abs(free0 - free1) < arena, f"free memory {free0} -> {free1}"
    with pytest.raises(provekit_amd.ProveKitHipError):  # above the hard cap: refused before anything is built
        provekit_amd.ProofEngine(small.r1cs, small.m, small.m_0, small.cfg_w, small.cfg_b, lanes=33)
    with small.engine(2) as eng:  # and the device is fine
        assert eng.prove_many([small.d[0]], [9]) == [small.single(0, 9)]


def test_io_pattern_and_hash_version_reach_every_lane(small):
    import provekit_amd

    ours = small.scheme.domain_separator
    theirs = ours.replace(b"merkle_digest", b"root").replace(b"stir_queries", b"stir_challenge_indexes")
    lanes = 4
    with small.engine(lanes) as eng:
        assert eng.domain_separator == ours
        eng.set_io_pattern(theirs)
        assert eng.domain_separator == theirs
        small.scheme.set_io_pattern(theirs)
        try:
            want = [small.single(0, 5000 + i) for i in range(3 * lanes)]
            got = eng.prove_many([small.d[0]] * (3 * lanes), [5000 + i for i in range(3 * lanes)])  # 3 waves: every lane has proved
            assert got == want and small.verify(got[0], theirs)
        finally:
            small.scheme.set_io_pattern(None)
        with pytest.raises(provekit_amd.ProveKitHipError, match="IO pattern"):
            eng.set_io_pattern(ours.replace(b"\0Hclaimed_evaluations", b"", 1))
        eng.set_io_pattern(None)
        assert eng.prove_many([small.d[0]] * lanes, [5000] * lanes) == [small.single(0, 5000)] * lanes
        # the hash version too: Skyscraper v1 on every lane gives the lone prover's v1 proofs
        eng.set_hash_version(1)
        small.ctx.set_hash_version(1)
        try:
            want = [small.single(1, 5100 + i) for i in range(2 * lanes)]
            assert eng.prove_many([small.d[1]] * (2 * lanes), [5100 + i for i in range(2 * lanes)]) == want
        finally:
            small.ctx.set_hash_version(2)
        assert small.single(1, 5100) != want[0]
        with pytest.raises(provekit_amd.ProveKitHipError):
            eng.set_hash_version(7)


def test_noir_prove_many_equals_noir_prove(oracle):
    """pke_noir_prove_many: witness transcript, builders, fill and prove per job on the lanes, against WhirR1CSScheme.noir_prove"""
    import provekit_amd
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for
    from provekit_amd.sparse_matrix import R1CS
    from provekit_amd.witness import WitnessProgram
    from test_gpu_prove import to_sparse
    from test_gpu_witness import _mont, _noir_instance

    builders, acir, pub_idx, nw, coeffs, trips = _noir_instance(oracle, 3, n_in=6, n_prod=3000)
    nc = trips[0][0][-1] + 1
    m, m_0 = 13, 12
    ctx = provekit_amd.Context(0)
    r1cs = R1CS(ctx, *(to_sparse(nc, nw, t) for t in trips), oracle.to_mont(oracle.ints_to_limbs(coeffs)))
    cfgs = (WhirConfig.for_size(m, 6.0), blinding_config_for(m_0, 6.0))
    scheme, prog, d_acir = WhirR1CSScheme(ctx, r1cs, m, m_0, *cfgs), WitnessProgram(ctx, builders), ctx.upload(_mont(oracle, acir))
    seeds = list(range(21, 21 + 7))
    want = [scheme.noir_prove(prog, d_acir, len(acir), pub_idx, seed=s) for s in seeds]
    with provekit_amd.ProofEngine(r1cs, m, m_0, *cfgs, lanes=3) as eng:
        with pytest.raises(provekit_amd.ProveKitHipError, match="witness builders"):
            eng.noir_prove_many([d_acir], len(acir), pub_idx, [1])
        eng.set_witness_builders(builders)
        assert eng.builders["n_acir"] == prog.n_acir
        assert eng.noir_prove_many([d_acir] * len(seeds), len(acir), pub_idx, seeds) == want
    prog.close()
    scheme.close()
    r1cs.close()
    ctx.close()


def test_destroy_idle_and_destroy_right_after_submit(small):
    from provekit_amd.engine import PKE_ERR_CANCELLED

    eng = small.engine(2)
    eng.close()  # nothing queued
    eng.close()  # twice is harmless
    eng = small.engine(1)
    jobs = [eng.submit(small.d[0], seed=6000 + i) for i in range(2)]
    eng.close()  # returns: the running job finished, the queued one finished or was reported cancelled
    final = [j._status.value for j in jobs]
    assert all(s in (0, PKE_ERR_CANCELLED) for s in final)
    for i, j in enumerate(jobs):
        if final[i] == 0:
            assert j.wait() == small.single(0, 6000 + i)
        else:
            with pytest.raises(Exception):
                j.wait()
            assert j._len.value == 0
    assert [j._status.value for j in jobs] == final  # final means final


def test_the_cpp_demo_runs_its_engine_section(tmp_path):
    assert os.path.exists(DEMO), "examples/prove_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "300", DEMO, "12", "10", "600", "300", "7", str(tmp_path / "demo")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok transcript_bytes=")
    assert [l for l in lines if l.startswith("engine ")] == ["engine lanes=4 proofs=8 identical_to_single_prove=yes"]
