#!/usr/bin/env python3
"""bench.py -- proofs/sec of the WHIR prover hot path on MI355X (BASELINE.json metric), one JSON line.

A "step" is the device work of one `prove` on the poseidon-rounds size class (BASELINE configs[1]; m = 21,
m_0 = 20, synthetic satisfiable R1CS + satisfying witness since the .nps is absent from the reference tree): batch-2 WHIR commit of the
masked witness (to_coeffs, RS-encode NTT, Skyscraper Merkle), the 20-round zk-sumcheck with its blinding
commitment and small WHIR proof, the external row and weighted sums, and the 4-round WHIR batch opening
(fold, re-commit, OOD, PoW grind, STIR openings, equality weights, quadratic sumcheck) -- every call through
the C ABI of libprovekit_hip.so, inputs resident in HBM when the clock starts.  The host side is the compiled driver
(pk_prove: Skyscraper duplex-sponge transcript, blinding algebra, challenge bookkeeping); the proof string it returns is
the same one tests/test_gpu_prove.py feeds to the independent verifier.

Multi-GPU (--gpus N under torch.distributed.run): each rank proves independent statements on its own GPU
(weak scaling, no data-path collective); value = total proofs / max-over-ranks time.

A plain run sets up, warms up, times --steps steps and prints the headline; --full adds every secondary figure (rooflines,
one proof at a time, the other size classes, the 2^26 commit, the PCIe-inclusive rate, the CPU baseline, the multi-rank
probes).  --dump-outputs DIR writes the proofs of the last timed step for output-for-output comparison of two builds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec


def synth_r1cs(ctx, m_0, n_wit, seed):
    """R1CS-shaped synthetic instance, SATISFIABLE by construction: 3/4 * 2^m_0 constraints
    (sum a z)(sum b z) = z[out_i] with 3 entries per row in A and B over the inputs -- one of them the constant-one witness in
    half of the rows, so its column has ~2^18.6 entries like a real system's -- C selecting a fresh output per row, small interned
    coefficients; built vectorised.  -> (R1CS, mats, interner, num_constraints, n_in)"""
    from provekit_amd.field import ints_to_limbs
    from provekit_amd.sparse_matrix import R1CS, SparseMatrix

    rng = np.random.default_rng(seed)
    nc = (3 << m_0) // 4 - 3  # not a power of two on purpose: exercises the zero padding
    n_in = n_wit - 1 - nc
    assert n_in >= 8, "witness capacity too small for one output per constraint"
    mats = []
    for _ in range(2):
        base = np.sort(rng.integers(0, 1 + n_in - 2, size=(nc, 3), dtype=np.int64), axis=1) + np.arange(3)
        base[rng.random(nc) < 0.5, 0] = 0  # a constant term in half of the rows: the constant-one witness' column is as heavy as in a real system
        nri = (np.arange(nc, dtype=np.uint32) * 3).astype(np.uint32)
        mats.append(SparseMatrix(nc, n_wit, nri, base.reshape(-1).astype(np.uint32), rng.integers(0, 16, size=3 * nc).astype(np.uint32)))
    mats.append(SparseMatrix(nc, n_wit, np.arange(nc, dtype=np.uint32), (1 + n_in + np.arange(nc)).astype(np.uint32), np.zeros(nc, dtype=np.uint32)))
    R = (1 << 256) % 21888242871839275222246405745257275088548364400416034343698204186575808495617
    P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    interner = ints_to_limbs([(v * R) % P for v in [1, 2, 3, 5, 7, P - 1, P - 2, 11, 13, 17, 19, 23, 29, 31, 37, 41]])
    return R1CS(ctx, *mats, interner), mats, interner, nc, n_in


def satisfying_witness(ctx, r1cs, n_wit, nc, n_in, seed):
    """z = [1 | random inputs | outputs (A z) o (B z)], the outputs computed by the library itself (pk_r1cs_matvec, pk_fe_mul);
    checked with pk_r1cs_test_witness_satisfaction.  -> (device buffer, host copy)"""
    from provekit_amd._lib import lib
    from provekit_amd.field import ints_to_limbs, random_field

    R = (1 << 256) % 21888242871839275222246405745257275088548364400416034343698204186575808495617
    z = np.zeros((n_wit, 4), dtype=np.uint64)
    z[0] = ints_to_limbs([R])[0]
    z[1 : 1 + n_in] = random_field(n_in, seed)
    d_z = ctx.upload(z)
    az, bz = r1cs.matvec(0, d_z), r1cs.matvec(1, d_z)
    ctx._check(lib.pk_fe_mul(ctx.handle, az.ptr, bz.ptr, d_z.view_fe(1 + n_in), nc))
    r1cs.test_witness_satisfaction(d_z)
    return d_z, ctx.download_fe(d_z, n_wit)


def leaf_hash_bytes(cfg_list):
    """algorithmic bytes of every leaf_hash launch of one step: n_leaves * (width + 1) * 32"""
    total, launches, compresses = 0, 0, 0
    for n_vars, batch, rounds in cfg_list:
        rows = 1 << (n_vars + 1 - 4)
        total += rows * (16 * batch + 1) * 32
        compresses += rows * (16 * batch - 1)
        launches += 1
        for r in range(rounds):
            rows >>= 1
            total += rows * 17 * 32
            compresses += rows * 15
            launches += 1
    return total, launches, compresses


def proof_algorithmic_bytes(m, m_0, n_wit, cfg_w, cfg_b):
    """ALGORITHMIC bytes of one proof, every kernel class with SURVEY 8d's per-unit figures: what a proof must
    move through HBM if every array were read and written exactly once per logical pass.  Used for the aggregate
    `step_algorithmic_GBps` (all of a step's bytes over the step's wall time)."""
    FE = 32
    total = 0

    def whir(n, batch, cfg, n_weights_len):
        nonlocal total
        N = 1 << n
        # masks + to_coeffs (64 B per element per polynomial), commit: coeffs read + leaves written + digests
        total += batch * N * FE + batch * N * 2 * FE
        total += batch * N * FE + batch * 2 * N * FE + 2 * (2 * N >> 4) * FE
        total += batch * N * FE  # commitment OOD evaluations (Horner over every polynomial)
        total += (batch + 1) * N * FE * 2  # batch combination of coefficient and evaluation tables
        total += 2 * N * FE + n_weights_len * 2 * FE  # initial weights: eq accumulate (write) + statement weights (axpy)
        ln, nv, rows = N, n, 2 * N >> 4
        for r in range(cfg.n_rounds + 1):
            for _ in range(min(4, nv)):  # quadratic sumcheck sub-rounds: 2 arrays read, halves written
                total += 2 * ln * FE + ln * FE
                ln >>= 1
            nv -= 4
            if r == cfg.n_rounds:
                break
            total += (1 << (nv + 4)) * FE + (1 << nv) * FE  # coefficient fold
            rows >>= 1
            total += (1 << nv) * FE + rows * 16 * FE + 2 * rows * FE  # round commit
            total += (1 << nv) * FE  # OOD
            total += 2 * (1 << nv) * FE  # equality weights of the STIR + OOD points (read-modify-write)
        total += N * FE + n_weights_len * 2 * FE  # deferred weight evaluations: eq table + dots

    whir(m, 2, cfg_w, 3 * n_wit)
    whir(cfg_b.n_vars, 2, cfg_b, 4 * m_0)
    M0 = 1 << m_0
    total += n_wit * FE + 3 * M0 * FE + M0 * FE  # witness bounds (z read, a b c written), eq table
    ln = M0
    for _ in range(m_0):  # cubic rounds: 4 arrays read, halves written
        total += 4 * ln * FE + 2 * ln * FE
        ln >>= 1
    total += M0 * FE + 3 * n_wit * FE + 3 * 2 * n_wit * FE  # eq(alpha), external rows, weighted sums
    return total


def ntt_roofline(prof, steps, m, cfg_w, cfg_b, peak_modmul=None):
    """RS-encode kernels (deinterleave + NTT passes) of one proof, one proof at a time: 64 B per codeword element; and the
    second roofline: modular multiplications -- 0.5 log2(N) butterfly products plus one inter-pass twiddle per
    element and pass boundary -- over the measured peak rate of the product the NTT is made of (the Shoup product by a constant,
    a GENERAL product: 143 multiply-adds; not the squaring's 126 the hash's peak is measured on)."""
    elems, muls = 0, 0.0

    def encode(rows, cols):
        nonlocal elems, muls
        n = rows * cols
        log_n = rows.bit_length() - 1
        passes = 1 if log_n <= 9 else (2 if log_n <= 18 else 3)
        elems += n
        muls += n * (0.5 * log_n + (passes - 1))

    for n_vars, batch, rounds in ((m, 2, cfg_w.n_rounds), (cfg_b.n_vars, 2, cfg_b.n_rounds)):
        rows = 1 << (n_vars + 1 - 4)
        encode(rows, 16 * batch)
        for _ in range(rounds):
            rows >>= 1
            encode(rows, 16)
    ms = sum(prof.get(k, (0, 0.0))[1] for k in ("ntt_pass", "ntt_pass_last", "deinterleave")) / max(steps, 1)
    achieved = 64.0 * elems / (ms * 1e-3) / 1e9 if ms else 0.0
    out = {"kernels": "deinterleave_kernel + ntt8_pass_kernel (all RS-encodes of one proof)", "bound": "hbm", "achieved": achieved,
           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "ms_per_proof": ms,
           "algorithmic_bytes_per_proof": 64.0 * elems,
           "note": "integer-ALU bound: ~0.5*log2(N)+passes modular multiplies per element (DESIGN.md 4)"}
    if peak_modmul and ms:
        rate = muls / (ms * 1e-3)
        out["alu"] = {"achieved": rate / 1e12, "peak": peak_modmul / 1e12, "unit": "T modmul/s", "frac": rate / peak_modmul,
                      "modmul_per_proof": muls, "peak_is": "register-resident Shoup products by a constant (tools/probes pk_probe_constmul_rate), best over occupancy / ILP"}
    return out


def cpu_baseline(m, m_0, mats, interner, nc, n_wit, cfg_w, cfg_b, domain_separator, z_host, seed, gpu_proof, budget_s=75.0):
    """The SAME step on the host cores: one whole proof of the bench's statement through oracle/prover_ref.py -- the reference's
    WhirR1CSProver::prove (provekit/prover/src/whir_r1cs.rs:42-100) restated on the C oracle's kernels (oracle/pk_oracle.c, OpenMP
    wherever the reference uses rayon; the sparse products serial as in the reference), transcript and blinding algebra included --
    with the key the GPU proof was made with, so the two proof strings can be compared byte for byte.  A reported baseline only.
    Run at all threads, then at 16 and at 1 while the time budget lasts (the serial fraction shows in the ratio)."""
    sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import prover_ref as PR
    import verifier as V

    def vcfg(c):
        return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, list(c.num_queries), list(c.ood_samples), list(c.pow_bits),
                            c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)

    r1cs = (nc, n_wit, [(mt.new_row_indices, mt.col_indices, mt.values) for mt in mats], interner)
    host = PR.usable_cores()  # the cgroup quota counts, not the CPUs the container can see
    all_threads = host["usable"]
    out = {"threads": {}, "host": host}
    spent = 0.0
    for threads in (all_threads, 4, 1):
        if threads > all_threads or str(threads) in out["threads"]:
            continue
        # a run at fewer threads takes about all_threads / threads times the parallel part: skip what cannot fit the budget
        est = out["threads"][str(all_threads)]["s_per_proof"] * (all_threads / threads) * 0.8 if out["threads"] else 0.0
        if spent + est > budget_s:
            out["threads"][str(threads)] = {"skipped": f"estimated {est:.0f} s: over the {budget_s:.0f} s budget of this leg (run bench.py --cpu-baseline-budget to raise it)"}
            continue
        PR.L.pko_set_num_threads(threads)
        stage = {}
        t0 = time.perf_counter()
        proof = PR.prove(domain_separator, m, m_0, vcfg(cfg_w), vcfg(cfg_b), r1cs, z_host, seed, stage)
        dt = time.perf_counter() - t0
        spent += dt
        out["threads"][str(threads)] = {"s_per_proof": dt, "proofs_per_s": 1.0 / dt, "stage_s": stage}
        if threads == all_threads:
            out.update(seconds=dt, cores=threads, stage_s=stage, proof_bytes=len(proof),
                       matches_gpu_transcript=(proof == gpu_proof) if gpu_proof is not None else None)
    PR.L.pko_set_num_threads(all_threads)
    return out


def commit_probe(ctx, torch, local_rank, n_vars=26, reps=3, world=1, dist=None, one_gpu=False, takes_part=True, transport=None):
    """BASELINE configs[4] as a secondary figure of the default line: one batch-2 WHIR commit of 2^26 seeded coefficients
    (RS-encode of 2 x 16 NTTs of 2^23 + 2^23 leaf hashes of width 32 + the tree), buffers allocated once.  At world 1 it is
    timed with hipEvents on the context's stream; at world > 1 `ctx` has joined the run's device set, the commit is SHARDED
    by leaf index behind the C ABI (rank g encodes and hashes the rows i = g mod G, one all-gather of leaf digests) and the
    clock is the launcher contract's: barrier, wall time, max over ranks -- so one `--gpus N` run yields both the weak-scaling
    proofs/s and north_star's strong-scaling commit curve.  `world` here is the number of ranks the commit is sharded over (G, a
    power of two <= the run's world size); ranks outside the group (`takes_part` False: `ctx` is None) only keep the barriers
    and the max-over-ranks clock company.  Algorithmic bytes as BASELINE.md 4."""
    import ctypes as C

    from provekit_amd._lib import lib
    from provekit_amd.device_set import max_over_ranks

    n, rows, width = 1 << n_vars, 1 << (n_vars + 1 - 4), 32
    polys = []
    if takes_part:
        for b in range(2):
            t = torch.randint(0, 2**62, (n, 4), dtype=torch.int64, device=f"cuda:{local_rank}", generator=torch.Generator(device=f"cuda:{local_rank}").manual_seed(17 + b))
            t[:, 3] &= (1 << 60) - 1
            polys.append(t)
        torch.cuda.synchronize()
        ptrs = (C.c_void_p * 2)(*[int(t.data_ptr()) for t in polys])
        szs = [C.c_size_t() for _ in range(3)]
        ctx._check(lib.pk_commit_sizes(ctx.handle, 2, n_vars, 1, 4, *[C.byref(x) for x in szs]))
        leaves, nodes, scratch = (ctx.alloc_fe(x.value) for x in szs)
    root_buf = (C.c_uint8 * 32)()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    ms = []
    for i in range(reps + 1):
        if dist is not None:
            barrier()
            t0 = time.perf_counter()
            if takes_part:
                ctx._check(lib.pk_commit_into(ctx.handle, ptrs, 2, n_vars, 1, 4, leaves.ptr, nodes.ptr, scratch.ptr, root_buf, None))
            barrier()
            t = 1e3 * max_over_ranks(time.perf_counter() - t0, dist, None if one_gpu else f"cuda:{local_rank}")
        else:
            ctx.timer_start()
            ctx._check(lib.pk_commit_into(ctx.handle, ptrs, 2, n_vars, 1, 4, leaves.ptr, nodes.ptr, scratch.ptr, root_buf, None))
            t = ctx.timer_stop()
        if i:
            ms.append(t)
    if takes_part:
        for b in (leaves, nodes, scratch):
            b.free()
    del polys
    root = bytes(root_buf).hex()
    alg = 32 * 2 * n + 32 * 2 * 2 * n + 64 * rows
    best = min(ms)
    how = ("one GPU" + ("" if dist is None else "; wall clock, max over ranks")) if world == 1 else (
        f"sharded by leaf index over {world} ranks, " + ("host-transport (gloo) all-gather, single-GPU development mode" if one_gpu
                                                        else "RCCL all-gather of leaf digests over xGMI") + "; wall clock, max over ranks")
    return {"workload": f"batch-2 WHIR commit of 2^{n_vars} coefficients (rate 1/2, fold 16): {rows * 31 + rows - 1} compressions, 32 NTTs of 2^{n_vars - 3}; {how}",
            "n_gpus": world, "scaling": "strong", "ms_per_commit": best, "commits_per_s": 1e3 / best, "algorithmic_GB": alg / 1e9,
            "achieved_GBps": alg / (best * 1e-3) / 1e9, "frac_of_hbm_peak": alg / (best * 1e-3) / 1e9 / (HBM_PEAK_GBS * world), "root": root,
            "transport": transport or ("none" if world == 1 else ("host" if one_gpu else "rccl"))}


def join_subgroup(ctx, rank, G, dist, one_gpu, groups):
    """make `ctx` rank `rank` of the first G ranks of the run (every rank of the run calls this; ranks >= G pass ctx = None).
    RCCL: rank 0's unique id goes round through the launcher's process group.  Development mode (every rank on GPU 0): the
    library's host transport over a gloo subgroup.  Returns the object to keep alive."""
    from provekit_amd.device_set import HostTransport
    from provekit_amd._lib import lib

    if one_gpu:
        if G not in groups:
            groups[G] = dist.new_group(ranks=list(range(G)), backend="gloo")  # collective over the whole run
        if ctx is None:
            return None
        ht = HostTransport(dist, groups[G])
        ctx._check(lib.pk_comm_init_host(ctx.handle, G, rank, ht.callback, None))
        return ht
    import provekit_amd

    box = [provekit_amd.Context.comm_unique_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    if ctx is not None:
        ctx.comm_init_rank(box[0], G, rank)
    return None


def rccl_probe(provekit_amd, torch, rank, local_rank, world, dist, one_gpu, groups, mib=32, reps=5):
    """Evidence that the library's OWN communicator (not torch's) spans the ranks of this run: a context joins the device set
    exactly as the sharded commit's will, reports what pk_comm_info says, and times an all-gather of `mib` MiB per rank (the
    2^26 commit's digest block per GPU at 8 ranks) with hipEvents on the context's stream.  World 1: the RCCL the library would
    use, nothing to gather."""
    import ctypes as C

    from provekit_amd._lib import lib

    out = {"world": 1, "transport": "none"}
    try:
        v, path = provekit_amd.Context.rccl_version()
        out["version"], out["library"] = v, path
    except Exception as e:  # noqa: BLE001
        out["version"], out["library"] = None, f"not loadable: {e}"[:120]
    if world == 1:
        return out
    ctx = provekit_amd.Context(local_rank)
    keep = join_subgroup(ctx, rank, world, dist, one_gpu, groups)  # noqa: F841
    r, w, kind = ctx.comm_info()
    out.update(world=w, rank=r, transport={1: "local", 2: "rccl", 3: "host"}.get(kind, str(kind)))
    nbytes = mib << 20
    send, recv = ctx.alloc(nbytes), ctx.alloc(nbytes * world)
    torch.cuda.synchronize()
    dist.barrier()
    ts = []
    for i in range(reps + 1):
        ctx.timer_start()
        ctx._check(lib.pk_comm_all_gather(ctx.handle, send.ptr, recv.ptr, nbytes))
        t = ctx.timer_stop()
        if i:
            ts.append(t)
    # every rank's block arrived: a checksum word written by each rank before one more (small) gather
    tag = np.full((8,), 0x5EED0000 + rank, dtype=np.uint64)
    ctx.upload_into(send.ptr, tag)
    ctx._check(lib.pk_comm_all_gather(ctx.handle, send.ptr, recv.ptr, 64))
    got = ctx.download(recv, (world, 8))
    out["ranks_seen"] = sorted(int(x) - 0x5EED0000 for x in got[:, 0])
    us = 1e3 * sorted(ts)[len(ts) // 2]
    out[f"allgather_{mib}MiB_us"] = us
    out["allgather_GBps_per_rank_received"] = nbytes * (world - 1) / (us * 1e-6) / 1e9
    send.free()
    recv.free()
    ctx.comm_destroy()
    ctx.close()
    return out


def single_stream_figures(torch, ctx, prover, d_z, latency_pass, sharded, iso_steps=8):
    """one proof at a time on `ctx` (the chip otherwise idle): per-kernel durations with event profiling on (the roofline's isolated figures),
    then the single-stream latency proper without events, then the same in the library's latency mode, and the multiplier's peak rate"""
    import ctypes as C

    ctx.profile(True)
    ctx.profile_reset()
    iso_times = []
    for i in range(iso_steps):
        t1 = time.perf_counter()
        prover.prove_nocopy(d_z, seed=5000 + i)  # returns with the proof on the host: the stream is drained
        iso_times.append(time.perf_counter() - t1)
    torch.cuda.synchronize()
    iso_dt = sorted(iso_times)[iso_steps // 2]  # median: the first proofs after a many-prover phase still see its clocks / queues
    prof_iso = ctx.profile_read()
    ctx.profile(False)

    def one_at_a_time(first_seed):
        ts = []
        for i in range(iso_steps + 2):
            t1 = time.perf_counter()
            prover.prove_nocopy(d_z, seed=first_seed + i)
            ts.append(time.perf_counter() - t1)
        return sorted(ts[2:])[iso_steps // 2]

    if latency_pass:
        iso_dt = one_at_a_time(5500)  # the single-stream figure proper: no event pairs around the launches
    # the same in the library's latency mode (pk_ctx_set_latency_mode: sumcheck rounds enqueued one ahead behind a host-published gate)
    lat_dt = None
    if latency_pass and not sharded:
        try:
            ctx.set_latency_mode(True)
            lat_dt = one_at_a_time(6000)
        finally:
            ctx.set_latency_mode(False)
    # SURVEY 8d's second roofline: peak rate of the register-resident Montgomery squaring, best over occupancy / ILP
    # ... and, for the NTT (whose products are all by constants), the peak rate of the register-resident Shoup product it is made of
    peak_modmul, peak_constmul = 0.0, 0.0
    try:  # the probes live in tools/libpk_probes.so (the lab), not in the product library
        from tools.pk_probes import lib as probes

        for waves in (2, 4, 8):
            for ilp in (1, 2):
                r = C.c_double()
                ctx._check(probes.pk_probe_modmul_rate(ctx.handle, waves, ilp, 2000, C.byref(r)))
                peak_modmul = max(peak_modmul, r.value)
                ctx._check(probes.pk_probe_constmul_rate(ctx.handle, waves, ilp, 1500, 1, C.byref(r)))
                peak_constmul = max(peak_constmul, r.value)
    except ImportError as e:
        print(f"[bench] no multiplier-peak probe ({e}): roofline.alu.peak is null", file=sys.stderr)
    return {"iso_dt": iso_dt, "lat_dt": lat_dt, "prof_iso": prof_iso, "iso_steps": iso_steps, "peak_modmul": peak_modmul, "peak_constmul": peak_constmul}


def single_stream_probe(provekit_amd, torch, local_rank, m, latency_pass):
    """internal (--single-stream-probe): single_stream_figures on the bench's statement in a fresh process; prints one JSON object"""
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for

    m_0, n_wit = m - 1, (1 << (m - 1)) - 5
    ctx = provekit_amd.Context(local_rank)
    r1cs, _, _, nc, n_in = synth_r1cs(ctx, m_0, n_wit, seed=1234)
    d_z, _ = satisfying_witness(ctx, r1cs, n_wit, nc, n_in, 99)
    prover = WhirR1CSScheme(ctx, r1cs, m, m_0, WhirConfig.derive(m), blinding_config_for(m_0))
    for i in range(60):  # ~0.6 s of proofs first: a fresh process finds the chip at its idle clocks
        prover.prove_nocopy(d_z, seed=100 + i)
    out = single_stream_figures(torch, ctx, prover, d_z, latency_pass, False)
    prover.close()
    r1cs.close()
    ctx.close()
    return out


def sharded_proof_probe(provekit_amd, torch, rank, local_rank, world, dist, one_gpu, groups, mm, reps=3):
    """BASELINE configs[3] under several ranks: ONE proof of the m = `mm` size class (the p256 class: 25) sharded over ALL ranks of the
    run behind the C ABI -- every commit split by leaf index with an all-gather of leaf digests, inner trees by contiguous subtree,
    sumcheck tables / weights / OOD evaluations by blocks, opened rows collected from their owners -- strong scaling, the launcher
    contract's clock (barrier, wall time, max over ranks).  Rank 0 also proves the same statement alone with the same key: the two
    proof strings must be the same bytes."""
    import hashlib

    from provekit_amd.device_set import max_over_ranks
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for

    m_0, n_wit = mm - 1, (1 << (mm - 1)) - 5
    cfg_w, cfg_b = WhirConfig.derive(mm), blinding_config_for(m_0)
    dev = None if one_gpu else f"cuda:{local_rank}"

    def barrier():
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()

    ctx = provekit_amd.Context(local_rank)
    r1cs, _, _, nc, n_in = synth_r1cs(ctx, m_0, n_wit, seed=4321 + mm)  # the same statement and witness on every rank
    d_z, z_host = satisfying_witness(ctx, r1cs, n_wit, nc, n_in, 7 + mm)
    lone_ms, lone_proof = None, None
    if rank == 0:  # the lone prover first, on a context without a communicator
        lone = WhirR1CSScheme(ctx, r1cs, mm, m_0, cfg_w, cfg_b)
        lone.prove_nocopy(d_z, seed=1)
        ts = []
        for i in range(reps):
            t0 = time.perf_counter()
            lone_proof = lone.prove(d_z, seed=2 + i)
            ts.append(time.perf_counter() - t0)
        lone_ms = 1e3 * sorted(ts)[len(ts) // 2]
        lone.close()
    keep = join_subgroup(ctx, rank, world, dist, one_gpu, groups)  # noqa: F841 (kept alive); from here on this context shards
    prover = WhirR1CSScheme(ctx, r1cs, mm, m_0, cfg_w, cfg_b)
    prover.prove_nocopy(d_z, seed=1)
    ts, proof = [], None
    for i in range(reps):
        barrier()
        t0 = time.perf_counter()
        proof = prover.prove(d_z, seed=2 + i)
        barrier()
        ts.append(max_over_ranks(time.perf_counter() - t0, dist, dev))
    ms = 1e3 * sorted(ts)[len(ts) // 2]
    out = {"workload": f"one proof of the m={mm} size class ({nc} constraints, {n_wit} witnesses, derived schedule) sharded over {world} ranks "
                       f"({'host-transport, single-GPU development mode' if one_gpu else 'RCCL over xGMI'}); wall clock, max over ranks, median of {reps}",
           "m": mm, "n_gpus": world, "scaling": "strong", "ms_per_proof": ms, "proofs_per_s": 1e3 / ms, "one_gpu_ms_per_proof": lone_ms,
           "speedup_vs_one_gpu": (lone_ms / ms) if lone_ms else None, "proof_bytes": len(proof), "proof_sha256_16": hashlib.sha256(proof).hexdigest()[:16],
           "equals_the_lone_provers_transcript": (proof == lone_proof) if rank == 0 else None}
    prover.close()
    ctx.comm_destroy()
    d_z.free()
    r1cs.close()
    ctx.close()
    torch.cuda.empty_cache()
    return out


# provers in flight per size class on one MI355X (the memory allows 37 at m = 23 and 9 at m = 25): where more stop paying -- m = 23: 14 -> 66.2,
# 20 -> 67.0, 24 -> 65.8 proofs/s; m = 25: 3 -> 15.7-15.9, 6 -> 15.9-16.1, 8 -> 16.0 (three provers' kernels already fill the chip): profiles/r06_size_class_sweep.jsonl
SIZE_CLASS_PROVERS_CAP = {23: 20, 25: 6}


def size_class_probe(provekit_amd, torch, local_rank, m, proofs_per_prover=3):
    """Secondary figure of the default line: another BASELINE size class (configs[2]: m = 23, configs[3]: m = 25) on this GPU --
    the reference's own derived WHIR schedule for that size, a satisfiable synthetic R1CS of the same construction as the bench's
    (ONE statement and witness shared by the provers of the class; masks differ per proof), provers capped at half the HBM.
    A handful of proofs each: throughput with all provers in flight, then one proof at a time."""
    import threading

    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, arena_bytes, blinding_config_for

    m_0 = m - 1
    n_wit = (1 << (m - 1)) - 5
    cfg_w, cfg_b = WhirConfig.derive(m), blinding_config_for(m_0)
    torch.cuda.empty_cache()  # the commit probe's coefficient tensors
    free, total = torch.cuda.mem_get_info(local_rank)
    # what a prover really holds: its arena (pk_scheme_arena_bytes: every buffer of one proof), its copy of the witness, its context's
    # scratch; the R1CS and the twiddle tables are shared by the provers of a device.  As many as fit in 80 % of the free HBM, up to
    # the count past which more provers in flight stop paying (profiles/r06_size_class_sweep.jsonl); PK_BENCH_SIZE_CLASS_PROVERS overrides.
    per_prover = arena_bytes(m, m_0, n_wit, cfg_w) + 32 * n_wit + (256 << 20)
    conc = max(1, min(SIZE_CLASS_PROVERS_CAP.get(m, 16), int(0.8 * free / per_prover)))
    if os.environ.get("PK_BENCH_SIZE_CLASS_PROVERS"):
        conc = max(1, min(int(os.environ["PK_BENCH_SIZE_CLASS_PROVERS"]), int(0.95 * free / per_prover)))
    c0 = provekit_amd.Context(local_rank)
    r1cs, _, _, nc, n_in = synth_r1cs(c0, m_0, n_wit, seed=4321 + m)
    d_z, z_host = satisfying_witness(c0, r1cs, n_wit, nc, n_in, 7 + m)
    ctxs = [c0] + [provekit_amd.Context(local_rank) for _ in range(conc - 1)]
    provers = [WhirR1CSScheme(c, r1cs, m, m_0, cfg_w, cfg_b) for c in ctxs]  # a pk_r1cs is immutable: one upload serves every context
    wit = [d_z] + [c.upload(z_host) for c in ctxs[1:]]

    def wave(first_seed, per):
        def work(w):
            for i in range(per):
                provers[w].prove_nocopy(wit[w], seed=first_seed + w * per + i)

        ths = [threading.Thread(target=work, args=(w,)) for w in range(conc)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()

    from provekit_amd.hostinfo import usable_cores

    wait = os.environ.get("PK_BENCH_SIZE_CLASS_WAIT") or ("poll" if conc > usable_cores()["usable"] else "spin")
    if wait == "poll":
        provekit_amd.Context.set_host_wait(local_rank, "poll")  # more provers than cores: the library's own query-and-sleep wait (switchable)
    wave(900000, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wave(1, proofs_per_prover)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    provekit_amd.Context.set_host_wait(local_rank, "spin")
    singles = []
    for i in range(3):
        t1 = time.perf_counter()
        provers[0].prove_nocopy(wit[0], seed=77 + i)
        singles.append(time.perf_counter() - t1)
    out = {"m": m, "m_0": m_0, "schedule": "derived by pk_whir_config_derive (a restatement of WhirConfig::new pinned against the reference at n = 21 and n = 8 only: "
                                       "queries / pow_bits at this size are an extrapolation)",
           "constraints": nc, "witnesses": n_wit, "queries": list(cfg_w.num_queries) + [cfg_w.final_queries],
           "pow_bits": list(cfg_w.pow_bits) + [cfg_w.final_pow_bits], "provers": conc, "host_wait": wait, "arena_bytes_per_prover": per_prover,
           "proofs_timed": conc * proofs_per_prover,
           "proofs_per_s": conc * proofs_per_prover / dt, "single_proof_ms": 1e3 * sorted(singles)[1]}
    for p in provers:
        p.close()
    for w in wit[1:]:
        w.free()
    r1cs.close()
    for c in ctxs:
        c.close()
    torch.cuda.empty_cache()
    return out


def commit_workload(args, rank, local_rank, world, dist, torch):
    """configs[4]: one batch-2 commit of 2^m coefficients (default m as given; 26 for the BASELINE config), sharded by
    leaf index over the ranks behind the C ABI (pk_commit_into on a context that joined the device set: rank g encodes and
    hashes the rows i = g mod G, ncclAllGather of the leaf digests over xGMI, inner tree on every rank): strong scaling,
    one collective per commit."""
    import ctypes as C

    import provekit_amd
    from provekit_amd._lib import lib

    from provekit_amd.device_set import join_device_set, max_over_ranks

    m = args.m
    ctx = provekit_amd.Context(local_rank)
    # RCCL over xGMI, one rank per GPU; PK_BENCH_ONE_GPU=1 (development aid: every rank on GPU 0, where RCCL cannot form a
    # communicator) takes the library's host transport over the launcher's gloo group instead -- the same sharded commit code
    one_gpu = os.environ.get("PK_BENCH_ONE_GPU") == "1"
    transport = join_device_set(ctx, rank, world, dist, "host" if one_gpu else "rccl")  # noqa: F841 (kept alive)
    n = 1 << m
    # seeded uniform coefficients generated on the device (identical on every rank: each rank needs the full vectors)
    polys = []
    for bidx in range(2):
        t = torch.randint(0, 2**62, (n, 4), dtype=torch.int64, device=f"cuda:{local_rank}", generator=torch.Generator(device=f"cuda:{local_rank}").manual_seed(17 + bidx))
        t[:, 3] &= (1 << 60) - 1  # < 2^252 < p: a valid field element image
        polys.append(t)
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * 2)(*[int(t.data_ptr()) for t in polys])
    szs = [C.c_size_t() for _ in range(3)]
    ctx._check(lib.pk_commit_sizes(ctx.handle, 2, m, 1, 4, *[C.byref(x) for x in szs]))
    leaves, nodes, scratch = (ctx.alloc_fe(x.value) for x in szs)
    root = (C.c_uint8 * 32)()

    def commit():
        ctx._check(lib.pk_commit_into(ctx.handle, ptrs, 2, m, 1, 4, leaves.ptr, nodes.ptr, scratch.ptr, root, None))

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(max(args.warmup, 1)):
        commit()
    ctx.profile(args.full)  # hipEvent pairs around the launches: the roofline / per-stage figures of --full
    ctx.profile_reset()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        commit()  # blocking: returns the root (stream synchronised)
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0, dist, None if one_gpu else f"cuda:{local_rank}")
    prof = ctx.profile_read()
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, [("root", bytes(root))])
        emit_commit_line(args, world, m, dt, prof, bytes(root).hex(),
                         ("host-transport (gloo) all-gather of leaf digests, single-GPU development mode" if one_gpu else
                          "RCCL all-gather of leaf digests") + " behind the C ABI (pk_commit_into)")
    if dist is not None:
        dist.destroy_process_group()


def emit_commit_line(args, world, m, dt, prof, root_hex, how):
    n, rows = 1 << m, 1 << (m + 1 - 4)
    alg_bytes = 32 * 2 * n + 32 * 2 * 2 * n + 64 * rows  # coeffs read + leaves written + digests
    line = {
        "metric": "commits/sec (2^m-coefficient batch-2 WHIR commit: RS-encode NTT + Skyscraper Merkle)",
        "value": args.steps / dt, "unit": "commits/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "u32x8 (BN254-Fr, 256-bit Montgomery integers)", "data": "synthetic",
        "config": {"workload": f"synthetic WHIR commit: batch 2, n={m}, rate 1/2, fold 16, sharded by leaf index over {world} GPU(s), {how}",
                   "root": root_hex},
    }
    if args.full:  # the per-launch figures of the events recorded in the timed region
        n_l, ms_l = prof.get("leaf_hash", (1, 0.0))
        avg_ms = ms_l / max(n_l, 1)
        lh_bytes = (rows // world) * 33 * 32
        achieved = lh_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms else 0.0
        line.update({
            "commit_GBps_algorithmic": alg_bytes / (dt / args.steps) / 1e9,
            "roofline": {"kernel": "leaf_hash_kernel", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": avg_ms,
                         "algorithmic_bytes_per_launch": lh_bytes},
            "stage_ms_per_step": {k: round(v[1] / args.steps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])},
        })
    emit(line)


def self_launch(args):
    """`python bench.py --gpus N` with no launcher around it: start N ranks of this file under torch.distributed.run on this
    node (one process per GPU, rendezvous on 127.0.0.1 at a free port) and pass rank 0's JSON line through.  N is clamped to
    the GPUs present unless PK_BENCH_ONE_GPU=1 (development aid: every rank on GPU 0 over gloo)."""
    import socket
    import subprocess

    n = args.gpus
    if os.environ.get("PK_BENCH_ONE_GPU") != "1":
        import torch  # (torch's HIP runtime must be the first to initialise in a process that uses both: not pk_device_count here)

        have = torch.cuda.device_count()
        if have < n:
            print(f"[bench] --gpus {n} asked for, {have} GPU(s) visible: running on {max(have, 1)}", file=sys.stderr)
            n = max(have, 1)
    argv = [a for a in sys.argv[1:]]
    for i, a in enumerate(argv):  # rewrite --gpus to what will really run
        if a == "--gpus":
            argv[i + 1] = str(n)
        elif a.startswith("--gpus="):
            argv[i] = f"--gpus={n}"
    for i, a in enumerate(argv):  # the launcher's own parser rejects --m as an ambiguous abbreviation
        if a == "--m":
            argv[i] = "--log2-size"
    if n <= 1:
        os.environ["WORLD_SIZE"] = "1"
        sys.argv = [sys.argv[0]] + argv
        return main()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PK_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    rc = subprocess.call(cmd, env=env)
    if rc:
        raise SystemExit(rc)


_STDOUT_FD = None


def emit(line):
    """the one JSON line, on the real stdout"""
    sys.stdout.flush()
    if _STDOUT_FD is not None:
        os.dup2(_STDOUT_FD, 1)
    print(json.dumps(line), flush=True)


DUMP_LIMIT_BYTES = 64 * 10**6


def dump_outputs(out_dir, named_bytes):
    """--dump-outputs: every (name, bytes) as DIR/<name>.npy, one float32 per byte (exact), in the given order while the files fit
    DUMP_LIMIT_BYTES -- a fixed prefix of the list, so two runs with the same arguments write the same files"""
    os.makedirs(out_dir, exist_ok=True)
    used = 0
    for name, raw in named_bytes:
        a = np.frombuffer(bytes(raw), dtype=np.uint8).astype(np.float32)
        if used + a.nbytes + 128 > DUMP_LIMIT_BYTES:  # 128: the .npy header
            break
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        used += a.nbytes + 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=12, help="timed steps; one step = one wave of --concurrency proofs per GPU")
    ap.add_argument("--warmup", type=int, default=2, help="untimed warm-up steps (waves)")
    ap.add_argument("--m", "--log2-size", dest="m", type=int, default=21,
                    help="log2 of the committed polynomial size (poseidon-rounds: 21).  Under torch.distributed.run spell it "
                         "--log2-size: the launcher's own parser rejects --m as an ambiguous abbreviation")
    ap.add_argument("--host-wait", choices=["auto", "spin", "block", "poll"], default="auto",
                    help="how the provers' host threads wait for the GPU: spin (HIP default), block (sleep on the interrupt), auto = block only when this "
                         "rank's share of the usable host cores is smaller than its number of provers")
    ap.add_argument("--no-sharded-proof", action="store_true", help="under several ranks: skip the secondary figure 'one proof of the p256 size class sharded over all ranks'")
    ap.add_argument("--sharded-proof-log2-size", type=int, default=25, help="size class of that figure (25 = BASELINE configs[3])")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-budget", type=float, default=75.0, help="seconds the CPU-baseline leg may spend on its runs at fewer threads (the run at all usable cores always happens)")
    ap.add_argument("--no-commit-probe", action="store_true", help="skip the secondary 2^26 commit figure (configs[4]) of the default line")
    ap.add_argument("--commit-log2-size", type=int, default=26, help="log2 coefficients of the secondary commit figure (26 = BASELINE configs[4])")
    ap.add_argument("--size-classes", default="23,25",
                    help="other BASELINE size classes reported as secondary keys of the default line (configs[2]: 23, configs[3]: 25); '' = none")
    ap.add_argument("--size-class-probe", type=int, default=0,
                    help="internal: run ONE size-class probe in this (fresh) process and print its JSON object; the default line spawns one "
                         "such process per class: run back to back inside one process, whichever probe comes later measures up to 25 %% "
                         "low (m = 25 15.1 -> 12.3 proofs/s, 2^26 commit 57.8 -> 74.6 ms).  Not the allocator (allocate/free churn alone does not "
                         "reproduce it, tools/alloc_effect.py); most likely the package power limit: 16 provers draw ~1.28 kW and already run at 2.26 GHz "
                         "instead of 2.39 (tools/power_trace.sh), and seconds of that heat the package for whatever follows.  The idle seconds a fresh "
                         "process brings remove the effect; every figure then matches a dedicated run of that size")
    ap.add_argument("--single-stream-probe", action="store_true", help="internal: the one-proof-at-a-time figures of the default line in this (fresh, spinning) process; prints their JSON object")
    ap.add_argument("--no-latency-pass", action="store_true", help="skip the untimed one-at-a-time passes after the isolated-kernel pass (rocprofv3 runs: keeps the trace to "
                                                                   "the timed region + 8 isolated proofs)")
    ap.add_argument("--no-h2d-probe", action="store_true", help="skip the secondary PCIe-inclusive rate (witness uploaded before every proof)")
    ap.add_argument("--workload", choices=["prove", "commit"], default="prove",
                    help="prove = BASELINE configs[1] (default, the judged line); commit = one batch-2 WHIR commit of 2^m coefficients "
                         "(configs[4] with --m 26), SHARDED over the ranks with an all-gather of leaf digests (strong scaling)")
    ap.add_argument("--concurrency", type=int, default=20,
                    help="provers per GPU, each with its own context/stream/arena (host transcript work of one proof overlaps "
                         "the kernels of another); 1 = strictly one proof at a time.  20 with sleeping host threads is the measured optimum on one "
                         "MI355X (profiles/r05_wait_ab.jsonl: 16 spinning 260.7, 16 blocking 262.6, 20 blocking 266.8 proofs/s on one box; polling = blocking + 1 %%)")
    ap.add_argument("--sharded", action="store_true",
                    help="prove workload, latency mode (BASELINE configs[3]): ONE proof at a time sharded over all ranks -- every large "
                         "commit split by leaf index with an RCCL all-gather of leaf digests behind the C ABI; strong scaling")
    ap.add_argument("--h2d", action="store_true",
                    help="upload the witness from (pageable) host memory before every proof: the PCIe-inclusive rate DESIGN.md quotes; "
                         "never the judged line (inputs are resident when the clock starts)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline figure: the one-proof-at-a-time and isolated-kernel passes (roofline, single_stream), "
                         "the size classes, the 2^26 commit, the PCIe-inclusive rate, the CPU baseline, the library's communicator probe and, "
                         "under several ranks, the sharded figures.  The --no-* switches above trim a --full run.  Without it a run sets up, "
                         "warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32): prove = the proof "
                         "strings of its proofs (proof_000.npy, ... one value per byte, in seed order, as many as fit 64 MB), commit = "
                         "the Merkle root (root.npy).  Inputs and keys are seeded: the same arguments give the same files")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args)

    if os.environ.get("PK_BENCH_DUMP_AFTER_S"):  # debugging aid: every thread's Python stack on stderr after N seconds (a hang shows where)
        import faulthandler

        faulthandler.dump_traceback_later(float(os.environ["PK_BENCH_DUMP_AFTER_S"]), repeat=False, file=sys.stderr)

    # stdout carries exactly one JSON line: libraries that print banners there (RCCL's version block at communicator
    # creation) are sent to stderr for the duration of the run
    global _STDOUT_FD
    sys.stdout.flush()
    _STDOUT_FD = os.dup(1)
    os.dup2(2, 1)

    # One hardware queue per prover stream: the HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES (default 4) hardware
    # queues, and with 4 the one-workgroup kernels of some provers block the chip-filling kernels of others (head-of-line).
    # Must be set before the runtime initialises (i.e. before torch is imported).
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # development aid: PK_BENCH_ONE_GPU=1 runs a multi-rank launch with every rank on GPU 0 over gloo, to exercise the
    # N>1 control flow (barriers, max-over-ranks, the sharded commit's collectives) on a single-GPU box; never a measurement
    one_gpu = os.environ.get("PK_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local_rank = 0
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch

    if not torch.cuda.is_available():  # (also: torch's HIP runtime initialises before this library's first call)
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    import provekit_amd

    # How the provers' host threads wait for the device, decided ONCE, before torch or this library creates a stream on the device (the mode must not change while
    # work is in flight: a wait that blocks on a signal created for polling never wakes -- measured as a hang).  Spinning is
    # HIP's default and the fastest for one proof at a time; it costs a busy core per waiting thread, so when the cores this process may use
    # (cgroup quota / ranks on this node) are fewer than the provers it runs, the threads sleep on the completion interrupt instead.
    from provekit_amd.hostinfo import usable_cores

    cores = usable_cores()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    cores_per_rank = cores["usable"] / max(local_world, 1)
    # auto: many provers in flight -> PK_WAIT_POLL, the library's own query-and-sleep loop (as fast as blocking or faster, a third of its host CPU,
    # and -- being the library's own -- safe to switch: it is on for the many-prover phases and off for the one-at-a-time passes); one prover -> spin.
    # Provers that each have a core to themselves keep spinning: polling notices completion up to 0.1 ms late, 65 times per proof, which a
    # chip full of other provers' work hides and a chip with three provers on it (the m = 25 class) does not (15.0 -> 14.3 proofs/s).
    # (From 16 provers up sleeping is at least as fast even when every prover has a core: 16 spinning 260.7, 16 sleeping 262.6 proofs/s.)
    wait_mode = args.host_wait if args.host_wait != "auto" else (
        "poll" if (args.concurrency > cores_per_rank or args.concurrency >= 16) and not args.sharded else "spin")
    block_wait = wait_mode == "block"  # a mode of the RUNTIME: fixed for the life of the process, one-at-a-time figures from a fresh process
    if block_wait:
        provekit_amd.Context.set_host_wait(local_rank, "block")

    def throughput_wait(on):
        if wait_mode == "poll":
            provekit_amd.Context.set_host_wait(local_rank, "poll" if on else "spin")

    dist = None
    if world > 1 or "TORCHELASTIC_RUN_ID" in os.environ or os.environ.get("PK_BENCH_FORCE_DIST"):
        # launched by torch.distributed.run: one rank per GPU over RCCL ("nccl" is RCCL on ROCm)
        import torch.distributed as dist

        torch.cuda.set_device(local_rank)
        if os.environ.get("MASTER_ADDR", "127.0.0.1") in ("127.0.0.1", "localhost"):
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")  # one node: gloo need not resolve the container's hostname to find an interface
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    # a process group of its own for the watchdogs' verdicts ("did a guarded step hang on some rank?"): the stuck thread may sit inside a
    # collective of the default group, where a second collective from the main thread would pair with the wrong operation on the peers
    flags_group = None
    if dist is not None:
        try:
            flags_group = dist.new_group(backend="gloo")
        except Exception as e:  # noqa: BLE001 -- e.g. no interface gloo can bind: the verdicts then travel over the default group
            print(f"[bench] no gloo group for the watchdogs' verdicts ({str(e)[:120]}): using the default group", file=sys.stderr)

    def any_rank(flag):
        if dist is None:
            return bool(flag)
        if flags_group is None:
            return max_over_ranks(1.0 if flag else 0.0, dist, None if one_gpu else f"cuda:{local_rank}") > 0
        t = torch.tensor([1.0 if flag else 0.0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=flags_group)
        return t.item() > 0

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")

    import provekit_amd
    from provekit_amd.field import random_field
    from provekit_amd.scheme import WhirConfig, WhirR1CSScheme, blinding_config_for

    if args.workload == "commit":
        return commit_workload(args, rank, local_rank, world, dist, torch)
    if args.size_class_probe:
        return emit(size_class_probe(provekit_amd, torch, local_rank, args.size_class_probe))
    if args.single_stream_probe:
        return emit(single_stream_probe(provekit_amd, torch, local_rank, args.m, not args.no_latency_pass))

    m = args.m

    def run_size_classes():
        import subprocess

        figs = {}
        for mm in [int(x) for x in args.size_classes.split(",") if x.strip()]:
            try:  # a fresh process per class on this GPU (see --size-class-probe)
                env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "TORCHELASTIC_RUN_ID", "PK_BENCH_FORCE_DIST")}
                env["LOCAL_RANK"] = str(local_rank)  # the same device; no process group in the child
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--size-class-probe", str(mm)], env=env, capture_output=True, text=True,
                                     timeout=600)
                lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
                figs[str(mm)] = json.loads(lines[-1]) if out.returncode == 0 and lines else {"error": (out.stderr or "no output")[-200:]}
            except Exception as e:  # noqa: BLE001
                figs[str(mm)] = {"error": str(e)[:200]}
        return figs

    # On one GPU the size classes are measured FIRST, before this process creates a prover: taken after the main run they read 6-7 % low (m = 23:
    # 59.6 against 64.2 proofs/s, m = 25: 14.2 against 15.1, alternating on one box; the headline is the same either way: 268.6 / 268.0) -- the chip has
    # just spent seconds at its power limit and this process still holds queues on it.  Under several ranks they stay at the end (rank 0 would keep the
    # others waiting inside the communicator probe's watchdog).
    size_figs = {}
    if args.full and os.environ.get("PK_BENCH_SIZE_CLASSES_LAST") != "1" and rank == 0 and m == 21 and not args.sharded and args.size_classes and world == 1:
        size_figs = run_size_classes()
    # The one-proof-at-a-time figures of a process that will run its provers' threads in blocking-wait mode are taken by a FRESH process in
    # the default spinning mode, and FIRST, before this process creates a prover (a second process on a GPU where another holds two dozen idle
    # hardware queues runs ~3.5 % slower -- measured: 9.9 against 9.6 ms per proof)
    ss = None
    if args.full and block_wait and rank == 0 and not args.sharded:
        try:
            import subprocess

            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "TORCHELASTIC_RUN_ID", "PK_BENCH_FORCE_DIST", "PK_BENCH_TEST_HANG")}
            env["LOCAL_RANK"] = str(local_rank)
            cmd = [sys.executable, os.path.abspath(__file__), "--single-stream-probe", "--log2-size", str(m), "--host-wait", "spin"] + (["--no-latency-pass"] if args.no_latency_pass else [])
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode == 0 and lines:
                ss = json.loads(lines[-1])
                ss["prof_iso"] = {k: tuple(v) for k, v in ss["prof_iso"].items()}
                ss["how"] = "a fresh process in spinning-wait mode (this one runs its provers' threads blocking)"
            else:
                print(f"[bench] single-stream probe failed ({(out.stderr or 'no output')[-200:]}): measuring in this process", file=sys.stderr)
        except Exception as e:  # noqa: BLE001
            print(f"[bench] single-stream probe failed ({e}): measuring in this process", file=sys.stderr)

    import threading

    m, m_0 = args.m, args.m - 1
    n_wit = (1 << (m - 1)) - 5
    cfg_w = WhirConfig.derive(m)  # the reference's own schedule (new_whir_config_for_size): queries, OOD samples, pow_bits
    cfg_b = blinding_config_for(m_0)
    conc = 1 if args.sharded else max(1, args.concurrency)
    # every prover owns its arena (pk_scheme_arena_bytes, ~20.6 x 32 B x 2^m), a copy of the statement and of the witness and a workspace:
    # keep the provers within 80 % of the HBM
    from provekit_amd.scheme import arena_bytes

    per_prover = arena_bytes(m, m_0, n_wit, cfg_w) + 8 * 32 * (1 << m_0) + (256 << 20)
    conc = max(1, min(conc, int(float(os.environ.get("PK_BENCH_HBM_FRACTION", "0.8")) * torch.cuda.get_device_properties(local_rank).total_memory / per_prover)))
    from provekit_amd.device_set import join_device_set, max_over_ranks

    workers = []  # (ctx, prover, witness): one independent prover per worker, all on this rank's GPU
    transports = []
    for w in range(conc):
        c = provekit_amd.Context(local_rank)
        if args.sharded and world > 1:  # this context is one rank of the device set: its commits are sharded from here on
            transports.append(join_device_set(c, rank, world, dist, "host" if one_gpu else "rccl"))
        srank = 0 if args.sharded else rank  # the ranks of a sharded prover hold the SAME statement and witness
        r1cs_w, mats, interner, nc, n_in = synth_r1cs(c, m_0, n_wit, seed=1234 + srank)
        # one witness per rank, each prover with its own copy: a proof is then a function of its seed alone, whichever prover the
        # dynamic hand-out gives it to, so what --dump-outputs writes is the same from run to run
        if w == 0:
            d_z, z_host = satisfying_witness(c, r1cs_w, n_wit, nc, n_in, 99 + srank)
        else:
            d_z = c.upload(z_host)
        if os.environ.get("PK_BENCH_LATENCY_ALL") == "1":  # experiment: every prover in latency mode while they share the chip
            c.set_latency_mode(True)
        workers.append((c, WhirR1CSScheme(c, r1cs_w, m, m_0, cfg_w, cfg_b), d_z, r1cs_w, z_host))
    ctx = workers[0][0]
    mats0, interner0 = mats, interner  # every prover of a rank proves the same statement (one seed) and witness

    def run_proofs(first_seed, count, keep=None):
        """`count` proofs through the `conc` provers of this GPU.  Work is handed out dynamically (each prover thread takes the
        next proof when it finishes one), so the chip stays full until the last wave whatever the count; ctypes releases the
        GIL inside pk_prove.  Seeds are injected (test hook) only to make runs comparable; production passes none.
        keep: a dict that receives the proof strings of the last `conc` proofs (the last step), by position in the step."""
        import itertools

        nxt = itertools.count()
        lock = threading.Lock()

        def work(w):
            c, prover, d_z, _, z_host = workers[w]
            while True:
                with lock:
                    i = next(nxt)
                if i >= count:
                    return
                if args.h2d:
                    c.upload_into(d_z.ptr, z_host)
                if keep is not None and i >= count - conc:
                    keep[i - (count - conc)] = prover.prove(d_z, seed=first_seed + i)
                else:
                    prover.prove_nocopy(d_z, seed=first_seed + i)

        ths = [threading.Thread(target=work, args=(w,)) for w in range(conc)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # The library's own communicator, before anything is timed (under a watchdog: a communicator that cannot form costs the run its
    # collective figures and nothing else)
    groups, hung = {}, False
    rccl_fig = None
    if args.full and not args.sharded:
        box = {}

        def probe():
            torch.cuda.set_device(local_rank)  # the current device is per thread
            if os.environ.get("PK_BENCH_TEST_HANG") == "probe":  # test hook: a communicator that never forms
                threading.Event().wait()
            try:
                box.update(fig=rccl_probe(provekit_amd, torch, rank, local_rank, world, dist, one_gpu, groups))
            except Exception as e:  # noqa: BLE001
                box.update(fig={"world": world, "error": str(e)[:300]})

        th = threading.Thread(target=probe, daemon=True)
        th.start()
        th.join(float(os.environ.get("PK_BENCH_RCCL_LIMIT_S", "120")))
        hung = th.is_alive()
        rccl_fig = {"world": world, "error": "the library's communicator did not form / gather within its limit"} if hung else box.get("fig")
    dev_for_flags = None if one_gpu else f"cuda:{local_rank}"
    # the ranks must agree on what happens next (a rank that skips a collective the others enter would hang them): flags travel over the
    # launcher's process group, which is torch's own communicator, not the library's
    hung_any = any_rank(hung)
    comm_ok = not hung_any and not any_rank((rccl_fig or {}).get("error"))

    # one step = one wave of `conc` proofs (a batch of synthetic statements through the hot path), so any --steps the driver
    # passes measures the steady state of a full chip rather than a ragged tail
    throughput_wait(True)
    run_proofs(100000, args.warmup * conc)
    # hipEvent pairs around the launches of ONE of the `conc` provers (worker 0) during the timed region: the source of the
    # *_under_load figures.  PK_BENCH_NO_TIMED_PROFILE=1 turns it off for an A/B (profiles/r05_timed_profile_ab.json: no
    # measurable difference)
    timed_profile = args.full and os.environ.get("PK_BENCH_NO_TIMED_PROFILE") != "1"
    ctx.profile(timed_profile)
    ctx.profile_reset()
    last_step = {} if args.dump_outputs else None
    barrier()
    cpu0 = time.process_time()  # CPU seconds of every thread of this process: what the provers' host side costs (transcript, launches, waiting)
    t0 = time.perf_counter()
    run_proofs(1, args.steps * conc, last_step)
    barrier()
    own_dt = time.perf_counter() - t0
    host_cpu_ms_per_proof = 1e3 * (time.process_time() - cpu0) / (args.steps * conc)
    host_cores_busy = (time.process_time() - cpu0) / own_dt
    dt = max_over_ranks(own_dt, dist, None if one_gpu else f"cuda:{local_rank}")
    prof = ctx.profile_read()
    if last_step is not None and rank == 0:
        dump_outputs(args.dump_outputs, [(f"proof_{k:03d}", last_step[k]) for k in sorted(last_step)])
    throughput_wait(False)
    # One proof at a time on an otherwise idle chip: isolated kernel durations for the roofline, the single-stream figures, the multiplier peak.
    # Spinning waits here: the polling mode of the many-prover phases is the library's own loop and was switched off above.  (With
    # --host-wait block -- a mode of the runtime, fixed for the life of the process -- these figures were taken at the start by a FRESH process in
    # spinning mode, `ss` above: a blocked thread wakes ~20 us after its kernel, 65 times per proof, no part of a single prover's latency.)
    if args.full and ss is None and (rank == 0 or not block_wait):
        ss = single_stream_figures(torch, ctx, workers[0][1], workers[0][2], not args.no_latency_pass, args.sharded)
        ss["how"] = "this process, after the timed region, spinning waits" + (" -- NO: blocking-wait mode, a single prover pays ~20 us per synchronisation for it" if block_wait else "")
    if ss is None:
        ss = {"iso_dt": float("nan"), "lat_dt": None, "prof_iso": {}, "iso_steps": 8, "peak_modmul": 0.0, "peak_constmul": 0.0, "how": "rank 0 only"}
    iso_dt, lat_dt, prof_iso, iso_steps, peak_modmul = ss["iso_dt"], ss["lat_dt"], ss["prof_iso"], ss["iso_steps"], ss["peak_modmul"]

    # ---- secondary figures of the default line (each guarded: none may break the line) -----------------------------------
    # (b) BASELINE configs[4]: the 2^26 commit -- on one GPU, and under several ranks SHARDED over the first G = 1, 2, 4, 8 <= N of them
    # in the same invocation, so that one `--gpus N` run yields north_star's whole strong-scaling curve
    def run_commit_probe():
        if not (args.full and m == 21 and not args.sharded and not args.no_commit_probe):
            return None
        try:
            if world == 1:
                fig = commit_probe(ctx, torch, local_rank, n_vars=args.commit_log2_size)
                torch.cuda.empty_cache()
                return fig
            curve = {}
            G = 1
            while G <= world:
                takes_part = rank < G
                cctx = provekit_amd.Context(local_rank) if takes_part else None
                keep = join_subgroup(cctx, rank, G, dist, one_gpu, groups) if G > 1 else None  # noqa: F841 (kept alive)
                try:
                    curve[str(G)] = commit_probe(cctx, torch, local_rank, n_vars=args.commit_log2_size, world=G, dist=dist, one_gpu=one_gpu,
                                                 takes_part=takes_part)
                finally:
                    if takes_part:
                        if G > 1:
                            cctx.comm_destroy()
                        cctx.close()
                    torch.cuda.empty_cache()
                G *= 2
            top = str(max(int(k) for k in curve))
            fig = dict(curve[top])
            base = curve["1"]["ms_per_commit"]
            fig["curve"] = {k: {"n_gpus": v["n_gpus"], "ms_per_commit": v["ms_per_commit"], "speedup_vs_1": base / v["ms_per_commit"],
                                "achieved_GBps": v["achieved_GBps"], "frac_of_hbm_peak": v["frac_of_hbm_peak"], "transport": v["transport"],
                                "root": v["root"]} for k, v in curve.items()}
            fig["roots_agree"] = len({v["root"] for v in curve.values()}) == 1
            return fig
        except Exception as e:  # e.g. a GPU with less memory
            return {"error": str(e)[:200]}

    # (a) PCIe-inclusive rate: the same waves with the witness uploaded before every proof.  On one GPU it runs LAST, so that it cannot disturb
    # the figures above (see --size-class-probe: probes run back to back in one process were measured to depress whichever comes later)
    def run_h2d_probe():
        if not args.full or args.h2d or args.sharded or args.no_h2d_probe:
            return None
        try:
            args.h2d = True
            throughput_wait(True)
            run_proofs(200000, 2 * conc)
            barrier()
            t1 = time.perf_counter()
            run_proofs(300000, 8 * conc)
            barrier()
            return world * 8 * conc / max_over_ranks(time.perf_counter() - t1, dist, None if one_gpu else f"cuda:{local_rank}")
        except Exception as e:  # noqa: BLE001
            print(f"[bench] h2d probe failed: {e}", file=sys.stderr)
            return None
        finally:
            args.h2d = False
            throughput_wait(False)

    # Order.  One GPU: the commit probe first (before anything else allocates and releases large buffers in this process), the h2d probe last.
    # Several ranks: every figure that needs only torch's collectives first, then the sharded commit -- the one step of this file that goes
    # through the library's own RCCL communicator -- under a watchdog: if it does not come back, the line is printed without it and the
    # process leaves without another collective, so a stuck communicator can cost the run that one figure and nothing else.
    h2d_rate, sharded_fig = None, None
    if world > 1 and not comm_ok:
        h2d_rate = run_h2d_probe()  # torch's collectives only
        commit_fig = {"error": "skipped: the library's communicator did not pass its probe on every rank (see `rccl`)"}
    elif world > 1 and args.full:
        h2d_rate = run_h2d_probe()
        time.sleep(2.0)  # idle seconds after 16 provers at the power limit (see --size-class-probe)
        box = {}
        def guarded():
            torch.cuda.set_device(local_rank)  # the current device is per thread
            if os.environ.get("PK_BENCH_TEST_HANG") == "commit":  # test hook: a sharded step that never comes back
                threading.Event().wait()
            box.update(fig=run_commit_probe())
            if m == 21 and not args.no_sharded_proof and (world & (world - 1)) == 0 and world <= 16 and not (box.get("fig") or {}).get("error"):
                try:  # configs[3]: one proof of the p256 size class sharded over all ranks (every rank takes the same branch: the commit figure is rank-independent)
                    box.update(sharded=sharded_proof_probe(provekit_amd, torch, rank, local_rank, world, dist, one_gpu, groups, args.sharded_proof_log2_size))
                except Exception as e:  # noqa: BLE001
                    box.update(sharded={"error": str(e)[:300]})

        th = threading.Thread(target=guarded, daemon=True)
        th.start()
        th.join(float(os.environ.get("PK_BENCH_COMMIT_LIMIT_S", "420")))
        hung = th.is_alive()
        hung_any = any_rank(hung)
        commit_fig = {"error": "the sharded commit / proof did not return within its limit on some rank; skipped"} if hung_any else box.get("fig")
        sharded_fig = None if hung_any else box.get("sharded")
    else:
        commit_fig = run_commit_probe()  # None without --full
    if world == 1:
        h2d_rate = run_h2d_probe()
    # Everything that needs this process's provers is done.  The CPU leg will want a GPU proof to compare bytes with: take it now, then release
    # the provers -- a fresh process on a GPU where another holds two dozen idle hardware queues measures ~3.5 % low (9.9 against 9.6 ms per proof)
    cpu_seed, gpu_proof, ds0, z0 = (4242).to_bytes(32, "little"), None, workers[0][1].domain_separator, workers[0][4]
    if args.full and rank == 0 and not args.no_cpu_baseline and world == 1:
        gpu_proof = workers[0][1].prove(workers[0][2], seed=cpu_seed)
    # (c) the other BASELINE size classes (configs[2] m = 23, configs[3] m = 25), rank 0's GPU only
    if args.full and rank == 0 and m == 21 and not args.sharded and args.size_classes and not size_figs:
        for c_, prover_, d_z_, r1cs_, _ in workers:
            prover_.close()
            d_z_.free()
            r1cs_.close()
            c_.close()
        workers.clear()
        torch.cuda.empty_cache()
        size_figs = run_size_classes()
    if dist is not None and not hung_any:
        dist.barrier()

    if rank == 0:
        line = {
            "metric": "proofs/sec (noir-r1cs prove hot path, WHIR commit + sumcheck + folding rounds)",
            "value": (1 if args.sharded else world) * args.steps * conc / dt,
            "unit": "proofs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True,
            "scaling": "strong" if args.sharded else "weak",
            "vs_baseline": None,
            "dtype": "u32x8 (BN254-Fr, 256-bit Montgomery integers)",
            "data": "synthetic",
            "config": {
                "workload": f"poseidon-rounds size class: m={m}, m_0={m_0}, satisfiable synthetic R1CS ({nc} constraints, {n_wit} witnesses, a constant term in half of the rows of A and B), batch-2 WHIR commit + zk-sumcheck + {cfg_w.n_rounds}-round WHIR opening, "
                            f"queries {cfg_w.num_queries}/{cfg_w.final_queries}, pow_bits {cfg_w.pow_bits}/{cfg_w.final_pow_bits} (WhirConfig::new derivation, security 128, "
                            f"ConjectureList), blinding WHIR n={cfg_b.n_vars} queries {cfg_b.num_queries}/{cfg_b.final_queries}, Skyscraper-sponge transcript, ChaCha12 masks",
                "proofs_per_step": conc * (1 if args.sharded else world),
                "host_wait": ({"block": "blocking (pk_device_set_host_wait: the provers' host threads sleep on the completion interrupt)",
                               "poll": "polling (pk_device_set_host_wait PK_WAIT_POLL: the library's own query-and-sleep loop)", "spin": "spinning (HIP default)"}[wait_mode])
                             + f"; {cores['usable']} usable host cores (logical {cores['logical_cpus']}, cgroup quota {cores['cgroup_cpu_quota']}) for {local_world} rank(s) on this node",
                "host_cpu_ms_per_proof": round(host_cpu_ms_per_proof, 2),
                "host_cores_busy_in_timed_region": round(host_cores_busy, 2),
                "profiling_in_timed_region": (f"hipEvent pairs around the launches of 1 of the {conc} provers per GPU" if timed_profile else False),
                "launcher": ("bench.py --gpus N started its own ranks (torch.distributed.run, 127.0.0.1)" if os.environ.get("PK_BENCH_SELF_LAUNCHED") else
                             ("torch.distributed.run" if dist is not None else "single process")),
                "parallelism": (f"one step = one proof, sharded over {world} GPU(s): every commit of >= 64 rows per rank split by leaf index, "
                                "RCCL all-gather of leaf digests + all-reduce of opened rows behind the C ABI; the rest of the proof is "
                                "replicated on every rank") if args.sharded else f"one step = one wave of {conc} proofs per GPU; {world} GPU(s) x {conc} concurrent provers per GPU, work handed out "
                               f"dynamically (independent proofs, no collective; "
                               f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')})"
                               + (", witness uploaded over PCIe before every proof (--h2d)" if args.h2d else ""),
            },
        }
        if args.full:
            # roofline of the dominant kernel (leaf_hash): algorithmic bytes per launch / measured avg duration
            bytes_step, launches_step, compresses_step = leaf_hash_bytes([(m, 2, cfg_w.n_rounds), (cfg_b.n_vars, 2, cfg_b.n_rounds)])
            n_l, ms_l = prof.get("leaf_hash", (0, 0.0))
            avg_ms = ms_l / max(n_l, 1)  # in the timed region: a launch shares the chip with the other provers' kernels
            achieved_load = (bytes_step / launches_step) / (avg_ms * 1e-3) / 1e9 if n_l else 0.0
            n_i, ms_i = prof_iso.get("leaf_hash", (0, 0.0))
            iso_avg_ms = ms_i / max(n_i, 1)  # the kernel by itself (one proof at a time, same process, same hipEvent timing)
            achieved = (bytes_step / launches_step) / (iso_avg_ms * 1e-3) / 1e9 if n_i else 0.0
            step_bytes = proof_algorithmic_bytes(m, m_0, n_wit, cfg_w, cfg_b) * conc
            # HBM bytes per launch come from rocprofv3 PMC passes (tools/pmc.sh: separate FETCH_SIZE / WRITE_SIZE runs, FETCH doubled
            # for gfx950 as the microarch guide prescribes); counters cannot be read from inside this process.  A committed summary is
            # used ONLY if it was taken with this very binary (sha256 of libprovekit_hip.so recorded by the tool) on this workload
            # size; otherwise the field is null rather than a stale number.
            traffic, valu_busy = None, None
            try:
                import glob
                import hashlib

                lib_sha = hashlib.sha256(open(provekit_amd.LIB_PATH, "rb").read()).hexdigest()[:16]
                for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_leaf_hash.json"))):
                    pmc = json.load(open(fn))
                    if pmc.get("lib_sha16") == lib_sha and pmc.get("m") == m:
                        traffic = pmc["traffic_bytes_per_launch"]
                        valu_busy = pmc.get("valu_busy_pct_largest_launch")
            except Exception:
                pass
            iso_leaf_ms = prof_iso.get("leaf_hash", (1, 0.0))[1] / max(prof_iso.get("leaf_hash", (1, 0.0))[0], 1)
            # per-proof kernel time by stage, from the one-proof-at-a-time pass (in the timed region a prover's kernels share the
            # chip with the other provers', so their elapsed times there say little about the work)
            stage_ms = {k: round(v[1] / iso_steps, 4) for k, v in sorted(prof_iso.items(), key=lambda kv: -kv[1][1])}
            line.update({
                "roofline": {
                    "kernel": "leaf_hash_kernel (Skyscraper leaf digests)",
                    "bound": "hbm",
                    "achieved": achieved,
                    "peak": HBM_PEAK_GBS,
                    "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS,
                    "traffic": traffic,
                    "traffic_note": ("replayed from the rocprofv3 PMC summary under profiles/ taken with this exact binary (sha256 match), not "
                                     "measured by this run") if traffic is not None else "no PMC summary of this binary under profiles/",
                    "algorithmic_bytes_per_launch": bytes_step / launches_step,
                    "launches_per_proof": launches_step,
                    "launches_per_step": launches_step * conc,
                    "avg_launch_ms": iso_avg_ms,
                    "achieved_under_load": achieved_load,
                    "frac_under_load": achieved_load / HBM_PEAK_GBS,
                    "avg_launch_ms_under_load": avg_ms,
                    "note": "integer-ALU bound (14 Montgomery squarings per compression, DESIGN.md 4).  achieved / frac / avg_launch_ms: the "
                            "kernel by itself, hipEvent pairs around every launch on the work stream with one proof in flight (the figure rocprofv3 "
                            f"--kernel-trace reports at concurrency 1); *_under_load: the same launches inside the timed region, where {conc} provers' "
                            "kernels share the chip, so it falls as throughput rises",
                    "alu": {
                        "achieved": 14.0 * (compresses_step / launches_step) / max(iso_leaf_ms * 1e-3, 1e-12) / 1e12,
                        "peak": peak_modmul / 1e12 if peak_modmul else None,
                        "unit": "T modmul/s",
                        "frac": 14.0 * (compresses_step / launches_step) / max(iso_leaf_ms * 1e-3, 1e-12) / peak_modmul if peak_modmul else None,
                        "valu_busy_pct_largest_launch": valu_busy,
                        "note": "isolated launches; achieved counts only the 14 Montgomery squarings of each compression (the 4 bars, "
                                "18 round-constant additions/reductions and the layout conversion are extra work on the same VALUs); peak = "
                                "pk_probe_modmul_rate, register-resident squaring chains, best of 2/4/8 waves per SIMD x ILP 1/2",
                    },
                },
                # every kernel's algorithmic bytes (SURVEY 8d per-unit figures, proof_algorithmic_bytes) over the step's wall time
                "step_algorithmic_GBps": step_bytes / (dt / args.steps) / 1e9,
                "step_algorithmic_bytes": step_bytes,
                # BASELINE.json's metric also asks for achieved HBM GB/s on the WHIR NTT: algorithmic bytes = 64 B per codeword
                # element (one logical read + write) over the measured time of all encode kernels of a proof
                "roofline_ntt": ntt_roofline(prof_iso, iso_steps, m, cfg_w, cfg_b, ss.get("peak_constmul") or None),
                "single_stream": {"ms_per_proof": 1e3 * iso_dt, "proofs_per_s": 1.0 / iso_dt,
                                  "latency_mode_ms_per_proof": None if lat_dt is None else 1e3 * lat_dt,
                                  "note": "one proof at a time; latency_mode = pk_ctx_set_latency_mode (sumcheck rounds enqueued one ahead "
                                          "behind a host-published gate; same transcript); measured in " + ss["how"]},
                "stage_ms_per_proof_isolated": stage_ms,
            })
        if h2d_rate is not None:
            line["h2d_inclusive_proofs_per_s"] = h2d_rate
            line["h2d_note"] = (f"same workload, {conc} provers, the 32 x {n_wit} B witness uploaded from pageable host memory before every proof; "
                                "never `value` (inputs are resident when the clock starts)")
        if rccl_fig is not None:
            line["rccl"] = rccl_fig
        if commit_fig is not None:
            line["commit_2p26" if args.commit_log2_size == 26 else f"commit_2p{args.commit_log2_size}"] = commit_fig
        if sharded_fig is not None:
            line[f"sharded_proof_m{args.sharded_proof_log2_size}"] = sharded_fig
        if size_figs:
            line["size_classes"] = size_figs
        if args.full and not args.no_cpu_baseline and world == 1:
            cb = cpu_baseline(m, m_0, mats0, interner0, nc, n_wit, cfg_w, cfg_b, ds0, z0, cpu_seed, gpu_proof, budget_s=args.cpu_baseline_budget)
            line["cpu_baseline"] = {
                "value": 1.0 / cb["seconds"],
                "unit": "proofs/s",
                "cores": cb["cores"],
                "kind": "port",
                "sample": f"1 whole proof (a step is {conc} of them) of the same statement (m={m}) through oracle/prover_ref.py + oracle/pk_oracle.c: both commitments, the "
                          f"zk sumcheck with its blinding algebra, the blinding WHIR, external rows and sums, the {cfg_w.n_rounds}-round witness WHIR with proof of work and "
                          "STIR openings, and the Skyscraper-sponge transcript -- the reference's prove end to end (whir_r1cs.rs:42-100); OpenMP wherever the reference uses "
                          "rayon, sparse products serial as in the reference; same 32-byte key as a GPU proof of this run",
                "matches_gpu_transcript": cb["matches_gpu_transcript"],
                "proof_bytes": cb["proof_bytes"],
                "stage_s": cb["stage_s"],
                "by_threads": {k: ({"proofs_per_s": v["proofs_per_s"], "s_per_proof": v["s_per_proof"]} if "s_per_proof" in v else v) for k, v in cb["threads"].items()},
                "host": cb["host"],
                "cores_note": "cores = what this process may use: min(logical CPUs, affinity, cgroup CPU quota) -- OpenMP threads beyond the quota are throttled and "
                              "make the run slower (tools/cpu_scaling.py, profiles/r05_cpu_scaling.json)",
            }
        emit(line)
    if hung_any:
        sys.stderr.flush()
        os._exit(0)  # a thread of this process (or of a peer) is still inside the stuck collective: no orderly teardown
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
