"""Shared by test_whir_pcs_linear_host.py and test_gpu_whir_pcs_linear.py: deterministic dense weight tables and tags, and a
linear-statement opening built on the CPU from the oracle prover's parts, as whir_pcs_cases.oracle_opening builds the evaluation
statement's (oracle/prover_ref.py, imported, not edited)."""
import struct

import numpy as np

import whir_pcs_cases as K

P = K.P
# (n_vars, batch, q, l): one point-free statement per size, one with every count above one, the widest weight count
SHAPES = [(8, 1, 0, 1), (8, 2, 2, 3), (12, 1, 1, 2), (12, 2, 0, 16)]


def weight_tables(oracle, n_vars, l, eq_point=None, seed=21):
    """l tables as canonical ints: random values with 0, 1 and p - 1 planted; with l >= 2 the second is all zero; with l >= 3 the
    third is eq_table(eq_point) (default: the first of K.points(n_vars, 1))"""
    out = []
    for i in range(l):
        w = K.random_ints(1 << n_vars, seed + 31 * i)
        w[0], w[-1] = P - 1, 0
        if len(w) > 2:
            w[1] = 1
        out.append(w)
    if l >= 2:
        out[1] = [0] * (1 << n_vars)
    if l >= 3:
        pt = eq_point or K.points(n_vars, 1)[0]
        out[2] = oracle.limbs_to_ints(oracle.from_mont(oracle.eq_table(oracle.to_mont(oracle.ints_to_limbs(pt)))))
    return out


def tags(l, seed=9):
    t = K.random_ints(l, seed)
    for i, special in enumerate((0, 1, P - 1)):
        if i + 1 < l:
            t[i + 1] = special
    return t


def mont(oracle, ints):
    return oracle.to_mont(oracle.ints_to_limbs(ints))


def expected_sums(polys, weights):
    return [[sum(a * b for a, b in zip(w, f)) % P for w in weights] for f in polys]


def oracle_linear_opening(oracle, cfg, polys, pts, weights, tag_ints, pattern, hash_version=2, prove_weights=None, claimed_sums=None):
    """The transcript pkw_open_linear writes, from the oracle's parts: Merlin over `pattern`, commit, commit_transcript, the points,
    the tags, the evaluations and the sums absorbed, whir_prove with the weight list [eq tables..., weight tables...].
    prove_weights / claimed_sums let a test build a DISHONEST proof (WHIR run over other tables than the tags stand for).
    -> (proof bytes, root bytes, evaluations, sums)"""
    import prover_ref as PR

    n, N = cfg.n_vars, 1 << cfg.n_vars
    vc = K.vcfg(cfg)
    tm = PR.Timers()
    T = PR.Merlin(pattern)
    com = PR.Commitment()
    com.evals = [PR.mont_many(p) for p in polys]
    com.polys = [oracle.to_coeffs(e, n) for e in com.evals]

    def commit(c, ps, tm_):  # prover_ref.commit with the hash version as a parameter (its own is fixed at 2)
        leaves = oracle.rs_encode(ps[0] if len(ps) == 1 else np.concatenate(ps), len(ps), c.n_vars, c.starting_log_inv_rate, c.folding_factor)
        return leaves, oracle.merkle_commit(leaves, hash_version), leaves.shape[0], leaves.shape[1]

    saved = PR.commit
    PR.commit = commit
    try:
        com.tree = PR.commit(vc, com.polys, tm)
        PR.commit_transcript(T, vc, com, tm)
        if pts:
            T.add_scalars([x for p in pts for x in p])
        T.add_scalars(list(tag_ints))
        vals = K.expected_evals(polys, pts)
        if pts:
            T.add_scalars([v for row in vals for v in row])
        sums = expected_sums(polys, weights) if claimed_sums is None else claimed_sums
        T.add_scalars([v for row in sums for v in row])
        tables = [oracle.eq_table(mont(oracle, p)) for p in pts] + [PR.mont_many(w) for w in (prove_weights or weights)]
        PR.whir_prove(T, vc, com, tables, [N] * len(tables), tm)
    finally:
        PR.commit = saved
    assert T.finished(), "the proof ended before its IO pattern did"
    return bytes(T.out), com.tree[1][1].tobytes(), vals, sums


def deferred_offset(proof, count):
    """byte offset of the first deferred value: the last hint is u32 length, u64 count, count = q + l elements"""
    off = len(proof) - 32 * count
    assert struct.unpack_from("<I", proof, off - 12)[0] == 8 + 32 * count and struct.unpack_from("<Q", proof, off - 8)[0] == count
    return off
