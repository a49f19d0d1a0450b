"""Shared by test_whir_pcs_host.py and test_gpu_whir_pcs*.py: small WHIR configs, deterministic polynomials and points, an
opening proof built on the CPU from the oracle prover's parts (oracle/prover_ref.py, imported, not edited), and the device tests'
size labels and pointer arrays."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from whir_pcs_helpers import ptrs  # noqa: E402,F401  (tools/: one definition for the bench tools and the device tests)

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# (n_vars, batch, q): n_vars = 8 is fold 4 with one WHIR round, 12 has two; the sizes the CPU suite's other provers use
SHAPES = [(8, 1, 1), (8, 2, 3), (12, 1, 3), (12, 2, 1)]


def small_config(n_vars, batch):
    """pk_whir_config_derive with cheap grinding and few queries, as tests/test_verify_host.py does for its cases"""
    from provekit_amd.scheme import WhirConfig

    c = WhirConfig.derive(n_vars, batch_size=batch)
    c.pow_bits = [4.0] * c.n_rounds
    c.final_pow_bits = 4.0
    c.num_queries = [20, 12, 9, 8][: c.n_rounds]
    return c


def vcfg(c):
    import verifier as V

    return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, list(c.num_queries), list(c.ood_samples), list(c.pow_bits),
                        c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)


def random_ints(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % P for _ in range(n)]


def many_ints(n, seed):
    """random_ints for large n: one draw of 40 n bytes cut into n values (other values than random_ints gives for the seed)"""
    raw = np.random.default_rng(seed).bytes(40 * n)
    return [int.from_bytes(raw[40 * i : 40 * i + 40], "little") % P for i in range(n)]


def polynomials(n_vars, batch, seed=3):
    """evaluation tables as canonical ints; 0, 1 and p - 1 among the random values"""
    out = []
    for b in range(batch):
        v = random_ints(1 << n_vars, seed + 100 * b)
        v[0] = 0
        v[-1] = P - 1
        if len(v) > 2:
            v[1] = 1
        out.append(v)
    return out


def points(n_vars, q, seed=5):
    """q points; coordinates 0, 1 and p - 1 next to random ones; with q >= 3 the last point repeats the first"""
    pts = [random_ints(n_vars, seed + 7 * i) for i in range(q)]
    for i, special in enumerate((0, 1, P - 1)):
        if i < q:
            pts[i][(3 * i) % n_vars] = special
    if q >= 3:
        pts[-1] = list(pts[0])
    return pts


def mont_points(oracle, pts):
    return np.stack([oracle.to_mont(oracle.ints_to_limbs(p)) for p in pts])


def expected_evals(polys, pts):
    import verifier as V

    return [[V.mle_eval_table(poly, pt) for pt in pts] for poly in polys]


def oracle_opening(oracle, cfg, polys, pts, pattern, hash_version=2, weight_points=None, claimed=None):
    """The transcript pkw_open writes, from the oracle's parts: Merlin over `pattern`, commit, commit_transcript, the points and
    the evaluations absorbed, whir_prove with the eq tables as weights.  weight_points / claimed let a test build a DISHONEST
    proof (weights of other points than the ones absorbed; other evaluations).  -> (proof bytes, root bytes, evaluations)"""
    import prover_ref as PR

    n, N = cfg.n_vars, 1 << cfg.n_vars
    vc = vcfg(cfg)
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
        T.add_scalars([x for p in pts for x in p])
        vals = expected_evals(polys, pts) if claimed is None else claimed
        T.add_scalars([v for row in vals for v in row])
        weights = [oracle.eq_table(oracle.to_mont(oracle.ints_to_limbs(p))) for p in (weight_points or pts)]
        PR.whir_prove(T, vc, com, weights, [N] * len(weights), tm)
    finally:
        PR.commit = saved
    assert T.finished(), "the proof ended before its IO pattern did"
    return bytes(T.out), com.tree[1][1].tobytes(), vals


# ---- what the device tests of the three statement forms share (test_gpu_whir_pcs*.py) ---------------------------------------------------
def low_vars():
    """log2 of the elements one workgroup covers per step, in the evaluation (its tile) and in the weighted sums (the grid has one
    workgroup up to there, two above)"""
    import pk_probes
    from provekit_amd import whir_pcs

    b = next(n for n in range(1, 31) if pk_probes.lib.pk_probe_whir_wsum_grid(n) == 2) - 1
    assert b == whir_pcs.low_vars() == 8  # the tests' sizes straddle it; a library with another tile or step needs another look at them
    return b


def resolve_n(label):
    """a size label of a parametrised test -> n_vars"""
    b = low_vars()
    return {"0": 0, "1": 1, "4": 4, "b-1": b - 1, "b": b, "b+1": b + 1, "13": 13}[label]


def deferred_offset(proof, q):
    """byte offset of the first deferred value: the last hint is u32 length, u64 count, q elements"""
    off = len(proof) - 32 * q
    assert struct.unpack_from("<I", proof, off - 12)[0] == 8 + 32 * q and struct.unpack_from("<Q", proof, off - 8)[0] == q
    return off
