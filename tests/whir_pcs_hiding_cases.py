"""Shared by test_whir_pcs_hiding_host.py and test_gpu_whir_pcs_hiding.py: configs that keep the mask budget, the extended tables
[f_b || mask_b] and g built on the CPU from oracle/prover_ref.py's random_fe, and the hiding opening the ORACLE prover builds over
them (whir_pcs_cases.oracle_opening at the points (0, z) under the hiding pattern).  One Case per shape is built once and shared."""
import os
import re

import whir_pcs_cases as K

ROOT = K.ROOT
# (n + 1, B, q): the committed config has n + 1 variables and B + 1 polynomials; the caller's B polynomials have n
SHAPES = [(8, 1, 1), (8, 3, 3), (12, 1, 3), (12, 2, 1)]
KEY = bytes(range(32))
LABEL = b"provekit-hip/whir-pcs-hiding/v1"


def streams():
    """(PKW_RNG_MASK0, PKW_RNG_G) as csrc/rng_core.hpp states them, and csrc/internal.hpp's RNG_* numbers"""
    src = open(os.path.join(ROOT, "provekit_amd", "csrc", "rng_core.hpp")).read()
    m = re.search(r"PKW_RNG_MASK0 = (\d+), PKW_RNG_G = (\d+)", src)
    proof = re.search(r"enum \{ (RNG_MASK = .*?) \}", open(os.path.join(ROOT, "provekit_amd", "csrc", "internal.hpp")).read()).group(1)
    return int(m.group(1)), int(m.group(2)), [int(x) for x in re.findall(r"= (\d+)", proof)]


def budget(cfg):
    """the values of each masked polynomial that leave through the proof, and the mask coefficients there are"""
    return cfg.commitment_ood_samples + (cfg.num_queries[0] << cfg.folding_factor), 1 << (cfg.n_vars - 1)


def hiding_config(n1, B):
    """small_config(n + 1, B + 1) with num_queries[0] lowered until the mask budget holds (6 queries at n + 1 = 8: 96 + 1 <= 128)"""
    c = K.small_config(n1, B + 1)
    q = list(c.num_queries)
    q[0] = min(q[0], ((1 << (n1 - 1)) - c.commitment_ood_samples) >> c.folding_factor)
    c.num_queries = q
    left, have = budget(c)
    assert 0 < left <= have
    return c


def extended_tables(n, B, key=KEY, seed=3):
    """-> (f: B tables of 2^n canonical ints, extended: B + 1 tables of 2^(n+1) canonical ints, draws: the B + 1 raw draws).  A
    drawn word is stored as it is, i.e. it IS the Montgomery form of the table's entry"""
    import prover_ref as PR

    mask0, g, _ = streams()
    f = K.polynomials(n, B, seed)
    draws = [PR.random_fe(key, mask0 + b, 1 << n) for b in range(B)] + [PR.random_fe(key, g, 2 << n)]
    ext = [f[b] + PR.unmont_many(draws[b]) for b in range(B)] + [PR.unmont_many(draws[B])]
    return f, ext, draws


class Case:
    def __init__(self, oracle, n1, B, q, key=KEY, hash_version=2, lead=0):
        from provekit_amd import whir_pcs

        self.n1, self.n, self.B, self.q = n1, n1 - 1, B, q
        self.cfg = hiding_config(n1, B)
        self.f, self.ext, self.draws = extended_tables(self.n, B, key)
        self.pts = K.points(self.n, q)
        self.mpts = K.mont_points(oracle, self.pts)
        self.ext_pts = [[lead] + p for p in self.pts]
        self.pattern = whir_pcs.io_pattern_hiding(self.cfg, q)
        self.proof, self.root, self.vals = K.oracle_opening(oracle, self.cfg, self.ext, self.ext_pts, self.pattern, hash_version)
        self.expected = K.expected_evals(self.f, self.pts)  # f_b(z_i)
        self.eval_offset = 32 + 32 * self.cfg.commitment_ood_samples * (B + 1) + 32 * q * n1

    def verify(self, proof=None, **kw):
        from provekit_amd import whir_pcs

        kw.setdefault("expected_root", self.root)
        pts = kw.pop("points", self.mpts)
        return whir_pcs.verify_hiding(self.cfg, pts, self.proof if proof is None else proof, **kw)


_cases = {}


def case(oracle, shape):
    """the shape's case under KEY and hash version 2, built once per process"""
    if shape not in _cases:
        _cases[shape] = Case(oracle, *shape)
    return _cases[shape]
