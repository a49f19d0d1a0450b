"""Shared by test_whir_pcs_configs_host.py and test_gpu_whir_pcs_configs.py: a grid over the WHIR configs libprovekit_whir.so accepts
(every fold at its size edges, rates above 1/2, batches 3 and 4, no folding round, a final sumcheck, 0..4 OOD samples, grinding at
each position alone, more than 32 weights in one combination), the oracle prover's opening of every entry with the STIR index counts
it drew (oracle/prover_ref.py, imported, not edited), and a walker that names the regions of an opening proof."""
import struct

import whir_pcs_cases as K
import whir_pcs_linear_cases as L
import whir_pcs_sparse_cases as S

DEFAULT_QUERIES = [7, 5, 4, 3, 3, 3, 3, 3, 3]
GRIND_BITS = 3.0  # a solve is a few hundred hashes


def config(n, fold, rate, batch, rounds=None, ood=None, commitment_ood=None, grind=True, queries=None, final_folding_pow=None):
    """pk_whir_config_derive's shape for (n, fold, rate, batch) with the round count kept or cut and every count small"""
    from provekit_amd.scheme import WhirConfig

    c = WhirConfig.derive(n, batch_size=batch, folding_factor=fold, starting_log_inv_rate=rate)
    r = c.n_rounds if rounds is None else rounds
    c.num_queries = list(queries or DEFAULT_QUERIES)[:r]
    assert len(c.num_queries) == r, "a query count for every round"
    c.ood_samples = [1 if ood is None else ood] * r
    c.pow_bits = [GRIND_BITS if grind else 0.0] * r
    c.final_queries = 4
    c.final_pow_bits = GRIND_BITS if grind else 0.0
    c.commitment_ood_samples = 1 if commitment_ood is None else commitment_ood
    c.final_folding_pow_bits = 0.0 if final_folding_pow is None else final_folding_pow
    return c


class Entry:
    """one grid entry: config()'s arguments, the number of points opened, and for the single-position grinding variants the one
    field that grinds (`only`: "round0", "final" or "final_folding")"""

    def __init__(self, n, fold, rate, batch, q=2, only=None, **kw):
        self.args, self.kw, self.q, self.only = (n, fold, rate, batch), kw, q, only
        self.n, self.fold, self.rate, self.batch = n, fold, rate, batch
        parts = [f"n{n}", f"k{fold}", f"r{rate}", f"b{batch}"] + [f"{k}={v}" for k, v in sorted(kw.items())]
        self.id = "-".join(parts + ([f"q{q}"] if q != 2 else []) + ([f"only-{only}"] if only else []))

    def cfg(self):
        c = config(*self.args, **self.kw)
        if self.only:
            assert not self.kw.get("grind", True) and not any(c.pow_bits) and not c.final_pow_bits and not c.final_folding_pow_bits
            if self.only == "round0":
                c.pow_bits[0] = GRIND_BITS
            elif self.only == "final":
                c.final_pow_bits = GRIND_BITS
            else:
                c.final_folding_pow_bits = GRIND_BITS
        return c

    def final_vars(self):
        c = self.cfg()
        return c.n_vars - c.folding_factor * (c.n_rounds + 1)

    def __repr__(self):
        return self.id


# every fold at its size edges: n = k, k + 1, 2k, 2k + 1, 3k + 2 at rate 1/2, one polynomial, the derived round count
FOLD_EDGES = [Entry(n, k, 1, 1) for k in (1, 2, 3, 4) for n in sorted({k, k + 1, 2 * k, 2 * k + 1, 3 * k + 2})]
FINAL_SUMCHECK = Entry(9, 2, 1, 2, rounds=1)  # five final variables
NO_OOD = Entry(6, 2, 2, 3, ood=0, commitment_ood=0, grind=False)
TWO_LEAVES = Entry(3, 1, 1, 1)  # two rounds at fold 1: the last tree has two leaves, both opened
MIXED = [
    NO_OOD,
    Entry(7, 3, 3, 4, ood=2, commitment_ood=2),
    Entry(9, 4, 2, 3, ood=4, commitment_ood=4),
    FINAL_SUMCHECK,
    Entry(10, 4, 1, 4, rounds=0, grind=False),  # no folding round; six final variables
    Entry(5, 1, 1, 2, rounds=2),
    Entry(8, 1, 3, 1),  # seven rounds at a constant rate
    Entry(9, 1, 1, 1),  # eight rounds
    Entry(6, 2, 1, 2, final_folding_pow=2.0),
]
SINGLE_GRIND = [Entry(8, 4, 1, 1, grind=False, only=o) for o in ("round0", "final", "final_folding")]
# the initial combination's weight count (points + commitment OOD samples) on both sides of eq_weights' chunk of 32, and the most
INITIAL_WEIGHTS = [(Entry(5, 2, 1, 2, q=q, commitment_ood=co), q + co) for q, co in ((31, 1), (32, 1), (28, 4), (29, 4), (64, 4))]
assert [w for _, w in INITIAL_WEIGHTS] == [32, 33, 32, 33, 68]
# a round's weight count (one OOD sample + the distinct STIR indexes) on both sides of the chunk: (entry, distinct indexes in round 0)
ROUND_WEIGHTS = [(Entry(8, 4, 2, 1, q=1, queries=[nq]), d) for nq, d in ((36, 30), (37, 31), (39, 32), (42, 33))]
ALL_ROWS = Entry(8, 4, 1, 1, queries=[400])  # every one of the initial tree's 32 rows opened
GRID = FOLD_EDGES + MIXED + SINGLE_GRIND + [e for e, _ in INITIAL_WEIGHTS] + [e for e, _ in ROUND_WEIGHTS] + [ALL_ROWS]
assert len({e.id for e in GRID}) == len(GRID)
assert TWO_LEAVES.id in {e.id for e in FOLD_EDGES}

HASH_V1 = [Entry(5, 2, 1, 1), Entry(7, 3, 3, 4, ood=2, commitment_ood=2), Entry(9, 4, 2, 3, ood=4, commitment_ood=4)]
TAMPERED = [FINAL_SUMCHECK, NO_OOD, TWO_LEAVES]
# the linear and the sparse statements: (entry, q, l)
LINEAR_COUNTS = [(0, 1), (2, 3), (1, 16)]
LINEAR = [Entry(2, 2, 1, 1), Entry(5, 1, 1, 2), Entry(7, 3, 3, 4, ood=2, commitment_ood=2), FINAL_SUMCHECK, NO_OOD]

# the bounds of the family: (what, the refused config's Entry arguments, the accepted neighbour's, is the neighbour small enough to open)
BOUNDS = [
    ("fold 5 | 4", ((10, 5, 1, 1), dict(rounds=0)), ((10, 4, 1, 1), dict(rounds=0)), True),
    ("n + rate = 29 | 28", ((27, 4, 2, 1), {}), ((26, 4, 2, 1), {}), False),
    ("a final polynomial of 17 | 16 variables", ((21, 4, 1, 1), dict(rounds=0)), ((20, 4, 1, 1), dict(rounds=0)), False),
    ("fold * (rounds + 1) = n + 1 | n", ((7, 2, 1, 1), dict(rounds=3)), ((8, 2, 1, 1), dict(rounds=3)), True),
    # n + rate = rounds + fold needs fold * (rounds + 1) > n as well (rate >= 1), so the round rule speaks first: a refusal all the same
    ("a round's tree of one leaf | two", ((3, 1, 1, 1), dict(rounds=3)), ((3, 1, 1, 1), dict(rounds=2)), True),
    ("5 | 4 OOD samples per round", ((8, 4, 1, 1), dict(ood=5)), ((8, 4, 1, 1), dict(ood=4)), True),
    ("5 | 4 OOD samples per commitment", ((8, 4, 1, 1), dict(commitment_ood=5)), ((8, 4, 1, 1), dict(commitment_ood=4)), True),
    ("batch 5 | 4", ((6, 2, 1, 5), {}), ((6, 2, 1, 4), {}), True),
]


def recording_stir_queries(fn):
    """fn() with prover_ref.stir_queries wrapped, as oracle_opening wraps prover_ref.commit -> (fn's result, [(asked, distinct,
    rows of the opened tree)] per call: the rounds in order, then the final openings)"""
    import prover_ref as PR

    counts = []
    saved = PR.stir_queries

    def stir_queries(T, domain_size, fold, nq):
        idx = saved(T, domain_size, fold, nq)
        counts.append((nq, len(idx), domain_size >> fold))
        return idx

    PR.stir_queries = stir_queries
    try:
        return fn(), counts
    finally:
        PR.stir_queries = saved


class Opening:
    """the oracle prover's opening of one entry at entry.q points, built once per (entry, hash version)"""

    def __init__(self, oracle, entry, hash_version=2):
        from provekit_amd import whir_pcs

        self.entry, self.cfg, self.q, self.hash_version = entry, entry.cfg(), entry.q, hash_version
        self.n, self.batch = entry.n, entry.batch
        self.polys = K.polynomials(self.n, self.batch)
        self.pts = K.points(self.n, self.q)
        self.mpts = K.mont_points(oracle, self.pts)
        self.pattern = whir_pcs.io_pattern(self.cfg, self.q)
        (self.proof, self.root, self.vals), self.counts = recording_stir_queries(
            lambda: K.oracle_opening(oracle, self.cfg, self.polys, self.pts, self.pattern, hash_version=hash_version))
        assert len(self.counts) == self.cfg.n_rounds + 1


class LinearOpening:
    """the oracle prover's opening of one entry at q points and l weights: whir_pcs_sparse_cases.weights as index/value lists and
    as the dense tables they stand for (one statement, one transcript)"""

    def __init__(self, oracle, entry, q, l):
        from provekit_amd import whir_pcs

        self.entry, self.cfg, self.q, self.l = entry, entry.cfg(), q, l
        self.n, self.batch = entry.n, entry.batch
        self.polys = K.polynomials(self.n, self.batch)
        self.pts = K.points(self.n, q) if q else []
        self.mpts = K.mont_points(oracle, self.pts) if q else None
        self.ws = S.weights(self.n, l)
        assert all(len(idx) <= 1 << self.n and all(i < 1 << self.n for i in idx) for idx, _ in self.ws)
        self.dense = [S.densify(self.n, w) for w in self.ws]
        self.mdense = [L.mont(oracle, w) for w in self.dense]
        self.tags = L.tags(l)
        self.mtags = L.mont(oracle, self.tags)
        self.pattern = whir_pcs.io_pattern_linear(self.cfg, q, l)
        self.proof, self.root, self.vals, self.sums = L.oracle_linear_opening(oracle, self.cfg, self.polys, self.pts, self.dense, self.tags, self.pattern)
        assert self.sums == S.sums(self.polys, self.ws)


_cache = {}


def opening(oracle, entry, hash_version=2):
    key = (entry.id, hash_version)
    if key not in _cache:
        _cache[key] = Opening(oracle, entry, hash_version)
    return _cache[key]


def linear_opening(oracle, entry, q, l):
    key = (entry.id, "linear", q, l)
    if key not in _cache:
        _cache[key] = LinearOpening(oracle, entry, q, l)
    return _cache[key]


# ---- the device buffers of an opening ----------------------------------------------------------------------------------------------------
def opening_buffers(cfg):
    """{name: field elements} of every buffer Opening::run (csrc/whir_pcs/pcs.cpp) takes from the arena for a config of at most 17
    variables, written down from its steps and not from plan(): the arena is their sum, each rounded up to 8 elements"""
    n, k, batch, N = cfg.n_vars, cfg.folding_factor, cfg.batch_size, 1 << cfg.n_vars
    assert n <= 17

    def eval_partials(polys):  # one partial per polynomial, point of a pass of 8 and workgroup; one workgroup per 2^8 elements
        return polys * 8 * (1 << max(n - 8, 0))

    def commit_scratch(nv, rate, width_batch):  # two codewords: pk_commit_sizes' rule outside a device set
        return 2 * (1 << (nv + rate - k)) * (width_batch << k)

    out = {"points": 64 * n, "evaluation partials": eval_partials(batch), "evaluations": 64 * batch, "coefficients": N, "p": N, "p half": N // 2, "w": N,
           "w half": N // 2}
    scratch = max(commit_scratch(n, cfg.starting_log_inv_rate, batch), eval_partials(4))  # a linear opening's deferred evaluations: 4 tables a launch
    nv, rate = n, cfg.starting_log_inv_rate
    for r in range(cfg.n_rounds):
        nv, rate = nv - k, rate + k - 1
        rows = 1 << (nv + rate - k)
        out[f"round {r} polynomial"], out[f"round {r} leaves"], out[f"round {r} nodes"] = 1 << nv, rows << k, 2 * rows
        scratch = max(scratch, commit_scratch(nv, rate, 1))
    out["final coefficients"] = 1 << (nv - k)
    out["scratch"] = scratch
    return out


def arena_fes(cfg):
    return sum((max(v, 1) + 7) // 8 * 8 for v in opening_buffers(cfg).values())


# ---- the layout of an opening proof ----------------------------------------------------------------------------------------------------
def walk(proof, cfg, q, l=0):
    """[(name, start, end)] of every region of an opening proof, in order, found by walking the config (a scalar is 32 bytes, a
    nonce 8, a hint a u32 length and its payload); regions of no bytes are listed too.  Ends at the proof's end or asserts"""
    regions = []
    i = 0

    def region(name, size):
        nonlocal i
        regions.append((name, i, i + size))
        i += size

    def hint(name):
        assert i + 4 <= len(proof), f"the proof ends inside {name}"
        (ln,) = struct.unpack_from("<I", proof, i)
        region(name, 4 + ln)

    def nonce(name, bits):
        region(name, 8 if bits > 0 else 0)

    k, batch = cfg.folding_factor, cfg.batch_size
    region("root", 32)
    region("commitment_ood_answers", 32 * cfg.commitment_ood_samples * batch)
    region("points", 32 * q * cfg.n_vars)
    region("tags", 32 * l)
    region("evaluations", 32 * q * batch)
    region("sums", 32 * l * batch)
    region("initial_sumcheck", 96 * k)
    for r in range(cfg.n_rounds):
        region(f"round{r}_root", 32)
        region(f"round{r}_ood_answers", 32 * cfg.ood_samples[r])
        nonce(f"round{r}_nonce", cfg.pow_bits[r])
        hint(f"round{r}_stir_answers")
        hint(f"round{r}_merkle_proof")
        region(f"round{r}_sumcheck", 96 * k)
    final_vars = cfg.n_vars - k * (cfg.n_rounds + 1)
    region("final_coeffs", 32 << final_vars)
    nonce("final_nonce", cfg.final_pow_bits)
    hint("final_stir_answers")
    hint("final_merkle_proof")
    region("final_sumcheck", 96 * final_vars)
    nonce("final_folding_nonce", cfg.final_folding_pow_bits)
    hint("deferred")
    assert i == len(proof), f"the layout walk ended at {i}, the proof at {len(proof)}"
    return regions


def offsets(proof, cfg, q, l=0):
    """name -> byte offset of one representative of a region"""
    reg = {name: (a, b) for name, a, b in walk(proof, cfg, q, l)}
    first_tree = "round0_stir_answers" if cfg.n_rounds else "final_stir_answers"
    pos = {name: a for name, (a, b) in reg.items() if b > a}
    for tag, name in (("first_tree_leaf", first_tree), ("last_tree_leaf", "final_stir_answers")):
        a, _ = reg[name]
        (count,) = struct.unpack_from("<Q", proof, a + 4)
        (width,) = struct.unpack_from("<Q", proof, a + 12)
        assert count >= 1 and width >= 2
        pos[tag] = a + 4 + 8 + (count - 1) * (8 + 32 * width) + 8 + 32 * (width - 1)  # the last element of the last opened leaf
    a, b = reg["deferred"]
    pos["deferred_value"] = b - 32
    return pos


def first_difference(got, want, cfg, q, l=0):
    """'' for equal byte strings, else where they first differ and in which region of the reference's layout"""
    if got == want:
        return ""
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    where = next((name for name, a, b in walk(want, cfg, q, l) if a <= at < b), "past the end")
    return f"{len(got)} bytes against the oracle's {len(want)}: first difference at byte {at}, in {where}"
