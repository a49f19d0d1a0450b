"""Shared by test_prove_shapes_host.py and test_gpu_prove_shapes.py: a grid over the scheme shapes pk_scheme_create accepts (every folding
factor 1 .. 8 on the witness side and 1 .. 7 on the blinding side, rates above 1/2, no folding round, final sumchecks of 0, 1, 5 and 6
variables, 0 .. 4 OOD samples, grinding at each position alone at 3 and at 5 bits, the smallest schemes, an empty witness, both
capacities), the oracle prover's proof of every entry (oracle/prover_ref.py, imported, not edited), a walker that names the regions of
a pk_prove proof string, and the bounds of the family with the accepted neighbour of each.

Not in the grid: more than 32 initial weights.  eq_weights' chunk of 32 (mle.hip eq_accumulate) is not reachable from the INITIAL
combination of pk_prove: its points are the commitment's OOD samples alone, at most 4 -- the statement rows join w0 by axpy, not as
points.  (A round's weights pass 32 with enough STIR queries; test_gpu_opening_fused.py owns those counts.)"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEFAULT_QUERIES = [7, 5, 4] + [3] * 13  # a count for each of the 16 rounds a config may have
GRIND_BITS = 3.0  # a solve is a few hundred hashes; at most PK_HOST_POW_MAX_BITS = 4: the host grinder's side of pow_round
DEVICE_GRIND_BITS = 5.0  # above it: the device grinder's
SEED = 7


def nb_vars(m_0):
    """variables of the blinding config: next_power_of_two(4 m_0) + 1 (provekit/r1cs-compiler/src/whir_r1cs.rs:31-34)"""
    nb = 0
    while (1 << nb) < 4 * m_0:
        nb += 1
    return nb + 1


def config(n, fold, rate, rounds=None, ood=1, commitment_ood=1, grind=GRIND_BITS, final_folding_pow=0.0):
    """pk_whir_config_derive's shape for (n, fold, rate) at batch 2 with the round count kept or cut and every count small"""
    from provekit_amd.scheme import WhirConfig

    c = WhirConfig.derive(n, batch_size=2, folding_factor=fold, starting_log_inv_rate=rate)
    r = c.n_rounds if rounds is None else rounds
    c.num_queries = DEFAULT_QUERIES[:r]
    assert len(c.num_queries) == r, "a query count for every round"
    c.ood_samples = [ood] * r
    c.pow_bits = [float(grind)] * r
    c.final_queries = 4
    c.final_pow_bits = float(grind)
    c.commitment_ood_samples = commitment_ood
    c.final_folding_pow_bits = float(final_folding_pow)
    return c


def vcfg(c):
    import verifier as V

    return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, list(c.num_queries), list(c.ood_samples), list(c.pow_bits),
                        c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)


class Entry:
    """one scheme shape: (m, m_0), the statement -- nc constraints over n_in inputs (test_gpu_prove.satisfiable_r1cs: 1 + n_in + nc
    witnesses), or n_in = "empty": no witness at all and three matrices without entries -- and config()'s keyword arguments for the
    witness side (n = m) and the blinding side (n = nb_vars(m_0)).  only = (side, position, bits): nothing grinds but that one position
    ("round0", "final" or "final_folding") of that side ("w" or "b").  patch(sw, sb), for the refused side of a bound alone: applied to
    the two pk_whir_config structs last; scheme = (m, m_0) as pk_scheme_create is told them, where that is the bound"""

    def __init__(self, id, m, m_0, nc, n_in, w, b, only=None, patch=None, scheme=None):
        self.id, self.m, self.m_0, self.nc, self.n_in, self.w, self.b, self.only, self.patch = id, m, m_0, nc, n_in, dict(w), dict(b), only, patch
        self.scheme = scheme or (m, m_0)
        self.empty = n_in == "empty"
        self.nw = 0 if self.empty else 1 + n_in + nc

    def cfgs(self):
        cw, cb = config(self.m, **self.w), config(nb_vars(self.m_0), **self.b)
        if self.only:
            side, position, bits = self.only
            assert self.w.get("grind") == 0.0 and self.b.get("grind") == 0.0
            c = cw if side == "w" else cb
            if position == "round0":
                c.pow_bits[0] = float(bits)
            elif position == "final":
                c.final_pow_bits = float(bits)
            else:
                assert position == "final_folding"
                c.final_folding_pow_bits = float(bits)
        return cw, cb

    def structs(self):
        from provekit_amd.scheme import _cfg_struct

        sw, sb = (_cfg_struct(c) for c in self.cfgs())
        if self.patch:
            self.patch(sw, sb)
        return sw, sb

    def final_vars(self):
        return tuple(c.n_vars - c.folding_factor * (c.n_rounds + 1) for c in self.cfgs())

    def fits(self):
        return self.nw <= 1 << (self.m - 1) and self.nc <= 1 << self.m_0

    def __repr__(self):
        return self.id


F2 = dict(fold=2, rate=1)
F4 = dict(fold=4, rate=1)
NOGRIND = dict(grind=0.0)

# every fold on the witness side; the blinding side (5 variables at m_0 = 3) at the same fold where it has the variables
WITNESS_FOLDS = {k: Entry(f"witness-fold{k}", max(k + 1, 6), 3, 6, 3, dict(fold=k, rate=1), dict(fold=min(k, 4), rate=1)) for k in (1, 2, 3, 5, 6, 7, 8)}
BLINDING_FOLDS = {
    5: Entry("blinding-fold5", 8, 5, 20, 10, F4, dict(fold=5, rate=1)),
    6: Entry("blinding-fold6", 8, 5, 20, 10, F4, dict(fold=6, rate=1)),
    7: Entry("blinding-fold7", 10, 9, 300, 50, F4, dict(fold=7, rate=1)),
}
NO_OOD = Entry("no-ood-no-grinding", 8, 4, 12, 6, dict(F2, ood=0, commitment_ood=0, **NOGRIND), dict(F2, ood=0, commitment_ood=0, **NOGRIND))
M1 = Entry("m1-m0_1-one-witness", 1, 1, 0, 0, dict(fold=1, rate=1), dict(fold=1, rate=1))  # a two-row tree; blinding: 3 variables, 2 rounds
EMPTY = Entry("empty-witness-nc3", 5, 2, 3, "empty", F2, F2)
EMPTY_NC0 = Entry("empty-witness-nc0", 5, 2, 0, "empty", F2, F2)
CAPACITY = Entry("capacity-nw64-nc32", 7, 5, 32, 31, dict(fold=3, rate=1), dict(fold=3, rate=1))  # nw = 2^(m-1), nc = 2^m_0 at once
NC_CAPACITY = Entry("nc-at-capacity", 6, 3, 8, 4, F2, F2)  # nc = 2^m_0 alone
FOLD1_M9 = Entry("fold1-m9-eight-rounds", 9, 3, 6, 3, dict(fold=1, rate=1), F2)  # a constant rate while the domain halves
SINGLE_GRIND = [Entry(f"grind-{side}-{pos}-{int(bits)}bits", 8, 4, 12, 6, dict(F2, **NOGRIND), dict(F2, **NOGRIND), only=(side, pos, bits))
                for side in ("w", "b") for pos in ("round0", "final", "final_folding") for bits in (GRIND_BITS, DEVICE_GRIND_BITS)]
NO_ROUND = Entry("no-round-either-side", 10, 5, 20, 10, dict(F4, rounds=0), dict(F2, rounds=0))  # witness: fold 4, a final sumcheck of six variables
FINAL5 = Entry("fold2-m9-one-round", 9, 3, 6, 3, dict(F2, rounds=1), F2)  # a final sumcheck of five variables
GRID = list(WITNESS_FOLDS.values()) + list(BLINDING_FOLDS.values()) + [
    Entry("rates-quarter-eighth", 8, 4, 12, 6, dict(fold=2, rate=2), dict(fold=2, rate=3)),
    NO_ROUND,
    NO_OOD,
    Entry("ood4-against-2-and-3", 8, 4, 12, 6, dict(F2, ood=4, commitment_ood=4, final_folding_pow=2.0), dict(fold=1, rate=1, ood=2, commitment_ood=3, final_folding_pow=2.0)),
    M1,
    Entry("m2-fold1-nc1", 2, 1, 1, 0, dict(fold=1, rate=1), dict(fold=3, rate=1)),
    Entry("m2-fold2-nc1", 2, 1, 1, 0, F2, dict(fold=3, rate=1)),
    EMPTY,
    EMPTY_NC0,
    CAPACITY,
    FOLD1_M9,
    FINAL5,
] + SINGLE_GRIND + [
    Entry("witness-of-one", 5, 2, 0, 0, F2, F2),  # nw = 1, no constraint
    Entry("witness-odd-length", 6, 3, 6, 20, F2, F2),  # nw = 2^(m-1) - 5 = 27
    Entry("one-constraint", 6, 3, 1, 9, F2, F2),
    NC_CAPACITY,
]
assert len({e.id for e in GRID}) == len(GRID)
assert Entry("", 6, 3, 6, 20, F2, F2).nw == (1 << 5) - 5 and M1.nw == 1

# check B's subset: one entry per fold value, the no-OOD entry, the empty witness, m = 1, both capacity entries
LATENCY = list(WITNESS_FOLDS.values()) + [BLINDING_FOLDS[7], FOLD1_M9, NO_OOD, EMPTY, M1, CAPACITY, NC_CAPACITY]
HASH_V1 = [WITNESS_FOLDS[2], BLINDING_FOLDS[7], EMPTY]
TAMPERED = [WITNESS_FOLDS[1], WITNESS_FOLDS[8], BLINDING_FOLDS[7], NO_OOD, EMPTY, M1, FINAL5]
REUSE = [EMPTY, WITNESS_FOLDS[1], NO_OOD]  # NO_OOD: no point overwrites w0, so what the proof before left there would join the rows


# ---- the bounds of the family ----------------------------------------------------------------------------------------------------------
def _set(side, **fields):
    def patch(sw, sb):
        for k, v in fields.items():
            setattr(sw if side == "w" else sb, k, v)

    return patch


def _base(id, **kw):
    args = dict(m=6, m_0=3, nc=6, n_in=3, w=F2, b=F2)
    args.update(kw)
    return Entry(id, **args)


# (what, the cause as pk_scheme_create's error names it, the refused shape, its accepted neighbour or None, is the neighbour small enough
# to prove and compare, is the bound one of the WHIR config alone -- which the host-only entry points that take a config state too)
BOUNDS = [
    ("witness fold 9 | 8", "folding factor", _base("w-fold9", m=9, w=dict(fold=8, rate=1), patch=_set("w", folding_factor=9)), WITNESS_FOLDS[8], True, True),
    ("witness fold 0", "folding factor", _base("w-fold0", patch=_set("w", folding_factor=0)), None, False, True),
    ("blinding fold 9 | 7", "folding factor", _base("b-fold9", patch=_set("b", folding_factor=9)), BLINDING_FOLDS[7], True, True),
    ("fold * (rounds + 1) = n + 1 | n", "rounds exceed", _base("w-rounds-past-n", m=7, nc=6, n_in=3, w=dict(F2, rounds=3)), _base("w-rounds-at-n", m=8, w=dict(F2, rounds=3)), True, True),
    ("5 | 4 OOD samples per commitment", "OOD samples", _base("w-cood5", w=dict(F2, commitment_ood=5)), _base("w-cood4", w=dict(F2, commitment_ood=4)), True, True),
    ("5 | 4 OOD samples per round", "OOD samples", _base("b-ood5", b=dict(F2, ood=5)), _base("b-ood4", b=dict(F2, ood=4)), True, True),
    ("17 | 16 rounds", "too many WHIR rounds", _base("w-17-rounds", m=17, w=dict(fold=1, rate=1), patch=_set("w", n_rounds=17)), _base("w-16-rounds", m=17, w=dict(fold=1, rate=1)), False, True),
    ("witness batch 1 | 2", "batch", _base("w-batch1", patch=_set("w", batch_size=1)), _base("batch2"), True, False),
    ("witness batch 3 | 2", "batch", _base("w-batch3", patch=_set("w", batch_size=3)), None, False, False),
    ("blinding batch 3 | 2", "batch", _base("b-batch3", patch=_set("b", batch_size=3)), None, False, False),
    ("blinding batch 1 | 2", "batch", _base("b-batch1", patch=_set("b", batch_size=1)), None, False, False),
    ("witness n_vars = m + 1 | m", "does not match m", _base("w-nvars-off", patch=_set("w", n_vars=7)), None, False, False),
    ("blinding n_vars one more | exact", r"next_power_of_two\(4\*m_0\)\+1 variables", _base("b-nvars-more", patch=_set("b", n_vars=6)), None, False, False),
    ("blinding n_vars one fewer | exact", r"next_power_of_two\(4\*m_0\)\+1 variables", _base("b-nvars-fewer", patch=_set("b", n_vars=4)), None, False, False),
    ("m = 0 | 1", "scheme size out of range", Entry("m0", 1, 1, 0, 0, dict(fold=1, rate=1), dict(fold=1, rate=1), scheme=(0, 1)), M1, True, False),
    ("m = 28", "scheme size out of range", _base("m28", scheme=(28, 3)), None, False, False),
    ("m_0 = 0 | 1", "scheme size out of range", Entry("m_0-0", 1, 1, 0, 0, dict(fold=1, rate=1), dict(fold=1, rate=1), scheme=(1, 0)), M1, True, False),
    ("m_0 = 28", "scheme size out of range", _base("m_0-28", scheme=(6, 28)), None, False, False),
    ("witness length 2^(m-1) + 1 | 2^(m-1)", "witness length exceeds", _base("nw9", m=4, nc=4, n_in=4), _base("nw8", m=4, nc=4, n_in=3), True, False),
    ("constraints 2^m_0 + 1 | 2^m_0", "constraints exceed", _base("nc5", m=5, m_0=2, nc=5, n_in=2), _base("nc4", m=5, m_0=2, nc=4, n_in=2), True, False),
]
assert len({b[0] for b in BOUNDS}) == len(BOUNDS)


# ---- statements and the oracle's proofs ---------------------------------------------------------------------------------------------------
class Instance:
    """an entry's statement: the triplets of test_gpu_prove.satisfiable_r1cs, the CSR arrays the oracle takes and the witness"""

    def __init__(self, oracle, entry, seed=5):
        from test_gpu_prove import satisfiable_r1cs

        self.nc = entry.nc
        if entry.empty:
            self.nw, z, self.coeffs, self.trips = 0, [], [1, 2], (([], [], []),) * 3
        else:
            self.nw, z, self.coeffs, self.trips = satisfiable_r1cs(entry.nc, entry.n_in, seed)
        assert self.nw == entry.nw
        self.z = z
        self.csr = []
        for rows, cols, vals in self.trips:
            rows = np.array(rows, dtype=np.int64)
            self.csr.append((np.searchsorted(rows, np.arange(self.nc)).astype(np.uint32), np.array(cols, dtype=np.uint32), np.array(vals, dtype=np.uint32)))
        self.interner = oracle.to_mont(oracle.ints_to_limbs(self.coeffs))
        self.zm = oracle.to_mont(oracle.ints_to_limbs(z)) if self.nw else np.zeros((0, 4), dtype=np.uint64)
        self.canonical = [(t[0], t[1], [self.coeffs[v] for v in t[2]]) for t in self.trips]  # what verifier.verify's matrix check takes

    def other_witness(self, oracle, seed):
        """another satisfying witness of the same matrices' shape is another statement; for the reuse check any vector of the length
        will do: the prover does not test satisfaction"""
        rng = np.random.default_rng(seed)
        return oracle.to_mont(oracle.ints_to_limbs([int(x) for x in rng.integers(1, 2**62, size=self.nw)])) if self.nw else self.zm


def prove_with_hash_version(oracle, hash_version, fn):
    """fn() with prover_ref.commit's hash version as a parameter (its own is fixed at 2), as whir_pcs_cases.oracle_opening wraps it"""
    import prover_ref as PR

    if hash_version == 2:
        return fn()

    def commit(c, ps, tm_):
        leaves = oracle.rs_encode(ps[0] if len(ps) == 1 else np.concatenate(ps), len(ps), c.n_vars, c.starting_log_inv_rate, c.folding_factor)
        return leaves, oracle.merkle_commit(leaves, hash_version), leaves.shape[0], leaves.shape[1]

    saved = PR.commit
    PR.commit = commit
    try:
        return fn()
    finally:
        PR.commit = saved


_cache = {}


def instance(oracle, entry):
    if entry.id not in _cache:
        _cache[entry.id] = Instance(oracle, entry)
    return _cache[entry.id]


def oracle_proof(oracle, entry, seed=SEED, hash_version=2, witness=None):
    """-> (proof bytes, domain separator, (verifier config of the witness side, of the blinding side), Instance): the oracle prover's
    proof of the entry's statement under the key `seed`, built once per (entry, seed, hash version).  witness: other Montgomery values
    of the statement's length (not cached)"""
    import prover_ref as PR
    from provekit_amd.scheme import create_io_pattern

    key = (entry.id, seed, hash_version)
    if witness is None and key in _cache:
        return _cache[key]
    inst = instance(oracle, entry)
    cw, cb = entry.cfgs()
    ds = create_io_pattern(entry.m_0, cw, cb)
    vw, vb = vcfg(cw), vcfg(cb)
    zm = inst.zm if witness is None else witness
    proof = prove_with_hash_version(oracle, hash_version, lambda: PR.prove(ds, entry.m, entry.m_0, vw, vb, (inst.nc, inst.nw, inst.csr, inst.interner), zm,
                                                                          seed.to_bytes(32, "little")))
    out = (proof, ds, (vw, vb), inst)
    if witness is None:
        _cache[key] = out
    return out


# ---- the layout of a pk_prove proof string ---------------------------------------------------------------------------------------------
def walk(proof, m_0, cw, cb):
    """[(name, start, end)] of every region of a proof, in order, found by walking the two configs (a scalar is 32 bytes, a nonce 8, a
    hint a u32 length and its payload); regions of no bytes are listed too.  Ends at the proof's end or asserts"""
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

    def whir(side, c):
        k = c.folding_factor
        region(f"{side}/initial_sumcheck", 96 * k)
        for r in range(c.n_rounds):
            region(f"{side}/round{r}_root", 32)
            region(f"{side}/round{r}_ood_answers", 32 * c.ood_samples[r])
            region(f"{side}/round{r}_nonce", 8 if c.pow_bits[r] > 0 else 0)
            hint(f"{side}/round{r}_stir_answers")
            hint(f"{side}/round{r}_merkle_proof")
            region(f"{side}/round{r}_sumcheck", 96 * k)
        final_vars = c.n_vars - k * (c.n_rounds + 1)
        region(f"{side}/final_coeffs", 32 << final_vars)
        region(f"{side}/final_nonce", 8 if c.final_pow_bits > 0 else 0)
        hint(f"{side}/final_stir_answers")
        hint(f"{side}/final_merkle_proof")
        region(f"{side}/final_sumcheck", 96 * final_vars)
        region(f"{side}/final_folding_nonce", 8 if c.final_folding_pow_bits > 0 else 0)
        hint(f"{side}/deferred")

    region("witness/root", 32)
    region("witness/commitment_ood_answers", 32 * cw.commitment_ood_samples * 2)
    region("blinding/root", 32)
    region("blinding/commitment_ood_answers", 32 * cb.commitment_ood_samples * 2)
    region("sum_g", 32)
    region("zk_sumcheck", 128 * m_0)
    region("polynomial_sums", 64)
    whir("blinding", cb)
    hint("claimed_evaluations")
    whir("witness", cw)
    assert i == len(proof), f"the layout walk ended at {i}, the proof at {len(proof)}"
    return regions


def offsets(proof, m_0, cw, cb):
    """name -> byte offset of one representative of each region the tampering tests name"""
    reg = {name: (a, b) for name, a, b in walk(proof, m_0, cw, cb)}
    pos = {"first_commitment": reg["witness/root"][0]}
    for side in ("blinding", "witness"):
        a, _ = reg[f"{side}/final_stir_answers"]
        (count,) = struct.unpack_from("<Q", proof, a + 4)
        (width,) = struct.unpack_from("<Q", proof, a + 12)
        assert count >= 1 and width >= 2
        pos[f"{side}/opening_hint"] = a + 4 + 8 + (count - 1) * (8 + 32 * width) + 8 + 32 * (width - 1)  # the last element of the last opened leaf
        pos[f"{side}/final_coeffs"] = reg[f"{side}/final_coeffs"][0]
        pos[f"{side}/deferred_hint"] = reg[f"{side}/deferred"][1] - 32
    return pos


def first_difference(got, want, m_0, cw, cb):
    """'' for equal byte strings, else where they first differ and in which region of the reference's layout"""
    if got == want:
        return ""
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    where = next((name for name, a, b in walk(want, m_0, cw, cb) if a <= at < b), "past the end")
    return f"{len(got)} bytes against the oracle's {len(want)}: first difference at byte {at}, in {where}"
