"""Shared by test_witness_edge_cases_host.py and test_gpu_witness_edges.py: hand-built WitnessBuilder lists that land on the places
where csrc/witness.hip changes path -- the NARROW phase width, the wave-aggregated histogram, the Spice sort's workgroup seams, the
digit slices' word boundaries, the error record, program reuse.  Every function returns a Case: the list, its inputs, and what the
levelled program must look like for the case to hit its edge (`expect`, checked on the host with no device).

The thresholds are the values the library had when the cases were written; both test files assert that tools.pk_probes still
reports them before anything straddles them."""
import os
import random
import sys
from dataclasses import dataclass, field

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import witness_ref as R  # noqa: E402

from provekit_amd.witness import WitnessBuilder as WB  # noqa: E402

P = R.P
NARROW, SUM_HEAVY, SUM_CHUNK = 1024, 128, 1024  # csrc/witness_shape.hpp at the time of writing
WAVE = 64
# csrc/witness.hip's OP_* order: the columns of tools.pk_probes.witness_phases(...)["ops"]
OPS = ("CONST", "ACIR", "SUM", "PRODUCT", "CHALLENGE", "IDX_LOGUP", "INVERSE", "PROD_LINEAR", "LOGUP", "SPICE_FACTOR", "BINOP_DENOM", "DIGIT",
       "DIGIT_CHECK", "HIST_RANGE", "HIST_BINOP", "COUNT_OUT")
OP = {name: i for i, name in enumerate(OPS)}


@dataclass
class Case:
    builders: list
    acir: list
    nw: int
    expect: dict = field(default_factory=dict)  # n_levels, n_items, widths, n_none, blocks_before, ... (what the host test asserts)
    # error cases: the oracle panics at builders[panic_builder] and the library's message holds panic_msg; acir_good does not fail
    panic_builder: int = None
    panic_msg: str = None
    acir_good: list = None


class _List:
    """a builder list under construction: fresh witness indices, ACIR inputs appended with their values"""

    def __init__(self, seed=0):
        self.b, self.acir, self.nxt, self.rnd = [], [], 0, random.Random(seed)

    def fresh(self, n=1):
        i = self.nxt
        self.nxt += n
        return i

    def add(self, builder):
        self.b.append(builder)
        return len(self.b) - 1

    def acir_in(self, value, at=None):
        """a witness holding ACIR input `value` -> its witness index"""
        i = self.fresh() if at is None else at
        self.b.append(WB.Acir(i, len(self.acir)))
        self.acir.append(value % P)
        return i

    def fe(self):
        return self.rnd.randrange(P)

    def solved(self):
        """the sequential solver's witnesses for the list so far"""
        return R.solve_witness_vec(self.b, self.acir, [], self.nxt)

    def case(self, spare=1, **expect):
        nw = self.nxt + spare  # `spare` trailing witnesses nobody writes
        want = R.solve_witness_vec(self.b, self.acir, [], nw)
        expect.setdefault("n_none", sum(x is None for x in want))
        return Case(self.b, self.acir, nw, expect)


# ---- 1. phase widths ---------------------------------------------------------------------------------------------------------------
def phase_width(n):
    """4 inputs; a level of n independent products; a level of n consumers, one per producer"""
    L = _List(100 + n)
    ins = [L.acir_in(L.fe()) for _ in range(4)]
    prod = [L.fresh() for _ in range(n)]
    for i, w in enumerate(prod):
        L.add(WB.Product(w, ins[i % 4], ins[(i // 4) % 4]))
    for i, w in enumerate(prod):
        L.add(WB.Product(L.fresh(), w, ins[(i // 16) % 4]))
    return L.case(n_levels=3, n_items=4 + 2 * n, widths=[4, 0, n, 0, n, 0], n_none=1)


def _three_narrow_levels(L):
    ins = [L.acir_in(L.fe()) for _ in range(8)]
    lv1 = [L.fresh() for _ in range(10)]
    for i, w in enumerate(lv1):
        L.add(WB.Product(w, ins[i % 8], ins[(3 * i + 1) % 8]))
    lv2 = [L.fresh() for _ in range(10)]
    for i, w in enumerate(lv2):
        L.add(WB.Product(w, lv1[i], ins[i % 8]))
    return ins, lv1, lv2


def run_cut_by_long_sum():
    """three narrow levels; the middle one also holds a Sum of SUM_HEAVY + 1 terms and a range table of 4, so the narrow run that
    starts at phase 0 must stop before phase 5 (the long sum runs there) and a new run starts on that odd phase"""
    L = _List(11)
    ins, lv1, lv2 = _three_narrow_levels(L)
    small = [L.acir_in(v) for v in (0, 3, 3, 1)]
    s = L.fresh()
    L.add(WB.Sum(s, [(None if t % 3 == 0 else L.fe(), (ins + lv1)[t % 18]) for t in range(SUM_HEAVY + 1)]))
    # the range table must sit on level 2 as well: it looks up one level-1 product (0 times an input) and three inputs
    z = L.fresh()
    L.add(WB.Product(z, small[0], ins[0]))  # level 1, value 0
    table = L.fresh(4)
    L.add(WB.MultiplicitiesForRange(table, 4, [z] + small[1:]))
    for w in lv2 + [s, table + 3]:
        L.add(WB.Product(L.fresh(), w, ins[1]))
    # level 0: 8 + 4 inputs; 1: 10 + 1 products; 2: 10 products + 4 lookups (the sum is no item), then 4 counts; 3: 12 consumers
    return L.case(n_levels=4, n_items=12 + 11 + 14 + 4 + 12, widths=[12, 0, 11, 0, 14, 4, 12, 0], blocks_before=[0, 0, 0, 0, 0, 1, 0, 0], n_none=1)


def run_cut_by_spice():
    """the same with a Spice block in place of the long sum"""
    L = _List(12)
    ins, lv1, lv2 = _three_narrow_levels(L)
    small = [L.acir_in(v) for v in (0, 3, 3, 1)]
    z = L.fresh()
    L.add(WB.Product(z, small[0], ins[0]))  # level 1, value 0
    init = L.fresh(4)  # never written: the memory starts as None
    outs = [L.fresh() for _ in range(5)]
    rv, rt = L.fresh(4), L.fresh(4)
    # addresses: a level-1 product (0) and inputs, so the block is on level 2
    L.add(WB.SpiceWitnesses(4, init, [("store", z, outs[0], lv1[0], outs[1]), ("load", small[1], lv1[1], outs[2]), ("store", small[2], outs[3], ins[0], outs[4])], rv, rt))
    table = L.fresh(4)
    L.add(WB.MultiplicitiesForRange(table, 4, [z] + small[1:]))
    for w in lv2 + [outs[1], outs[3], rv + 3, rt + 1, table]:
        L.add(WB.Product(L.fresh(), w, ins[1]))
    # None: init (4), the old value of the first store (cell 0 was None), rv[1], rv[2] (never touched), the spare
    return L.case(n_levels=4, n_items=12 + 11 + 14 + 4 + 15, widths=[12, 0, 11, 0, 14, 4, 15, 0], blocks_before=[0, 0, 0, 0, 0, 1, 0, 0], n_none=4 + 1 + 2 + 1)


def _bytes(L, n=32):
    return [L.acir_in(L.rnd.randrange(256)) for _ in range(n)]


def wide_histogram_narrow_counts():
    """a range table of 256 with NARROW + 1 lookups: a wide histogram phase (its own launch), then the 256 counts as a narrow phase that
    starts a run on an odd phase; a product one level up reads two counts"""
    L = _List(13)
    by = _bytes(L)
    table = L.fresh(256)
    L.add(WB.MultiplicitiesForRange(table, 256, [by[L.rnd.randrange(32)] for _ in range(NARROW + 1)]))
    v = L.solved()
    L.add(WB.Product(L.fresh(), table + v[by[0]], table + v[by[1]]))
    return L.case(n_levels=3, n_items=32 + NARROW + 1 + 256 + 1, widths=[32, 0, NARROW + 1, 256, 1, 0], n_none=1)


def narrow_histogram_wide_counts():
    """a bin-op table with 10 lookups: a narrow histogram phase, then 65536 counts as a wide phase"""
    L = _List(14)
    by = _bytes(L)
    table = L.fresh(65536)
    pairs = [(("w", by[L.rnd.randrange(32)]), ("w", by[L.rnd.randrange(32)])) for _ in range(10)]
    L.add(WB.MultiplicitiesForBinOp(table, pairs))
    v = L.solved()
    hit = table + 256 * v[pairs[0][0][1]] + v[pairs[0][1][1]]
    L.add(WB.Product(L.fresh(), hit, table + 65535))
    return L.case(n_levels=3, n_items=32 + 10 + 65536 + 1, widths=[32, 0, 10, 65536, 1, 0], n_none=1)


def both_multiplicities_in_one_level():
    """a range table (300 lookups) and a bin-op table (10 lookups) on one level: one narrow histogram phase holding both variants,
    one wide count-out phase holding both tables"""
    L = _List(15)
    by = _bytes(L)
    rt, bt = L.fresh(256), L.fresh(65536)
    L.add(WB.MultiplicitiesForRange(rt, 256, [by[L.rnd.randrange(32)] for _ in range(300)]))
    pairs = [(("w", by[L.rnd.randrange(32)]), ("w", by[L.rnd.randrange(32)])) for _ in range(10)]
    L.add(WB.MultiplicitiesForBinOp(bt, pairs))
    v = L.solved()
    L.add(WB.Product(L.fresh(), rt + v[by[3]], bt + 256 * v[pairs[4][0][1]] + v[pairs[4][1][1]]))
    return L.case(n_levels=3, n_items=32 + 310 + 256 + 65536 + 1, widths=[32, 0, 310, 256 + 65536, 1, 0], n_none=1)


PHASE_CASES = {
    "products_1023": lambda: phase_width(NARROW - 1), "products_1024": lambda: phase_width(NARROW), "products_1025": lambda: phase_width(NARROW + 1),
    "run_cut_by_long_sum": run_cut_by_long_sum, "run_cut_by_spice": run_cut_by_spice, "wide_histogram_narrow_counts": wide_histogram_narrow_counts,
    "narrow_histogram_wide_counts": narrow_histogram_wide_counts, "both_multiplicities_in_one_level": both_multiplicities_in_one_level,
}


# ---- 2. histograms -----------------------------------------------------------------------------------------------------------------
def range_lookups(kind):
    """a range table of 256 over 256 witnesses that each hold their own byte (witness i = i), looked up as `kind` says; expect["bins"]
    = the counts that must come out, bin by bin"""
    L = _List(20)
    own = [L.acir_in(i) for i in range(256)]
    if kind == "one_wavefront_one_value":
        look = [own[7]] * WAVE
    elif kind == "4096_of_one_value":
        look = [own[201]] * 4096
    elif kind == "two_values_alternating":
        look = [own[5], own[250]] * WAVE
    elif kind == "tail_of_two_lanes":
        look = [own[(7 * i) % 256] for i in range(2 * WAVE + 2)]
    elif kind == "256_distinct_witnesses":
        look = list(own)
        L.rnd.shuffle(look)
    elif kind == "high_limbs_set":  # into_bigint().0[0]: only the low 64 bits index the table
        look = [L.acir_in((1 << 64) + 7), L.acir_in((1 << 200) + 7), own[7], own[8]]
    else:
        raise KeyError(kind)
    table = L.fresh(256)
    L.add(WB.MultiplicitiesForRange(table, 256, look))
    L.add(WB.Product(L.fresh(), table + 7, table + 8))
    bins = [0] * 256
    v = L.solved()
    for w in look:
        bins[v[w] & 0xff] += 1
    n_in = len(L.acir)
    return L.case(n_levels=3, n_items=n_in + len(look) + 256 + 1, widths=[n_in, 0, len(look), 256, 1, 0], n_none=1, bins=bins, table=table)


def three_tables_in_one_level():
    """two range tables (256 with 100 lookups, 16 with 50) and a bin-op table (70 lookups, constants among the operands) on one level:
    in the sorted item list the first table's lookups end at lane 36 of the second wavefront, the range lookups at lane 22 of the
    third, where the bin-op lookups begin"""
    L = _List(21)
    by = _bytes(L)
    nib = [L.acir_in(L.rnd.randrange(16)) for _ in range(8)]
    ta, tb, tc = L.fresh(256), L.fresh(16), L.fresh(65536)
    L.add(WB.MultiplicitiesForRange(ta, 256, [by[L.rnd.randrange(32)] for _ in range(100)]))
    L.add(WB.MultiplicitiesForRange(tb, 16, [nib[L.rnd.randrange(8)] for _ in range(50)]))

    def operand():
        return ("c", L.rnd.randrange(256)) if L.rnd.random() < 0.3 else ("w", by[L.rnd.randrange(32)])

    pairs = [(operand(), operand()) for _ in range(70)]
    pairs[0], pairs[1] = (("c", 255), ("c", 255)), (("c", 0), ("w", by[0]))
    L.add(WB.MultiplicitiesForBinOp(tc, pairs))
    L.add(WB.Product(L.fresh(), ta + L.acir[0], tc + 65535))
    L.add(WB.Product(L.fresh(), tb + L.acir[32], tc + L.acir[0]))
    return L.case(n_levels=3, n_items=40 + 220 + 256 + 16 + 65536 + 2, widths=[40, 0, 220, 256 + 16 + 65536, 2, 0], n_none=1, hist_range=150, hist_binop=70)


def binop_lhs_above_2_56():
    """witness_builder.rs:184: (lhs.0[0] << 8) + rhs.0[0] on u64 drops lhs's high bits: lhs = 2^56 + 3, rhs = 5 counts in bin 3 * 256 + 5"""
    L = _List(22)
    lhs, rhs, a, b = L.acir_in((1 << 56) + 3), L.acir_in(5), L.acir_in(3), L.acir_in(5)
    table = L.fresh(65536)
    L.add(WB.MultiplicitiesForBinOp(table, [(("w", lhs), ("w", rhs)), (("w", a), ("w", b)), (("c", (1 << 56) + 3), ("c", 5)), (("w", a), ("c", 6))]))
    L.add(WB.Product(L.fresh(), table + 3 * 256 + 5, table + 3 * 256 + 6))
    return L.case(n_levels=3, n_items=4 + 4 + 65536 + 1, widths=[4, 0, 4, 65536, 1, 0], n_none=1, bin=table + 3 * 256 + 5, count=3)


RANGE_KINDS = ("one_wavefront_one_value", "4096_of_one_value", "two_values_alternating", "tail_of_two_lanes", "256_distinct_witnesses", "high_limbs_set")
HISTOGRAM_CASES = {**{k: (lambda k=k: range_lookups(k)) for k in RANGE_KINDS}, "three_tables_in_one_level": three_tables_in_one_level,
                   "binop_lhs_above_2_56": binop_lhs_above_2_56}


# ---- 3. Spice -----------------------------------------------------------------------------------------------------------------------
def _spice_block(L, M, n_ops, addr_of, none_cells=(), pool=None):
    """one block appended to L: addresses from ACIR bytes (addr_of(k) -> the address of operation k), values from a pool that holds
    two never-written witnesses, the initial memory from ACIR inputs except `none_cells`.  -> (outputs, the builder's index)"""
    addrs = {}
    for k in range(n_ops):
        a = addr_of(k)
        if a not in addrs:
            addrs[a] = L.acir_in(a)
    if pool is None:
        pool = [L.acir_in(L.fe()) for _ in range(6)] + [L.fresh(), L.fresh()]  # the last two: never written
    init = L.fresh(M)
    for c in range(M):
        if c not in none_cells:
            L.acir_in(L.fe(), at=init + c)
    ops, outs = [], []
    for k in range(n_ops):
        a, value = addrs[addr_of(k)], pool[L.rnd.randrange(len(pool))]
        if L.rnd.random() < 0.5:
            ts = L.fresh()
            ops.append(("load", a, value, ts))
            outs.append(ts)
        else:
            old, ts = L.fresh(), L.fresh()
            ops.append(("store", a, old, value, ts))
            outs += [old, ts]
    rv, rt = L.fresh(M), L.fresh(M)
    at = L.add(WB.SpiceWitnesses(M, init, ops, rv, rt))
    return outs + list(range(rv, rv + M)) + list(range(rt, rt + M)), at, pool, ops


def _sum_of_set(L, outs):
    """a Sum one level up over every output the sequential solver leaves set (it would unwrap a None)"""
    v = L.solved()
    terms = [(None if i % 2 else L.fe(), w) for i, w in enumerate(outs) if v[w] is not None]
    s = L.fresh()
    L.add(WB.Sum(s, terms))
    return len(terms)


def spice_ops(n_ops, M=8):
    """n_ops operations over M cells at random addresses, cell M - 1 initially None"""
    L = _List(300 + n_ops + M)
    outs, at, _, ops = _spice_block(L, M, n_ops, _addr_stream(M, n_ops), none_cells=(M - 1,))
    terms = _sum_of_set(L, outs)
    n_items = len(L.b) - 1 - (1 if terms > SUM_HEAVY else 0)
    # inputs; the block (with no operation it still copies the initial values the inputs wrote); the sum over its outputs
    return L.case(n_levels=3, n_items=n_items, blocks=1, n_ops=n_ops, M=M, ops=ops)


def _addr_stream(M, n_ops, seed=5):
    r = random.Random(seed * 1000 + n_ops)
    seq = [r.randrange(M) for _ in range(n_ops)]
    return lambda k: seq[k]


def spice_one_cell():
    """memory_length = 1: every operation on address 0"""
    L = _List(31)
    outs, _, _, ops = _spice_block(L, 1, 40, lambda k: 0)
    _sum_of_set(L, outs)
    return L.case(n_levels=3, blocks=1, n_ops=40, M=1, ops=ops)


def spice_one_address_of_many():
    """8 cells, every one of 70 operations on address 3: one run of equal keys across the whole sorted list"""
    L = _List(32)
    outs, _, _, ops = _spice_block(L, 8, 70, lambda k: 3, none_cells=(0,))
    _sum_of_set(L, outs)
    return L.case(n_levels=3, blocks=1, n_ops=70, M=8, ops=ops)


def spice_two_blocks_one_level(first, second):
    """two blocks on one level share the sort buffers (sized for the longer one)"""
    L = _List(33 + first)
    o1, _, _, _ = _spice_block(L, 8, first, _addr_stream(8, first, 6), none_cells=(2,))
    o2, _, _, _ = _spice_block(L, 5, second, _addr_stream(5, second, 7))
    _sum_of_set(L, o1 + o2)
    # both blocks run before phase 3; the sum over their outputs has more than SUM_HEAVY terms and runs before phase 5
    return L.case(n_levels=3, blocks=2, blocks_before=[0, 0, 0, 2, 0, 1])


def spice_blocks_in_two_levels():
    """the second block stores values the first one wrote (read timestamps, final values): it sits one level up"""
    L = _List(35)
    o1, _, pool, _ = _spice_block(L, 8, 30, _addr_stream(8, 30, 8))
    v = L.solved()
    pool2 = [w for w in o1 if v[w] is not None][:12] + pool[-2:]
    o2, _, _, _ = _spice_block(L, 4, 20, _addr_stream(4, 20, 9), pool=pool2)
    _sum_of_set(L, o1 + o2)
    return L.case(n_levels=4, blocks=2, blocks_before=[0, 0, 0, 1, 0, 1, 0, 0])


def spice_none_handling():
    """cell 2 starts as None and is never touched (its final value stays None, its final timestamp is 0); cell 1: a load of a
    never-written witness leaves None there, the store after it gets that None as its old value"""
    L = _List(36)
    a0, a1 = L.acir_in(0), L.acir_in(1)
    val = L.acir_in(L.fe())
    never = L.fresh()
    init = L.fresh(3)
    L.acir_in(L.fe(), at=init)
    L.acir_in(L.fe(), at=init + 1)
    ts0, old, ts1, ts2 = L.fresh(), L.fresh(), L.fresh(), L.fresh()
    rv, rt = L.fresh(3), L.fresh(3)
    L.add(WB.SpiceWitnesses(3, init, [("load", a1, never, ts0), ("store", a1, old, val, ts1), ("load", a0, val, ts2)], rv, rt))
    _sum_of_set(L, [ts0, old, ts1, ts2, rv, rv + 1, rv + 2, rt, rt + 1, rt + 2])
    # None: `never`, init + 2, the store's old value, rv + 2, the spare
    return L.case(n_levels=3, blocks=1, n_none=5, none_at=[never, init + 2, old, rv + 2])


def spice_address_above_2_64():
    """addr.into_bigint().0[0]: an address witness of 2^64 + 3 is address 3"""
    L = _List(37)
    big, three = L.acir_in((1 << 64) + 3), L.acir_in(3)
    val, val2 = L.acir_in(L.fe()), L.acir_in(L.fe())
    init = L.fresh(4)
    for c in range(4):
        L.acir_in(L.fe(), at=init + c)
    old, ts0, ts1 = L.fresh(), L.fresh(), L.fresh()
    rv, rt = L.fresh(4), L.fresh(4)
    L.add(WB.SpiceWitnesses(4, init, [("store", big, old, val, ts0), ("load", three, val2, ts1)], rv, rt))
    _sum_of_set(L, [old, ts0, ts1] + list(range(rv, rv + 8)))
    return L.case(n_levels=3, blocks=1, n_none=1, ts_of_second=ts1)


SPICE_OP_COUNTS = (0, 1, 255, 256, 257)
SPICE_CASES = {**{f"ops_{n}": (lambda n=n: spice_ops(n)) for n in SPICE_OP_COUNTS}, "one_cell": spice_one_cell, "one_address_of_many": spice_one_address_of_many,
               "two_blocks_300_then_7": lambda: spice_two_blocks_one_level(300, 7), "two_blocks_7_then_300": lambda: spice_two_blocks_one_level(7, 300),
               "blocks_in_two_levels": spice_blocks_in_two_levels, "none_handling": spice_none_handling, "address_above_2_64": spice_address_above_2_64}


# ---- 4. digits ----------------------------------------------------------------------------------------------------------------------
DIGIT_BASES = {
    "slices_32_64_33": [32, 64, 33],                  # slices of exactly 32, 64 and 33 bits
    "starts_31_32_63_ends_254": [31, 1, 31, 1, 190],  # slices that start at bits 31, 32, 63 (and 64); the last ends at bit 254
    "zero_width_in_the_middle": [8, 0, 8],
    "256_one_bit_digits": [1] * 256,
}


def digit_values(log_bases, seed=4):
    """0 and 1, 2^k - 1 and 2^k on every slice boundary k, p - 1, five random values: those that fit the bases (a value with a bit
    at or above their total is the overflow case of the error test) and the field"""
    total = sum(log_bases)
    bound = min(P, 1 << total)
    vals = [0, 1]
    k = 0
    for lb in log_bases:
        k += lb
        vals += [(1 << k) - 1, 1 << k]
    vals.append(P - 1)
    rnd = random.Random(seed)
    vals += [rnd.randrange(bound) for _ in range(5)]
    out = []
    for v in vals:
        if v < bound and v not in out:
            out.append(v)
    return out


def digits(name):
    L = _List(40)
    bases = DIGIT_BASES[name]
    vals = digit_values(bases)
    ws = [L.acir_in(v) for v in vals]
    first = L.fresh(len(bases) * len(ws))
    L.add(WB.DigitalDecomposition(bases, ws, first))
    L.add(WB.Product(L.fresh(), first, first + len(bases) * len(ws) - 1))
    n = len(ws)
    return L.case(n_levels=3, n_items=n + (len(bases) + 1) * n + 1, widths=[n, 0, (len(bases) + 1) * n, 0, 1, 0], n_none=1, values=vals)


DIGIT_CASES = {k: (lambda k=k: digits(k)) for k in DIGIT_BASES}


# ---- 5. builders that read what they write ------------------------------------------------------------------------------------------
def _self_spice(which):
    L = _List(50)
    a = [L.acir_in(x) for x in (0, 1, 0, 1)]
    vals = [L.acir_in(L.fe()) for _ in range(3)]
    M = 2
    init = L.fresh(M + 1)
    for c in range(M + 1):
        L.acir_in(L.fe(), at=init + c)
    old1, ts = L.fresh(), [L.fresh() for _ in range(4)]
    rv, rt = L.fresh(M), L.fresh(M)
    if which == "value_is_an_earlier_old_value":  # operation 3 stores what operation 1 got as its old value
        ops = [("load", a[0], vals[0], ts[0]), ("store", a[1], old1, vals[1], ts[1]), ("load", a[2], vals[2], ts[2]), ("load", a[3], old1, ts[3])]
        bad = old1
    elif which == "addr_is_an_earlier_timestamp":  # operation 2's address is operation 0's read timestamp (0)
        ops = [("load", a[0], vals[0], ts[0]), ("store", a[1], old1, vals[1], ts[1]), ("load", ts[0], vals[2], ts[2])]
        bad = ts[0]
    else:  # the final values land on the initial values, shifted by one
        ops = [("load", a[0], vals[0], ts[0]), ("store", a[1], old1, vals[1], ts[1])]
        rv, bad = init + 1, init + 1
    at = L.add(WB.SpiceWitnesses(M, init, ops, rv, rt))
    c = L.case()
    c.expect.update(builder=at, witness=bad)
    return c


def self_digits():
    """a decomposition of two values whose digit range contains the second value: the sequential solver overwrites it with a digit
    of the first value before it decomposes it"""
    L = _List(51)
    v0 = L.acir_in(0x030201)
    first = L.fresh(6)  # digits [8, 8, 8] x 2 values: place-major, so first + 2 is digit 1 of value 0
    L.acir_in(0x060504, at=first + 2)
    at = L.add(WB.DigitalDecomposition([8, 8, 8], [v0, first + 2], first))
    c = L.case()
    c.expect.update(builder=at, witness=first + 2)
    return c


SELF_DEPENDENT_CASES = {"spice_value_is_an_earlier_old_value": lambda: _self_spice("value_is_an_earlier_old_value"),
                        "spice_addr_is_an_earlier_timestamp": lambda: _self_spice("addr_is_an_earlier_timestamp"),
                        "spice_finals_overlap_the_initial_values": lambda: _self_spice("finals_overlap"), "digits_written_over_a_value": self_digits}


def range_table_reads_its_own_output_range():
    """a multiplicity table reads in one phase and writes in the next, like the reference: lookups inside its own output range are
    legal and see the values from before the table is written"""
    L = _List(52)
    table = L.fresh(4)
    for c, v in enumerate((2, 2, 0, 3)):
        L.acir_in(v, at=table + c)
    other = L.acir_in(1)
    L.add(WB.MultiplicitiesForRange(table, 4, [table, table + 1, other, table + 3, table + 2]))
    L.add(WB.Product(L.fresh(), table + 2, table + 3))
    return L.case(n_levels=3, n_items=5 + 5 + 4 + 1, widths=[5, 0, 5, 4, 1, 0], n_none=1, table=table, counts=[1, 1, 2, 1])


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def error_two_inverses():
    """builder 40 inverts the end of a 30-deep product chain that starts from a zero input (level 31); builder 60 inverts that zero
    input itself (level 1).  The sequential solver reaches builder 40 first"""
    L = _List(60)
    zero, x = L.acir_in(0), L.acir_in(L.fe())
    prev = zero
    for _ in range(30):
        w = L.fresh()
        L.add(WB.Product(w, prev, x))
        prev = w
    while len(L.b) < 40:
        L.add(WB.Constant(L.fresh(), len(L.b)))
    L.add(WB.Inverse(L.fresh(), prev))
    while len(L.b) < 60:
        L.add(WB.Constant(L.fresh(), len(L.b)))
    L.add(WB.Inverse(L.fresh(), zero))
    good = [L.fe(), L.acir[1]]
    return Case(L.b, L.acir, L.nxt + 1, dict(n_levels=32, n_items=61), 40, "inverse of zero", good)


def error_range_value_mid_wavefront():
    """200 lookups in range and one of 300 at position 100 (lane 36 of the second wavefront: its neighbours go on to count)"""
    L = _List(61)
    by = _bytes(L)
    bad = L.acir_in(300)
    look = [by[L.rnd.randrange(32)] for _ in range(200)]
    look.insert(100, bad)
    table = L.fresh(256)
    at = L.add(WB.MultiplicitiesForRange(table, 256, look))
    L.add(WB.Product(L.fresh(), table, table + 1))
    good = list(L.acir)
    good[32] = 30
    return Case(L.b, L.acir, L.nxt + 1, dict(n_levels=3, n_items=33 + 201 + 256 + 1, widths=[33, 0, 201, 256, 1, 0]), at, "multiplicity table", good)


DIGIT_OVERFLOW_BASES = {"total_20": [8, 8, 4], "total_63": [31, 32], "total_64": [32, 32], "total_65": [32, 33], "total_129": [32, 64, 33], "total_253": [61, 61, 61, 61, 9]}


def error_digit_overflow(name):
    """bases totalling less than 256 bits: 2^total - 1 decomposes, 2^total is "Higher order bits are not zero" """
    L = _List(62)
    bases = DIGIT_OVERFLOW_BASES[name]
    total = sum(bases)
    ws = [L.acir_in((1 << total) - 1), L.acir_in(1 << total), L.acir_in(5)]
    first = L.fresh(len(bases) * 3)
    at = L.add(WB.DigitalDecomposition(bases, ws, first))
    L.add(WB.Product(L.fresh(), first, first + 1))
    good = list(L.acir)
    good[1] = (1 << total) - 1
    n = (len(bases) + 1) * 3
    return Case(L.b, L.acir, L.nxt + 1, dict(n_levels=3, n_items=3 + n + 1, widths=[3, 0, n, 0, 1, 0]), at, "Higher order bits are not zero", good)


def error_spice_address():
    """an address equal to memory_length; memory_length - 1 passes"""
    L = _List(63)
    M = 6
    addr = [L.acir_in(v) for v in (M - 1, M, 0)]
    val = L.acir_in(L.fe())
    init = L.fresh(M)
    for c in range(M):
        L.acir_in(L.fe(), at=init + c)
    old, ts = L.fresh(), [L.fresh() for _ in range(3)]
    rv, rt = L.fresh(M), L.fresh(M)
    at = L.add(WB.SpiceWitnesses(M, init, [("load", addr[0], val, ts[0]), ("store", addr[1], old, val, ts[1]), ("load", addr[2], val, ts[2])], rv, rt))
    L.add(WB.Product(L.fresh(), rt + M - 1, old))
    good = list(L.acir)
    good[1] = M - 1
    return Case(L.b, L.acir, L.nxt + 1, dict(n_levels=3, blocks=1), at, "memory address", good)


ERROR_CASES = {"two_inverses": error_two_inverses, "range_value_mid_wavefront": error_range_value_mid_wavefront,
               **{f"digit_overflow_{k}": (lambda k=k: error_digit_overflow(k)) for k in DIGIT_OVERFLOW_BASES}, "spice_address": error_spice_address}


# ---- 7. reuse -----------------------------------------------------------------------------------------------------------------------
def reuse_program():
    """a range table, a bin-op table, a long sum and a Spice block in one program, and three ACIR vectors for it: the second has a
    lookup outside the range table (builder `panic_builder`), the first and third do not fail and share no counts"""
    L = _List(70)
    by = _bytes(L)
    rt_, bt = L.fresh(256), L.fresh(65536)
    at = L.add(WB.MultiplicitiesForRange(rt_, 256, [by[L.rnd.randrange(32)] for _ in range(150)]))
    L.add(WB.MultiplicitiesForBinOp(bt, [(("w", by[L.rnd.randrange(32)]), ("w", by[L.rnd.randrange(32)])) for _ in range(90)]))
    s = L.fresh()
    L.add(WB.Sum(s, [(L.fe(), rt_ + t) for t in range(256)]))  # the grand sum over the counts: a long sum one level up
    outs, _, _, _ = _spice_block(L, 16, 50, lambda k: L.acir[k % 32] % 16, pool=[by[0], by[1], s])  # no None here: which outputs are set must not depend on the inputs
    v = L.solved()
    L.add(WB.Sum(L.fresh(), [(None, w) for w in outs if v[w] is not None]))
    first = list(L.acir)
    rnd = random.Random(71)
    # inputs 0..31 are the bytes; the later ones are Spice addresses (below 16) or field elements
    third = [rnd.randrange(256) if i < 32 else rnd.randrange(16) if first[i] < 16 else rnd.randrange(P) for i in range(len(first))]
    second = list(third)
    second[9] = 256
    assert any(b == by[9] for b in L.b[at][3])
    return L.b, [first, second, third], L.nxt + 1, at
