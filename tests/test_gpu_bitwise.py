"""GPU: libprovekit_bitwise.so on the device.  The fused decomposition -- c, the 3 L digit columns and the multiplicities -- bit for bit
against Python ints (tests/bitwise_refs.py) for all three operations at every group count, on both sides of the LDS histogram's bound,
at 48 bits and over more than one tile, for edge values, random values, small values and full skew and for several grids, with nothing
written past an output's end and the operands unchanged; an operand outside the range or a given c that differs refused with the
smallest entry and its case named, whichever word of it is set; the proof bytes and claims against the Python reference; digit rows
outside the table and a wrong m reached through pkb_prove's refusals, with nothing written and the prover usable afterwards; the
arena's parts; the composition with libprovekit_whir.so; the C++ example."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import bitwise_refs as B  # noqa: E402
import fracsum_refs as F  # noqa: E402
import prodcheck_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(2, seed=53)
SENTINEL = 0xA5
KINDS = ("edges", "random", "small", "skew")
# (n, d, L): one group; two; (4, 6, 3) the spare group at the last LDS size; (4, 7, 3) the first device-atomic size; the u32-by-bytes
# shape; 48 bits; one wide digit; the last two sweep several tiles of 256 entries, and (11, 7, 3) with the spare group
SHAPES = [(1, 1, 1), (3, 4, 2), (4, 6, 3), (4, 7, 3), (4, 8, 4), (5, 12, 4), (5, 10, 1), (10, 8, 4), (11, 7, 3)]
PROOF_SHAPES = [(1, 1, 1), (3, 4, 2), (2, 6, 3), (3, 8, 4)]
OP_IDS = {B.AND: "and", B.XOR: "xor", B.OR: "or"}
SENTINEL_ELEMENT = np.full((1, 4), int.from_bytes(bytes([SENTINEL]) * 8, "little"), dtype=np.uint64)


def sentinel_fe(ctx, rows):
    """rows + 1 elements on the device with the sentinel behind the end: what a kernel does not write there stays.  Short buffers are
    sentinel bytes throughout; a long one (m of a wide digit) is zeroed, which no test takes for written: its non-zero bins must appear"""
    if rows <= 1 << 16:
        return ctx.upload(np.repeat(SENTINEL_ELEMENT, rows + 1, axis=0))
    buf = ctx.alloc_fe(rows + 1)
    ctx.zero(buf.ptr, 32 * rows)
    ctx.upload_into(buf.ptr + 32 * rows, SENTINEL_ELEMENT)
    return buf


def untouched(ctx, buf, rows):
    """the element behind the end is the sentinel"""
    return ctx.download(buf.ptr + 32 * rows, (1, 4), np.uint64).tobytes() == bytes([SENTINEL]) * 32


class Outputs:
    """c, the 3 L digit columns and m of a statement on the device, each with a sentinel element behind its end"""

    def __init__(self, ctx, shape):
        n, d, L = shape
        self.ctx, self.n, self.d, self.L = ctx, n, d, L
        self.c = sentinel_fe(ctx, 1 << n)
        self.digits = [sentinel_fe(ctx, 1 << n) for _ in range(3 * L)]
        self.m = sentinel_fe(ctx, 1 << (2 * d))

    def get(self):
        """(c, [a's, b's, c's digit columns], {y: m[y]} of the non-zero m[y]), every element of m read: the zero element is zero words
        in Montgomery form too"""
        cols = [K.unmont(self.ctx.download_fe(b, 1 << self.n)) for b in [self.c] + self.digits]
        m = self.ctx.download_fe(self.m, 1 << (2 * self.d))
        at = np.flatnonzero(m.any(axis=1))
        return cols[0], [cols[1 + j * self.L : 1 + (j + 1) * self.L] for j in range(3)], dict(zip(at.tolist(), K.unmont(m[at])))

    def past_the_end_untouched(self):
        return all(untouched(self.ctx, b, 1 << self.n) for b in [self.c] + self.digits) and untouched(self.ctx, self.m, 1 << (2 * self.d))

    def free(self):
        for b in [self.c, self.m] + self.digits:
            b.free()


@pytest.mark.parametrize("op", B.OPS, ids=OP_IDS.get)
@pytest.mark.parametrize("shape", SHAPES)
def test_decompose_is_the_references_bit_for_bit_for_every_input_and_grid(ctx, shape, op):
    from tools.pk_probes import lib as probes
    from provekit_amd import bitwise as bw

    n, d, L = shape
    assert bw.count_lds_max_d() == 6
    prover = bw.Prover(ctx, bw.Statement(n, op, d, L))
    pl = B.plan(d, L)
    assert (prover.plan.bits, prover.plan.c, prover.plan.digit_of) == (pl["bits"], pl["c"], pl["digit_of"])
    tiles = max(1, (1 << n) // (256 * probes.pk_probe_bitwise_decompose_items()))
    out = Outputs(ctx, shape)
    for kind in KINDS:
        a, b = B.columns(n, d, L, kind)
        if kind == "edges":
            pairs = list(zip(a, b))
            assert all(pair in pairs for pair in B.edge_pairs(d, L)[: 1 << n]) and (0, 0) in pairs
            assert n < 2 or ((1 << pl["bits"]) - 1,) * 2 in pairs
        want = B.decompose_bins(op, d, L, a, b)
        assert sum(want[2].values()) == pl["c"] << n and all(y < 1 << (2 * d) for y in want[2])
        if kind == "skew":
            assert max(want[2].values()) >= 1 << n  # every entry of a group in one bin
        if kind == "small" and L > 1:
            assert want[2].get(0, 0) >= (L - 1) << n  # every high digit row is row 0
        images = K.mont(a), K.mont(b)
        d_a, d_b = ctx.upload(images[0]), ctx.upload(images[1])
        for grid in (0, 1, 2 * tiles + 1):  # the library's rule, one workgroup, an odd count above the tiles
            assert probes.pk_probe_bitwise_set_grid(prover.handle, grid) == 0
            prover.decompose(d_a, d_b, out.c, out.digits, out.m)
            assert prover.first_bad == bw.NO_BAD_ENTRY
            got = out.get()
            assert got[0] == want[0], (kind, grid)
            assert got[1] == want[1], (kind, grid)
            assert got[2] == want[2], (kind, grid)
            assert out.past_the_end_untouched(), (kind, grid)
        if kind == "edges":  # c given: read and compared, the same digits and m
            given = K.mont(want[0])
            ctx.upload_into(out.c.ptr, given)
            prover.decompose(d_a, d_b, out.c, out.digits, out.m, c_given=True)
            assert prover.first_bad == bw.NO_BAD_ENTRY and out.get() == want and out.past_the_end_untouched()
            assert ctx.download_fe(out.c, 1 << n).tobytes() == given.tobytes()  # a given c is not written
        assert ctx.download_fe(d_a, 1 << n).tobytes() == images[0].tobytes() and ctx.download_fe(d_b, 1 << n).tobytes() == images[1].tobytes()  # the operands are unchanged
        d_a.free()
        d_b.free()
    out.free()
    prover.close()


def test_the_probe_runs_the_decomposition_alone_and_states_the_grids(ctx):
    from tools.pk_probes import lib as probes

    n, op, d, L = 10, B.XOR, 8, 4
    grids = (ctypes.c_uint * 3)()
    assert probes.pk_probe_bitwise_grids(n, op, d, L, grids) == 0 and list(grids) == [4, 64, 64]
    assert probes.pk_probe_bitwise_grids(24, B.AND, 6, 3, grids) == 0 and list(grids) == [1024, 4, 4]
    assert probes.pk_probe_bitwise_grids(20, 3, 8, 4, grids) == -1 and probes.pk_probe_bitwise_grids(20, op, 13, 4, grids) == -1
    a, b = B.columns(n, d, L, "random")
    want = B.decompose_bins(op, d, L, a, b)
    d_a, d_b, out = ctx.upload(K.mont(a)), ctx.upload(K.mont(b)), Outputs(ctx, (n, d, L))
    d_counts, d_bad = ctx.upload(np.zeros(1 << (2 * d), dtype=np.uint32)), ctx.upload(np.zeros(1, dtype=np.uint64))
    ptrs = (ctypes.c_void_p * (3 * L))(*[buf.ptr for buf in out.digits])
    for grid in (0, 3):
        ms = ctypes.c_float(-1)
        assert probes.pk_probe_bitwise_decompose(ctx.handle, n, op, d, L, d_a.ptr, d_b.ptr, out.c.ptr, 0, ptrs, d_counts.ptr, d_bad.ptr, out.m.ptr, grid, ctypes.byref(ms)) == 0
        assert ms.value >= 0 and out.get() == want and out.past_the_end_untouched()
        assert int(ctx.download(d_bad, (1,), np.uint64)[0]) == 2**64 - 1
        counts = ctx.download(d_counts, (1 << (2 * d),), np.uint32)
        assert {int(y): int(counts[y]) for y in np.flatnonzero(counts)} == want[2]
    # a prover's profile: where its last calls' time went
    from provekit_amd import bitwise as bw

    prover = bw.Prover(ctx, bw.Statement(n, op, d, L))
    phases = (ctypes.c_double(-1), ctypes.c_double(-1))
    assert probes.pk_probe_bitwise_profile(prover.handle, *[ctypes.byref(x) for x in phases]) == 0 and [x.value for x in phases] == [0, 0]  # nothing has run
    prover.decompose(d_a, d_b, out.c, out.digits, out.m)
    prover.prove(out.digits, out.m)
    assert probes.pk_probe_bitwise_profile(prover.handle, *[ctypes.byref(x) for x in phases]) == 0 and all(x.value > 0 for x in phases)
    prover.close()
    for buf in (d_a, d_b, d_counts, d_bad):
        buf.free()
    out.free()


BAD_SHAPES = [(3, 4, 2), (4, 8, 4), (10, 8, 4)]
BAD_CASES = ["a = 2^bits at entry 0", "a = 2^bits at the last entry", "a = 2^bits at two entries", "b = 2^bits at entry 0", "b = 2^bits at the last entry",
             "b = 2^bits at two entries", "p - 1", "2^64", "only word 3 set", "c off in one bit at the first entry", "c off in one bit at the last entry",
             "c is the wrong op of a, b"]


@pytest.mark.parametrize("where", BAD_CASES)
@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_a_failing_entry_is_refused_with_the_smallest_entry_and_its_case(ctx, shape, where):
    from provekit_amd import bitwise as bw
    from provekit_amd._lib import ProveKitHipError

    n, d, L = shape
    op = B.OPS[(BAD_CASES.index(where) + BAD_SHAPES.index(shape)) % 3]  # every operation meets every kind of case
    bits, entries = d * L, 1 << n
    good = B.columns(n, d, L, "random", seed=3)
    a, b = list(good[0]), list(good[1])
    c, c_given = None, where.startswith("c ")
    if where.endswith("= 2^bits at entry 0"):
        col, want = (a if where[0] == "a" else b), 0
        col[0] = 1 << bits
    elif where.endswith("= 2^bits at the last entry"):
        col, want = (a if where[0] == "a" else b), entries - 1
        col[entries - 1] = 1 << bits
    elif where.endswith("= 2^bits at two entries"):  # and the other operand fails behind both: the smallest entry wins, with its own case
        col, other, want = (a, b, entries // 2) if where[0] == "a" else (b, a, entries // 2)
        col[entries - 2], col[entries // 2], other[entries - 1] = 1 << bits, (1 << bits) + 7, 1 << bits
    elif where == "p - 1":
        a[entries // 3], want = P - 1, entries // 3
    elif where == "2^64":
        b[1], want = 1 << 64, 1
    elif where == "only word 3 set":  # the low 64 bits, and the low 192, are zero: inside every range if the high words were not read
        a[entries - 2], want = 1 << 192, entries - 2
    else:
        c = [B.apply(op, u, v) for u, v in zip(a, b)]
        if where == "c off in one bit at the first entry":
            c[0], want = c[0] ^ (1 << (bits - 1)), 0
        elif where == "c off in one bit at the last entry":
            c[entries - 1], want = c[entries - 1] ^ 1, entries - 1
        else:
            wrong = B.OPS[(op + 1) % 3]
            c = [B.apply(wrong, u, v) for u, v in zip(a, b)]
            want = next(x for x in range(entries) if c[x] != B.apply(op, a[x], b[x]))
    case = B.first_bad(op, d, L, a, b, c)
    assert case is not None and case[0] == want
    reason = {"a": "a is not below 2\\^%d" % bits, "b": "b is not below 2\\^%d" % bits, "c": "c is not a %s b" % OP_IDS[op]}[case[1]]
    assert case[1] == ("c" if c_given else where[0] if where[1:3] == " =" else {"p - 1": "a", "2^64": "b", "only word 3 set": "a"}[where])
    prover = bw.Prover(ctx, bw.Statement(n, op, d, L))
    d_a, d_b, out = ctx.upload(K.mont(a)), ctx.upload(K.mont(b)), Outputs(ctx, shape)
    if c_given:
        ctx.upload_into(out.c.ptr, K.mont(c))
    with pytest.raises(ProveKitHipError, match="entry %d: %s" % (want, reason)) as e:
        prover.decompose(d_a, d_b, out.c, out.digits, out.m, c_given=c_given)
    assert e.value.code == bw.ERR_UNSATISFIED and prover.first_bad == want
    assert out.past_the_end_untouched()  # the outputs are not meaningful; nothing is written outside them
    # the prover stays usable
    ctx.upload_into(d_a.ptr, K.mont(good[0]))
    ctx.upload_into(d_b.ptr, K.mont(good[1]))
    prover.decompose(d_a, d_b, out.c, out.digits, out.m)
    assert prover.first_bad == bw.NO_BAD_ENTRY and out.get() == B.decompose_bins(op, d, L, *good) and out.past_the_end_untouched()
    d_a.free()
    d_b.free()
    out.free()
    prover.close()


def test_arena_bytes_states_its_parts(ctx):
    from provekit_amd import bitwise as bw, tuplelookup as tl

    def up(nbytes):
        return (nbytes + 63) // 64 * 64

    for n, op, d, L in ((1, B.AND, 1, 1), (9, B.XOR, 8, 4), (12, B.OR, 6, 3), (7, B.XOR, 4, 2), (5, B.AND, 10, 1)):
        # the table's three columns; the counts; the cell of the first bad entry
        own = 3 * up(32 << (2 * d)) + up(4 << (2 * d)) + 64
        assert bw.arena_bytes(bw.Statement(n, op, d, L)) == own + tl.arena_bytes(tl.Statement(n, 2 * d, 3, B.plan(d, L)["c"], 1))
        prover = bw.Prover(ctx, bw.Statement(n, op, d, L))  # and a prover of it is made and given back
        prover.close()
    assert bw.arena_bytes(bw.Statement(9, B.AND, 8, 3)) == bw.arena_bytes(bw.Statement(9, B.OR, 8, 4))  # the spare group: four groups either way


def same_claims(claims, ref):
    for name in ("z_lo", "z_t", "pow2"):
        assert K.unmont(getattr(claims, name)) == ref[name], name
    assert [K.unmont(row) for row in claims.digit_coeff] == ref["digit_coeff"]
    assert K.unmont(claims.digits_value) == [ref["digits_value"]] and K.unmont(claims.m_value) == [ref["m_value"]]


_REFERENCE = {}


def reference(n, op, d, L, kind, seed):
    """the Python reference's columns and proof of a case, computed once"""
    key = (n, op, d, L, kind, seed)
    if key not in _REFERENCE:
        a, b = B.columns(n, d, L, kind, seed=seed)
        c, digits, m = B.decompose(op, d, L, a, b)
        _REFERENCE[key] = (a, b, c, digits, m, B.prove(n, op, d, L, digits, m, BIND))
    return _REFERENCE[key]


def flat(parts):
    return [v for part in parts for v in part]


@pytest.mark.parametrize("op", B.OPS, ids=OP_IDS.get)
@pytest.mark.parametrize("shape", PROOF_SHAPES)
def test_proof_bytes_and_claims_are_the_references_and_a_prover_proves_two_column_sets(ctx, shape, op):
    from provekit_amd import bitwise as bw
    from provekit_amd._lib import ProveKitHipError

    n, d, L = shape
    stmt, bind = bw.Statement(n, op, d, L, 2), K.mont(BIND)
    prover = bw.Prover(ctx, stmt)
    out = Outputs(ctx, shape)
    proofs = []
    for kind in ("edges", "random"):  # the same prover, two column sets
        whole = kind == "edges" or 2 * d <= 12  # the reference prover walks the whole table: at 2^16 rows it proves one column set
        if whole:
            a, b, c, digits, m, ref = reference(n, op, d, L, kind, len(proofs))
        else:
            a, b = B.columns(n, d, L, kind, seed=len(proofs))
            c, digits, m = B.decompose(op, d, L, a, b)
        d_a, d_b = ctx.upload(K.mont(a)), ctx.upload(K.mont(b))
        prover.decompose(d_a, d_b, out.c, out.digits, out.m)
        proof, claims = prover.prove(out.digits, out.m, bind)
        assert len(proof) == bw.proof_bytes(stmt) == prover.last_len
        res, side, layer, seen = bw.verify(stmt, proof, bind)
        assert res.accepted and res.offset == len(proof) and (side, layer) == ("F", 0), res
        if whole:
            assert proof == ref["proof"]
            same_claims(claims, ref)
            same_claims(seen, ref)
        else:  # the reference's verifier accepts it and derives the same claims
            check, _, _, _, ref = B.verify(n, op, d, L, proof, BIND)
            assert check == "NONE"
            same_claims(claims, ref)
            same_claims(seen, ref)
        # the five claims hold of the columns' true evaluations, computed in Python
        abc, digit_evals, m_eval = B.evaluations((a, b, c), digits, m, ref)
        assert B.check_claims(ref, abc, digit_evals, m_eval) == "NONE"
        assert bw.check_claims(stmt, seen, K.mont(abc), K.mont(flat(digit_evals)), K.mont([m_eval])) == "NONE"
        assert bw.check_claims(stmt, seen, K.mont([abc[0], abc[1], (abc[2] + 1) % P]), K.mont(flat(digit_evals)), K.mont([m_eval])) == "RECOMPOSE_C"
        assert prover.prove(out.digits, out.m, bind)[0] == proof  # again: the same bytes
        got = out.get()
        assert (got[0], got[1]) == (c, digits) and got[2] == B.count_bins(d, L, digits) and out.past_the_end_untouched()  # the caller's columns are unchanged
        proofs.append(proof)
        d_a.free()
        d_b.free()
    assert proofs[0] != proofs[1]
    # a short buffer: the length is told, nothing is proved or written, the prover stays usable
    prover.fill = SENTINEL
    with pytest.raises(ProveKitHipError, match="the proof buffer holds") as e:
        prover.prove(out.digits, out.m, bind, capacity=len(proof) - 1)
    assert e.value.code == -1 and prover.last_len == len(proof) and bytes(prover.buffer) == bytes([SENTINEL]) * (len(proof) - 1)
    assert prover.prove(out.digits, out.m, bind)[0] == proof
    out.free()
    prover.close()


@pytest.mark.parametrize("shape, op", [((3, 4, 2), B.XOR), ((2, 6, 3), B.AND), ((3, 4, 2), B.OR)])
def test_rows_outside_the_table_and_a_wrong_m_are_refused_with_the_digit_and_the_entry(ctx, shape, op):
    """digit columns that did not come from pkb_decompose: one row with c_i wrong, one with a_i = 2^d (outside every table of d-bit
    digits), and a wrong m.  With the spare group ((2, 6, 3)) a row of digit 0 outside the table is named in its own group"""
    from provekit_amd import bitwise as bw
    from provekit_amd._lib import ProveKitHipError

    n, d, L = shape
    stmt, bind = bw.Statement(n, op, d, L, 2), K.mont(BIND)
    a, b, c, digits, m, ref = reference(n, op, d, L, "edges", 0)
    prover = bw.Prover(ctx, stmt)
    prover.fill = SENTINEL
    d_m = ctx.upload(K.mont(m))
    good = [ctx.upload(K.mont(col)) for col in flat(digits)]
    honest = prover.prove(good, d_m, bind)[0]
    assert honest == ref["proof"]

    def refused(changed, changed_m, reason):
        bad = [ctx.upload(K.mont(col)) for col in flat(changed)]
        d_bad_m = ctx.upload(K.mont(changed_m))
        with pytest.raises(ProveKitHipError, match=reason) as e:
            prover.prove(bad, d_bad_m, bind)
        assert e.value.code == bw.ERR_UNSATISFIED
        assert bytes(prover.buffer) == bytes([SENTINEL]) * len(honest)  # nothing is written
        assert prover.prove(good, d_m, bind)[0] == honest  # and the same prover then proves the good columns
        for buf in bad + [d_bad_m]:
            buf.free()

    def changed_at(j, i, x, value):
        out = [[list(col) for col in part] for part in digits]
        out[j][i][x] = value
        return out

    size = 1 << n
    named = r"entry %d of digit %d \(the row \(a_i, b_i, c_i\) must be a row of the %s table of %d-bit digits\) is not in the table: .*a row is not in t: stacked index %d "
    x, i = size - 1, L - 1  # c_i wrong in the top digit at the last entry
    refused(changed_at(2, i, x, digits[2][i][x] ^ 1), m, named % (x, i, OP_IDS[op], d, size * i + x))
    x, i = 1, min(1, L - 1)  # a_i = 2^d
    refused(changed_at(0, i, x, 1 << d), m, named % (x, i, OP_IDS[op], d, size * i + x))
    x = 2  # digit 0: looked up twice when there is a spare group, named in its own
    refused(changed_at(1, 0, x, 1 << d), m, named % (x, 0, OP_IDS[op], d, x))
    refused(digits, [(m[0] + 1) % P] + m[1:], "m is wrong")
    for buf in good + [d_m]:
        buf.free()
    prover.close()


def small_whir_config(n_vars, batch):
    """tests/whir_pcs_cases.py's cheap configuration, with a folding factor that fits three variables"""
    import whir_pcs_cases as W
    from provekit_amd.scheme import WhirConfig

    if n_vars >= 4:
        return W.small_config(n_vars, batch)
    c = WhirConfig.derive(n_vars, batch_size=batch, folding_factor=2)
    c.pow_bits = [4.0] * c.n_rounds
    c.final_pow_bits = 4.0
    c.num_queries = [20, 12, 9, 8][: c.n_rounds]
    return c


def test_composition_with_the_commitment_scheme(ctx):
    """(3, XOR, 8, 4): commit {a, b, c}, the digits of each column as a batch and m, bind the five roots, decompose, prove, verify, open
    the four batches at z_lo and m at z_t, verify the openings, check the claims on the opened values; with one evaluation changed the
    claims fail"""
    from provekit_amd import bitwise as bw, whir_pcs

    n, op, d, L = 3, B.XOR, 8, 4
    a, b = B.columns(n, d, L, "edges")
    d_a, d_b, out = ctx.upload(K.mont(a)), ctx.upload(K.mont(b)), Outputs(ctx, (n, d, L))
    plain = bw.Prover(ctx, bw.Statement(n, op, d, L))
    plain.decompose(d_a, d_b, out.c, out.digits, out.m)
    plain.close()
    assert out.get() == B.decompose_bins(op, d, L, a, b)
    cfgs = [small_whir_config(n, 3)] + [small_whir_config(n, L)] * 3 + [small_whir_config(2 * d, 1)]
    schemes = [whir_pcs.Scheme(ctx, cfg) for cfg in cfgs]
    batches = [[d_a, d_b, out.c]] + [out.digits[j * L : (j + 1) * L] for j in range(3)] + [[out.m]]
    coms = [scheme.commit(batch) for scheme, batch in zip(schemes, batches)]
    bind = K.mont([int.from_bytes(com.root(), "little") for com in coms])
    stmt = bw.Statement(n, op, d, L, 5)
    prover = bw.Prover(ctx, stmt)
    proof, _ = prover.prove(out.digits, out.m, bind)
    res, side, layer, seen = bw.verify(stmt, proof, bind)
    assert res.accepted, res
    opened = []
    for scheme, cfg, com, points in zip(schemes, cfgs, coms, [seen.z_lo[None]] * 4 + [seen.z_t[None]]):
        _, opening = scheme.open(com, points)
        wres, wevals = whir_pcs.verify(cfg, points, opening, expected_root=com.root())
        assert wres.accepted, wres
        opened.append(wevals)
    evs = [opened[0][:, 0], np.concatenate([opened[1 + j][:, 0] for j in range(3)]), opened[4][0, 0]]
    assert bw.check_claims(stmt, seen, *evs) == "NONE"
    for which, at, name in ((0, 0, "RECOMPOSE_A"), (0, 1, "RECOMPOSE_B"), (0, 2, "RECOMPOSE_C"), (1, 2 * L + 1, "DIGITS"), (2, None, "M")):
        changed = [x.copy() for x in evs]
        if at is None:
            changed[which] = K.mont([(K.unmont(changed[which][None])[0] + 1) % P])[0]
        else:
            changed[which][at] = K.mont([(K.unmont(changed[which][at][None])[0] + 1) % P])[0]
        assert bw.check_claims(stmt, seen, *changed) == name
    # other roots: another seed, rejected
    assert not bw.verify(stmt, proof, K.mont([1, 2, 3, 4, 5]))[0].accepted
    for closing in coms + [prover] + schemes:
        closing.close()
    d_a.free()
    d_b.free()
    out.free()


def test_the_cpp_demo_commits_proves_opens_checks_the_claims_and_sees_the_refusals():
    demo = os.path.join(ROOT, "examples", "bitwise_pcs_demo")
    assert os.path.exists(demo), "examples/bitwise_pcs_demo is built by __graft_entry__.build()"
    p = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "accepted" in p.stdout and "claims hold" in p.stdout
    assert "entry 7: b is not below 2^32" in p.stdout and "entry 9: c is not a xor b" in p.stdout
    assert "entry 5 of digit 2" in p.stdout and "is not in the table" in p.stdout
