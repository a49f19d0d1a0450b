"""GPU: libprovekit_memcheck.so on the device.  The trace builder bit for bit against a plain replay loop (tests/memcheck_refs.py) at
shapes that cross its seams, for every address pattern and several grids, with nothing written past an output's end, the inputs
unchanged and a bad address refused with the smallest index; the two leaf kernels bit-exact against Python ints; the proof bytes and
claims against the Python reference; a prover reused, a short buffer, the refusals with their reasons -- the future-read trace among
them; one larger size against pkw_evaluate; the composition with libprovekit_whir.so; the C++ example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import memcheck_refs as M  # noqa: E402
import prodcheck_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu
P = K.P
BIND = K.random_elements(3, seed=47)
GRIDS = (1, 3, 0)  # workgroups (0: the library's rule)
PATTERNS = ("one address", "last cell", "distinct", "round robin", "random")
BETAS = ("0", "1", "p-1", "random")
SENTINEL = 0xA5
OPS, CELLS = ("a", "wv", "rv", "rt", "m"), ("init", "fin", "ft")


def sweep(n, items):
    """an int, or "s-1", "s", "s+1": around 2^s rows, one workgroup's sweep at `items` rows per lane"""
    if isinstance(n, int):
        return n
    rows = 256 * items
    assert rows & (rows - 1) == 0
    return rows.bit_length() - 1 + int(n[1:] or 0)


def cells_for(n):
    """k in {1, 3, n - 2, n + 2}, kept inside 1 .. 27"""
    return sorted({min(max(k, 1), 27) for k in (1, 3, n - 2, n + 2)})


def sentinel_fe(ctx, rows):
    """rows + 1 elements of sentinel bytes on the device: what a kernel does not write stays"""
    return ctx.upload(np.full((rows + 1, 4), int.from_bytes(bytes([SENTINEL]) * 8, "little"), dtype=np.uint64))


def untouched(ctx, buf, rows):
    return ctx.download_fe(buf, rows + 1)[rows].tobytes() == bytes([SENTINEL]) * 32


class Device:
    """a trace's columns on the device; `outputs` allocates the builder's six with a sentinel element behind each"""

    def __init__(self, ctx, n, k):
        self.ctx, self.n, self.k, self.bufs = ctx, n, k, {}

    def put(self, tr, names=M.COLUMNS):
        for name in names:
            if name in self.bufs:
                self.bufs[name].free()
            self.bufs[name] = self.ctx.upload(K.mont(tr[name]))
        return self

    def outputs(self):
        for name in ("a", "rv", "rt", "m", "fin", "ft"):
            if name in self.bufs:
                self.bufs[name].free()
            self.bufs[name] = sentinel_fe(self.ctx, 1 << (self.n if name in OPS else self.k))
        return self

    def get(self, name):
        return K.unmont(self.ctx.download_fe(self.bufs[name], 1 << (self.n if name in OPS else self.k)))

    def free(self):
        for buf in self.bufs.values():
            buf.free()
        self.bufs = {}


def trace_case(ctx, prover, n, k):
    """every pattern at one (n, k)"""
    from tools.pk_probes import lib as probes
    from provekit_amd import memcheck as mc

    dev = Device(ctx, n, k)
    for number, name in enumerate(PATTERNS):
        if name == "distinct" and n > k:
            continue
        addr, wv, init = M.random_ops(n, k, seed=1000 * n + 10 * k + number, pattern_name=name)
        want = M.replay(addr, wv, init)
        if name == "distinct" and n < k:
            assert sum(t == 0 for t in want["ft"]) == (1 << k) - (1 << n)  # cells left untouched
        assert all(0 <= t <= i for i, t in enumerate(want["rt"]))
        dev.put(want, ("wv", "init"))
        addr_image = np.asarray(addr, dtype=np.uint32)
        d_addr = ctx.upload(addr_image)
        for grid in GRIDS if name in ("random", "round robin") else (0,):
            assert probes.pk_probe_mem_set_grid(prover.handle, grid) == 0
            dev.outputs()
            b = dev.bufs
            prover.trace(d_addr, b["wv"], b["init"], b["a"], b["rv"], b["rt"], b["fin"], b["ft"], b["m"])
            assert prover.first_bad == mc.NO_BAD_INDEX
            for col in ("a", "rv", "rt", "fin", "ft", "m"):
                assert dev.get(col) == want[col], (name, grid, col)
                assert untouched(ctx, b[col], 1 << (n if col in OPS else k)), (name, grid, col)  # nothing past the end
        # the inputs are unchanged
        assert ctx.download(d_addr, (1 << n,), np.uint32).tobytes() == addr_image.tobytes()
        assert dev.get("wv") == wv and dev.get("init") == init
        d_addr.free()
    dev.free()


@pytest.mark.parametrize("n", [1, 3, "s-1", "s", "s+1"])
def test_the_trace_builder_is_the_replay_loop_for_every_pattern_and_grid(ctx, n):
    from tools.pk_probes import lib as probes
    from provekit_amd import memcheck as mc

    n = sweep(n, probes.pk_probe_mem_trace_items())
    for k in cells_for(n):
        prover = mc.Prover(ctx, mc.Statement(n, k))
        trace_case(ctx, prover, n, k)
        prover.close()


@pytest.mark.parametrize("where", ["operation 0", "the last operation", "two operations", "2^32 - 1"])
@pytest.mark.parametrize("n, k", [(1, 1), (5, 3), (11, 4)])
def test_an_address_outside_the_memory_is_refused_with_the_smallest_index(ctx, n, k, where):
    from provekit_amd import memcheck as mc
    from provekit_amd._lib import ProveKitHipError

    addr, wv, init = M.random_ops(n, k, seed=3)
    rows = 1 << n
    if where == "operation 0":
        addr[0], want = 1 << k, 0
    elif where == "the last operation":
        addr[rows - 1], want = 1 << k, rows - 1
    elif where == "two operations":
        addr[rows - 1], addr[rows // 2], want = 1 << k, (1 << k) + 7, rows // 2
    else:
        addr[rows // 2], want = 2**32 - 1, rows // 2
    prover = mc.Prover(ctx, mc.Statement(n, k))
    dev = Device(ctx, n, k).put({"wv": wv, "init": init}, ("wv", "init")).outputs()
    d_addr, b = ctx.upload(np.asarray(addr, dtype=np.uint32)), dev.bufs
    with pytest.raises(ProveKitHipError, match="operation %d: its address is outside" % want) as e:
        prover.trace(d_addr, b["wv"], b["init"], b["a"], b["rv"], b["rt"], b["fin"], b["ft"], b["m"])
    assert e.value.code == mc.ERR_BAD_ARG and prover.first_bad == want
    for col in ("a", "rv", "rt", "fin", "ft", "m"):  # the bad address was followed nowhere past a table's end
        assert untouched(ctx, b[col], 1 << (n if col in OPS else k)), col
    # the prover stays usable
    good = M.replay(*M.random_ops(n, k, seed=4))
    dev.put(good, ("wv", "init"))
    ctx.upload_into(d_addr.ptr, np.asarray(good["a"], dtype=np.uint32))
    prover.trace(d_addr, b["wv"], b["init"], b["a"], b["rv"], b["rt"], b["fin"], b["ft"], b["m"])
    assert prover.first_bad == mc.NO_BAD_INDEX and all(dev.get(col) == good[col] for col in ("rv", "rt", "fin", "ft", "m"))
    d_addr.free()
    dev.free()
    prover.close()


def test_arena_bytes_states_the_tables_the_sorts_storage_and_the_three_inner_provers(ctx):
    # on the device: the sort is asked for its temporary storage, which it sizes for the device it runs on
    from provekit_amd import fracsum as fs, memcheck as mc

    for n, k in ((1, 1), (12, 7), (5, 13)):
        inner = fs.arena_bytes(fs.Statement(n + 1, 1, 0)) + fs.arena_bytes(fs.Statement(k + 1, 1, 0)) + fs.arena_bytes(fs.LookupStatement(n, n, 1))
        # two stacked tables and two sign tables; f and t; keys and sorted keys; counts; the cell of the first bad index
        own = 32 * 2 * ((2 << n) + (2 << k)) + 32 * 2 * (1 << n) + 8 * 2 * (1 << n) + 4 * (1 << n) + 8
        # ... and the sort's temporary storage, which the sort is asked for: at least a byte, and no more than another two key arrays and a MiB
        assert inner + own < mc.arena_bytes(mc.Statement(n, k)) <= inner + own + 16 * (1 << n) + (1 << 20)


def check_leaves(ctx, n, k, beta_kind, zero_leaf, seed):
    import random

    from tools.pk_probes import lib as probes
    from provekit_amd import memcheck as mc

    rng = random.Random(seed)
    # the leaf kernels take any columns: random elements everywhere, p - 1 and 0 among them
    tr = {name: [rng.choice((0, P - 1, rng.randrange(P))) if x % 5 == 0 else rng.randrange(P) for x in range(1 << (n if name in OPS else k))] for name in M.COLUMNS}
    beta = {"0": 0, "1": 1, "p-1": P - 1, "random": rng.randrange(P)}[beta_kind]
    gamma = rng.randrange(P)
    if zero_leaf:  # gamma is the last write's compressed triple
        i = (1 << n) - 1
        gamma = (tr["a"][i] + beta * tr["wv"][i] + beta * beta * (i + 1)) % P
    q_ops, q_mem, f = M.leaves(tr, gamma, beta)
    if zero_leaf:
        assert q_ops[(1 << n) - 1] == 0
    want = [K.mont(q_ops), K.mont(q_mem), K.mont(f)]
    dev = Device(ctx, n, k).put(tr)
    sizes = (2 << n, 2 << k, 1 << n)
    g, b = K.mont([gamma]), K.mont([beta])
    cols = mc.columns(dev.bufs)
    for grid in (None,) + GRIDS:  # None: the C ABI's entry, the library's grid
        outs = [sentinel_fe(ctx, size) for size in sizes]
        if grid is None:
            mc.leaves(ctx, n, k, dev.bufs, g, b, *outs)
        else:
            assert probes.pk_probe_mem_leaves(ctx.handle, n, k, C.addressof(cols), g.ctypes.data, b.ctypes.data, outs[0].ptr, outs[1].ptr, outs[2].ptr, grid, None) == 0
        for out, size, image in zip(outs, sizes, want):
            assert np.array_equal(ctx.download_fe(out, size), image) and untouched(ctx, out, size), (grid, size)
            out.free()
    for name in M.COLUMNS:  # the caller's columns are unchanged
        assert dev.get(name) == tr[name]
    dev.free()


def test_the_leaf_kernels_are_bit_exact_over_the_sweep_for_every_grid(ctx):
    # the kernels' paths depend on the shape (tile edges, the second half's offset) and never on the values: the beta kinds go round
    from tools.pk_probes import lib as probes

    items = probes.pk_probe_mem_leaf_items()
    shapes = [(n, k) for n in (sweep(s, items) for s in (1, 3, "s-1", "s", "s+1")) for k in cells_for(n)]
    for i, (n, k) in enumerate(shapes):
        check_leaves(ctx, n, k, BETAS[i % 4], zero_leaf=i % 5 == 0, seed=i)


@pytest.mark.parametrize("zero_leaf", [False, True], ids=["", "zero leaf"])
@pytest.mark.parametrize("beta_kind", BETAS)
def test_the_leaf_kernels_are_bit_exact_for_every_kind_of_beta(ctx, beta_kind, zero_leaf):
    check_leaves(ctx, 3, 2, beta_kind, zero_leaf, seed=77)


SCALARS = ("gamma", "beta", "ops_value", "mem_value", "rt_value", "m_value")
VECTORS = ("z_ops", "z_mem", "z_f", "z_t", "ops_coeff", "mem_coeff")


def same_claims(claims, ref):
    for name in SCALARS:
        assert K.unmont(getattr(claims, name)) == [ref[name]], name
    for name in VECTORS:
        assert K.unmont(getattr(claims, name)) == ref[name], name


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (3, 2), (4, 4)])
def test_proof_bytes_and_claims_are_the_references_and_a_prover_proves_two_traces(ctx, size):
    from provekit_amd import memcheck as mc
    from provekit_amd._lib import ProveKitHipError

    n, k = size
    stmt, bind = mc.Statement(n, k, 3), K.mont(BIND)
    prover = mc.Prover(ctx, stmt)
    dev = Device(ctx, n, k)
    proofs = []
    for seed, name in ((1, "random"), (2, "one address")):  # the same prover, two traces
        addr, wv, init = M.random_ops(n, k, seed=100 * n + k + seed, pattern_name=name)
        tr = M.replay(addr, wv, init)
        ref = M.prove(n, k, tr, BIND)
        dev.put(tr, ("wv", "init")).outputs()
        d_addr, b = ctx.upload(np.asarray(addr, dtype=np.uint32)), dev.bufs
        prover.trace(d_addr, b["wv"], b["init"], b["a"], b["rv"], b["rt"], b["fin"], b["ft"], b["m"])
        proof, claims = prover.prove(dev.bufs, bind)
        assert proof == ref["proof"] and len(proof) == mc.proof_bytes(stmt)
        same_claims(claims, ref)
        res, side, layer, seen = mc.verify(stmt, proof, bind)
        assert res.accepted and res.offset == len(proof), res
        same_claims(seen, ref)
        assert prover.prove(dev.bufs, bind)[0] == proof  # again: the same bytes
        proofs.append(proof)
        d_addr.free()
    assert proofs[0] != proofs[1]
    # a short buffer: the length is told, nothing is proved or written, the prover stays usable
    prover.fill = SENTINEL
    with pytest.raises(ProveKitHipError, match="the proof buffer holds") as e:
        prover.prove(dev.bufs, bind, capacity=len(proof) - 1)
    assert e.value.code == -1 and prover.last_len == len(proof) and bytes(prover.buffer) == bytes([SENTINEL]) * (len(proof) - 1)
    assert prover.prove(dev.bufs, bind)[0] == proof
    for name in M.COLUMNS:  # the caller's columns are unchanged
        assert dev.get(name) == tr[name]
    dev.free()
    prover.close()


def test_every_inconsistent_trace_is_refused_with_its_reason_and_nothing_is_written(ctx):
    from provekit_amd import memcheck as mc
    from provekit_amd._lib import ProveKitHipError

    n, k = 4, 3
    stmt, bind = mc.Statement(n, k, 3), K.mont(BIND)
    tr = M.replay(*M.random_ops(n, k, seed=12))
    honest_ref = M.prove(n, k, tr, BIND)
    prover = mc.Prover(ctx, stmt)
    prover.fill = SENTINEL
    good = Device(ctx, n, k).put(tr)
    honest, _ = prover.prove(good.bufs, bind)
    assert honest == honest_ref["proof"]

    def refused(changed, reason):
        bad = Device(ctx, n, k).put(changed)
        with pytest.raises(ProveKitHipError, match=reason) as e:
            prover.prove(bad.bufs, bind)
        assert e.value.code == mc.ERR_UNSATISFIED
        assert bytes(prover.buffer) == bytes([SENTINEL]) * len(honest)  # nothing is written
        assert prover.prove(good.bufs, bind)[0] == honest  # and the same prover then proves the good trace
        bad.free()

    def changed(column, index, value=None):
        out = {c: list(v) for c, v in tr.items()}
        out[column][index] = (out[column][index] + 1) % P if value is None else value
        return out

    refused(changed("rv", 5), "the multisets differ")
    refused(changed("fin", 2), "the multisets differ")
    refused(changed("m", 1), "a read is not older than its operation, or m is wrong")
    # gamma forced onto a leaf: gamma and beta depend on the statement and the bind elements alone, so the value is chosen after
    # them and no fixed transcript is needed.  The last write's wv makes its triple compress to gamma
    gamma, beta, _ = M.challenges(n, k, BIND)
    i = (1 << n) - 1
    hit = (gamma - tr["a"][i] - beta * beta * (i + 1)) * pow(beta, -1, P) % P
    on_leaf = changed("wv", i, hit)
    assert M.leaves(on_leaf, gamma, beta)[0][i] == 0
    refused(on_leaf, "a denominator is zero: gamma is a compressed triple of side OPS")
    good.free()
    prover.close()


def test_the_future_read_trace_balances_and_the_prover_refuses_it_naming_the_time_check(ctx):
    from provekit_amd import memcheck as mc
    from provekit_amd._lib import ProveKitHipError

    tr = M.future_read()
    written, read = M.triples(tr)
    assert written == read
    forged = M.prove(1, 1, tr, BIND, validate=False)
    assert forged["balanced"]  # the balance holds: part 1 of the claim is true of this trace
    stmt, bind = mc.Statement(1, 1, 3), K.mont(BIND)
    prover = mc.Prover(ctx, stmt)
    prover.fill = SENTINEL
    bad = Device(ctx, 1, 1).put(tr)
    with pytest.raises(ProveKitHipError, match="a read is not older than its operation") as e:
        prover.prove(bad.bufs, bind)
    assert e.value.code == mc.ERR_UNSATISFIED and bytes(prover.buffer) == bytes([SENTINEL]) * mc.proof_bytes(stmt)
    # the same prover proves what the memory really does with these operations
    real = M.replay(tr["a"], tr["wv"], tr["init"])
    good = Device(ctx, 1, 1).put(real)
    proof, _ = prover.prove(good.bufs, bind)
    assert proof == M.prove(1, 1, real, BIND)["proof"] and mc.verify(stmt, proof, bind)[0].accepted
    bad.free()
    good.free()
    prover.close()


def evaluations(ctx, whir_pcs, bufs, n, k, claims):
    """the nine evaluations of the claims from the device columns (pkw_evaluate)"""
    ops = whir_pcs.evaluate(ctx, [bufs[c] for c in ("a", "wv", "rv", "rt")], n, np.stack([claims.z_ops, claims.z_f]))
    mem = whir_pcs.evaluate(ctx, [bufs[c] for c in ("init", "fin", "ft")], k, claims.z_mem[None])
    m = whir_pcs.evaluate(ctx, [bufs["m"]], n, claims.z_t[None])
    return ops[:, 0], mem[:, 0], ops[3, 1], m[0, 0]


def test_one_larger_trace_is_verified_and_its_claims_hold_of_the_columns_evaluations(ctx):
    """n = 12, k = 10: nothing is proved in Python at this size"""
    from provekit_amd import memcheck as mc, whir_pcs

    n, k = 12, 10
    addr, wv, init = M.random_ops(n, k, seed=1210)
    want = M.replay(addr, wv, init)
    stmt = mc.Statement(n, k)
    prover = mc.Prover(ctx, stmt)
    dev = Device(ctx, n, k).put(want, ("wv", "init")).outputs()
    d_addr, b = ctx.upload(np.asarray(addr, dtype=np.uint32)), dev.bufs
    prover.trace(d_addr, b["wv"], b["init"], b["a"], b["rv"], b["rt"], b["fin"], b["ft"], b["m"])
    assert all(dev.get(col) == want[col] for col in ("a", "rv", "rt", "fin", "ft", "m"))
    proof, claims = prover.prove(dev.bufs)
    assert len(proof) == mc.proof_bytes(stmt)
    res, side, layer, seen = mc.verify(stmt, proof)
    assert res.accepted and res.offset == len(proof), res
    for name in SCALARS + VECTORS:
        assert np.array_equal(getattr(seen, name), getattr(claims, name)), name
    ops, mem, rt, m = evaluations(ctx, whir_pcs, dev.bufs, n, k, seen)
    assert mc.check_claims(stmt, seen, ops, mem, rt, m) == "NONE"
    for which, index in (("OPS", 2), ("MEM", 1)):
        o, c = ops.copy(), mem.copy()
        target = o if which == "OPS" else c
        target[index] = K.mont([(K.unmont(target[index])[0] + 1) % P])[0]
        assert mc.check_claims(stmt, seen, o, c, rt, m) == which
    assert mc.check_claims(stmt, seen, ops, mem, m, m) == "RT" and mc.check_claims(stmt, seen, ops, mem, rt, rt) == "M"
    d_addr.free()
    dev.free()
    prover.close()


def test_composition_with_the_commitment_scheme(ctx):
    """commit the operation columns as one batch, the memory columns as another and m, bind the roots, prove, open the operation columns
    at z_ops and z_f in one opening, the memory columns at z_mem and m at z_t, verify the openings, check the claims on the opened
    values; with one evaluation changed the claims fail"""
    import whir_pcs_cases as W
    from provekit_amd import memcheck as mc, whir_pcs

    n, k = 6, 4
    tr = M.replay(*M.random_ops(n, k, seed=64))
    dev = Device(ctx, n, k).put(tr)
    b = dev.bufs
    cfgs = [W.small_config(n, 4), W.small_config(k, 3), W.small_config(n, 1)]
    schemes = [whir_pcs.Scheme(ctx, cfg) for cfg in cfgs]
    groups = [[b[c] for c in ("a", "wv", "rv", "rt")], [b[c] for c in ("init", "fin", "ft")], [b["m"]]]
    coms = [scheme.commit(group) for scheme, group in zip(schemes, groups)]
    bind = K.mont([int.from_bytes(com.root(), "little") for com in coms])
    stmt = mc.Statement(n, k, 3)
    prover = mc.Prover(ctx, stmt)
    proof, _ = prover.prove(b, bind)
    res, side, layer, seen = mc.verify(stmt, proof, bind)
    assert res.accepted, res
    opened = []
    for scheme, cfg, com, points in zip(schemes, cfgs, coms, (np.stack([seen.z_ops, seen.z_f]), seen.z_mem[None], seen.z_t[None])):
        _, opening = scheme.open(com, points)
        wres, wevals = whir_pcs.verify(cfg, points, opening, expected_root=com.root())
        assert wres.accepted, wres
        opened.append(wevals)
    ops, mem, rt, m = opened[0][:, 0], opened[1][:, 0], opened[0][3, 1], opened[2][0, 0]
    assert mc.check_claims(stmt, seen, ops, mem, rt, m) == "NONE"
    changed = ops.copy()
    changed[3] = K.mont([(K.unmont(changed[3])[0] + 1) % P])[0]
    assert mc.check_claims(stmt, seen, changed, mem, rt, m) == "OPS"
    # other roots: other challenges, rejected at the first layer of side OPS
    res, side, layer, _ = mc.verify(stmt, proof, K.mont([1, 2, 3]))
    assert (res.check, side, layer) == ("SUM", "OPS", 1)
    for closing in coms + [prover] + schemes:
        closing.close()
    dev.free()


def test_the_cpp_demo_commits_traces_proves_opens_checks_the_claims_and_sees_the_refusals():
    demo = os.path.join(ROOT, "examples", "memcheck_pcs_demo")
    assert os.path.exists(demo), "examples/memcheck_pcs_demo is built by __graft_entry__.build()"
    out = subprocess.run(["timeout", "-k", "10", "120", demo, "10", "6"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("ok n=10 k=6 proof_bytes=%d " % M.proof_bytes(10, 6)) and "claims=hold" in lines[0] and "load_constraint=proved" in lines[0]
    assert lines[1].startswith("one rv changed: refused rc=-6") and "the multisets differ" in lines[1]
    assert lines[2].startswith("one m changed: refused rc=-6") and "m is wrong" in lines[2]
    assert lines[3].startswith("a read from the future: refused rc=-6") and "a read is not older than its operation" in lines[3]
