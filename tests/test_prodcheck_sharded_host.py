"""CPU: the host side of the sharded product sumcheck (include/provekit_sumcheck_sharded.h).  The header/library/binding symbol match
next to the lone library's untouched eleven; pkss_plan against the Python restatement of the ownership rule and the arena
(tests/prodcheck_shard_refs.py) for every size, world and shape; every plan refusal with its reason; the rule as a bijection with
the pair property; the rule and the plan under the sanitizers (a program of its own, run as a subprocess)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
HEADER = os.path.join(ROOT, "include", "provekit_sumcheck_sharded.h")
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pks_verify_asan")

import prodcheck_refs as K  # noqa: E402
import prodcheck_shard_refs as R  # noqa: E402

WORLDS = (2, 4, 8, 16)


def test_the_header_declares_what_the_library_exports_and_the_binding_binds():
    from provekit_amd import prodcheck, prodcheck_sharded

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pkss_[a-z0-9_]+)\s*\(", src)))
    nm = subprocess.run(["nm", "-D", "--defined-only", prodcheck.SUMCHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" [A-Za-z] (pkss_[a-z0-9_]+)$", nm, flags=re.M)))
    assert declared == exported == sorted(prodcheck_sharded.SIGNATURES)
    assert {"pkss_abi_version", "pkss_plan", "pkss_prover_create", "pkss_prove", "pkss_round_shard"} <= set(exported)
    assert prodcheck_sharded.lib.pkss_abi_version() == 1
    # the lone interface is what it was
    lone = sorted(set(re.findall(r" [A-Za-z] (pks_[a-z0-9_]+)$", nm, flags=re.M)))
    assert lone == sorted(prodcheck.SIGNATURES) and len(lone) == 11 and prodcheck.lib.pks_abi_version() == 1
    assert re.search(r"#define PKSS_CHUNK_LOG2 (\d+)", src).group(1) == str(R.C) == str(prodcheck_sharded.CHUNK_LOG2)
    # still nothing but the product's C ABI underneath
    und = subprocess.run(["nm", "-D", "--undefined-only", prodcheck.SUMCHECK_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not re.findall(r"\b_ZN2pk\w+", und) and not re.findall(r"\bpk[vw]_\w+", und), und
    assert set(re.findall(r"\bpk_\w+", und)) <= set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "provekit_hip.h")).read()))


def test_the_plan_is_the_rules_for_every_size_world_and_shape():
    from provekit_amd import prodcheck_sharded

    for name in K.SHAPES:
        for G in WORLDS:
            for n in range(1, 29):
                shape = K.Shape(name, n)
                p = prodcheck_sharded.plan(shape.statement(), G)
                assert (p.g, p.c, p.S, p.local_len, p.handover_len, p.arena_bytes) == R.plan(n, shape.m, G), (name, G, n)
                # S sharded rounds and no more: round i is sharded iff the bit it binds lies above the rank bits
                assert [n - 1 - i >= p.c + p.g for i in range(n)] == [i < p.S for i in range(n)]
                if p.S >= 2:  # the compacted tables are the arena's only part that grows with the tables: 1 / G of the lone prover's copies
                    rest = R.arena_elements(n, shape.m, G) - shape.m * (1 << (n - 1)) // G
                    assert rest == R.arena_elements(p.c + p.g + 1, shape.m, G) - R.eq_split_elements(p.c + p.g) + R.eq_split_elements(n - 1)
    # the issue's figure: 16 GiB of folded copies at n = 28, m = 4 on a lone prover, 1 / G of it here
    p = prodcheck_sharded.plan(K.Shape("four", 28).statement(), 16)
    assert 4 * 32 * (1 << 27) == 16 << 30 and 0 < p.arena_bytes - (16 << 30) // 16 < 4 << 20


@pytest.mark.parametrize("stmt, world, reason", [
    ((0, 2, [(1, 3)]), 2, "n must be"), ((29, 2, [(1, 3)]), 2, "n must be"),
    ((4, 0, [(1, 1)]), 2, "m must be"), ((4, 5, [(1, 3)]), 4, "m must be"),
    ((4, 2, []), 2, "T must be"), ((4, 2, [(1, 3)] * 5), 2, "T must be"),
    ((4, 2, [(1, 3)], False, 17), 2, "n_bind must be"),
    ((4, 2, [(1, 3), (1, 0)]), 2, "empty mask"),
    ((4, 2, [(1, 0b111)]), 2, "names a table >= m"),
    ((4, 3, [(1, 0b011)]), 2, "used by no term"),
    ((4, 4, [(1, 0b1111)]), 2, "more than 3 tables"),
    ((4, 2, [([2**64 - 1] * 4, 3)]), 2, "not below p"),
    ((12, 2, [(1, 3)]), 0, "at least 2"), ((12, 2, [(1, 3)]), 1, "at least 2"),
    ((12, 2, [(1, 3)]), 3, "power of two: 3 ranks"), ((12, 2, [(1, 3)]), 6, "power of two: 6 ranks"), ((12, 2, [(1, 3)]), 48, "power of two"),
    ((12, 2, [(1, 3)]), 32, "at most 16"), ((12, 2, [(1, 3)]), 2**31, "at most 16"),
])
def test_every_plan_refusal_is_made_with_a_reason(stmt, world, reason):
    from provekit_amd import prodcheck, prodcheck_sharded
    from provekit_amd._lib import ProveKitHipError

    with pytest.raises(ProveKitHipError, match=reason) as e:
        prodcheck_sharded.plan(prodcheck.Statement(*stmt), world)
    assert e.value.code == -1
    s = prodcheck.Statement(*stmt).struct()
    assert prodcheck_sharded.lib.pkss_plan(ctypes.addressof(s), world, None) == -1 and b"null pointer" in prodcheck.lib.pks_create_error()
    assert prodcheck_sharded.lib.pkss_plan(None, world, ctypes.byref(prodcheck_sharded.PlanStruct())) == -1
    assert b"null statement" in prodcheck.lib.pks_create_error()
    assert prodcheck_sharded.plan(prodcheck.Statement(12, 2, [(1, 3)]), 16).g == 4  # the largest world is taken


@pytest.mark.parametrize("G", [2, 4, 8])
def test_the_rule_is_a_bijection_and_compaction_keeps_pairs(G):
    g = R.log2(G)
    for n in range(R.C + g, R.C + g + 4):
        N = 1 << n
        seen = []
        for r in range(G):
            mine = R.owned(n, g, r)
            assert [R.compact(x, g) for x in mine] == list(range(N // G))  # 0 .. 2^n / G - 1, in order
            assert [R.expand(y, g, r) for y in range(N // G)] == mine
            seen += mine
        assert sorted(seen) == list(range(N))
        # the pair property at every round length down to 2^(c+g+1): the partner of an owned index is owned and compacts to the partner
        lengths = [N >> i for i in range(R.sharded_rounds(n, g))]
        assert lengths == [L for L in (N >> i for i in range(n)) if L >= 1 << (R.C + g + 1)]
        for L in lengths:
            for x in range(L // 2):
                assert R.owner(x + L // 2, g) == R.owner(x, g) and R.compact(x + L // 2, g) == R.compact(x, g) + (L // G) // 2
        # one length further the pair is split between two ranks: the round is not sharded
        L = 1 << (R.C + g)
        if L <= N:
            assert R.owner(L // 2, g) != R.owner(0, g)


def test_the_rule_and_the_plan_under_the_sanitizers():
    """shard.hpp's functions -- the ones the kernel is compiled from -- and pkss_plan, built with -fsanitize=address,undefined as a
    program of its own (make -C provekit_amd/csrc asan): the rule marks every slot of an exact-size heap block once, and the plan's
    lines are the reference's"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    for n, G in ((1, 2), (8, 2), (9, 2), (10, 2), (13, 2), (10, 4), (14, 4), (11, 8), (15, 8), (17, 16), (20, 16), (28, 16)):
        p = subprocess.run([ASAN, "shard", str(n), str(G)], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, (n, G, p.stdout, p.stderr[-3000:])
        want = [" ".join(str(v) for v in (n, m) + R.plan(n, m, G)) for m in (1, 2, 3, 4)]
        assert p.stdout.splitlines() == want, (n, G)
    for n, G, reason in ((0, 2, "n must be"), (29, 4, "n must be"), (12, 3, "power of two"), (12, 1, "at least 2"), (12, 32, "at most 16")):
        p = subprocess.run([ASAN, "shard", str(n), str(G)], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0 and p.stdout.startswith("-1 REFUSED") and reason in p.stdout, (n, G, p.stdout, p.stderr[-2000:])


def test_the_lone_prover_is_a_device_set_of_one_whose_arena_is_the_lone_rule():
    """The layout at g = 0 -- what pks_prover_create allocates, and what pkl_/pkg_prover_arena_bytes add up -- against round.hpp's rule,
    restated here: m folded copies of half length, one round's scratch (4 x 1024 partials and 8 results) and the split eq weights of
    R = n - 1 coordinates, 2^(H+1) + 2^(L+1) - 2 elements with L = R // 2 trailing and H = R - L leading ones.  The sanitizer build
    prints it as the shard mode's last column"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pks_verify_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    for n in (1, 2, 9, 28):
        p = subprocess.run([ASAN, "shard", str(n), "2", "lone"], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, (n, p.stdout, p.stderr[-3000:])
        lines = [line.split() for line in p.stdout.splitlines()]
        assert [line[:2] for line in lines] == [[str(n), str(m)] for m in (1, 2, 3, 4)]
        R_, L = n - 1, (n - 1) // 2
        H = R_ - L
        for m, line in zip((1, 2, 3, 4), lines):
            lone_arena_fes = m * (1 << (n - 1)) + (4 * 1024 + 8) + (2 << H) + (2 << L) - 2
            assert int(line[-1]) == 32 * lone_arena_fes, (n, m)
            assert line[:-1] == [str(v) for v in (n, m) + R.plan(n, m, 2)]  # the other columns are the plan's, as without `lone`
