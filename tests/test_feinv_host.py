"""CPU: the safegcd inverse (csrc/feinv.hpp) piecewise on the host build -- divsteps30, divsteps30_var, update_de, update_fg, normalize and the
two conversions through pk_selftest_inv30, on the records of tests/feinv_refs.py and against the definition stated there; the whole inverse
(ops 21, 22, 23 of pk_selftest_arith) on operands whose walks leave the middle of the road; and the same parts under AddressSanitizer +
UBSan as a program of its own (make -C provekit_amd/csrc asan).  First of all the operand sets are held to what they must reach, on the
reference alone: a set that quietly stops reaching an edge fails here, before anything of the library is compared.
tests/test_gpu_feinv.py is the device half."""
import os
import subprocess

import numpy as np
import pytest

import feinv_refs as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pk_feinv_asan")
P = fr.P


def host_part(part, rin):
    from provekit_amd._lib import lib

    rin = np.ascontiguousarray(rin, dtype=np.int32)
    out = np.full_like(rin, -1)
    assert lib.pk_selftest_inv30(part, rin.ctypes.data, out.ctypes.data, rin.shape[0]) == 0
    return out


def host_arith(op, xs):
    from provekit_amd._lib import lib

    a = fr.to_limbs(xs)
    out = np.empty_like(a)
    assert lib.pk_selftest_arith(op, a.ctypes.data, a.ctypes.data, out.ctypes.data, a.shape[0]) == 0
    return fr.from_limbs(out)


# ---- what the operand sets reach, on the reference alone -------------------------------------------------------------------------------
def test_the_definition_and_the_batched_bookkeeping_agree_on_every_step_record():
    """var_trace (the transliteration that reports limits, zero runs and swaps) returns the definition's matrix and eta on every record"""
    for op, (t, eta) in zip(fr.step_operands(), fr.step_results(1)):
        got = fr.var_trace(*op)
        assert (got[0], got[1]) == (t, eta), op
        assert all(abs(x) <= fr.B30 for x in t) and abs(t[0]) + abs(t[1]) <= fr.B30 and abs(t[2]) + abs(t[3]) <= fr.B30
    for t, _ in fr.step_results(0):
        assert abs(t[0]) + abs(t[1]) <= fr.B30 and abs(t[2]) + abs(t[3]) <= fr.B30


def test_the_step_records_reach_every_limit_run_and_swap_position():
    ops = fr.step_operands()
    assert 3000 <= len(ops) <= 6000 and all(f0 & 1 for _, f0, _ in ops)
    assert {eta for eta, _, _ in ops} >= set(range(-40, 41)) | {-300, 300, -750, 750}
    limits, runs, later, swaps, signs = set(), set(), set(), set(), set()
    for op in ops:
        _, eta, lim, run, swap = fr.var_trace(*op)
        limits.update(lim)
        runs.add(run[0])
        later.update(run[1:])
        swaps.update(swap)
        signs.add(eta < 0)
    assert limits == {1, 2, 3, 4, 5, 6}
    assert 30 in runs  # a zero run of all 30 steps: g0 = 0 mod 2^30
    assert 30 in later and runs | later >= set(range(31))  # ... and the one that follows g + w f = 0 before anything was shifted
    assert 0 in swaps and max(swaps) >= 28 and swaps >= {28, 29}  # a swap at the first step and at each of the last two
    assert signs == {False, True}  # eta' of both signs
    ms = [t for t, _ in fr.matrices()]
    assert (fr.B30, 0, 0, 1) in ms  # 30 zeros: f stays, g is divided by 2^30
    assert sum(1 for t in ms if abs(t[0]) + abs(t[1]) == fr.B30) >= 100 and sum(1 for t in ms if abs(t[2]) + abs(t[3]) == fr.B30) >= 1


def test_the_update_de_records_reach_both_ends_of_the_outputs_and_of_md():
    """the lowest md a batch's matrix allows is -2^29 - (2^30 - 1) = -1.5 * 2^30 + 1: no row of an n-step matrix has negative entries
    that sum below -2^(n-1) (checked exhaustively for n <= 8), and the multiple of p taken off is at most 2^30 - 1.  The set holds
    that floor exactly."""
    ops, res = fr.de_operands(), fr.de_results()
    assert len(ops) <= 30000
    ms = {t for t, _ in fr.matrices()}
    assert {t for _, _, t in ops} >= ms  # every matrix parts 0 and 1 produced
    edges = set(fr.DE_EDGES)
    assert {(d, e) for d, e, _ in ops if d in edges and e in edges} == {(d, e) for d in edges for e in edges}
    outs = [x for d, e, _, _ in res for x in (d, e)]
    mds = [x for _, _, md, me in res for x in (md, me)]
    assert all(-2 * P < x < P for x in outs)  # the invariant: nothing outside (-2p, p)
    assert min(outs) * 100 < -199 * P and min(outs) * 10**9 < -1999999999 * P  # below -1.99 p (and below -1.999999999 p)
    assert max(outs) * 100 > 99 * P and max(outs) == P - 1
    assert min(mds) == -3 * (1 << 29) + 1  # the floor
    assert max(mds) == 1 << 30
    assert min(x for _, _, t in ops for x in (min(t[0], 0) + min(t[1], 0), min(t[2], 0) + min(t[3], 0))) == -(1 << 29)


def test_the_other_part_records_meet_their_preconditions():
    assert all(abs(f) < 1 << 255 and abs(g) < 1 << 255 and (f - f0) % fr.B30 == 0 and (g - g0) % fr.B30 == 0
               for (f, g, t), (f0, g0) in zip(fr.fg_operands()[::2], (fg for _, fg in fr.matrices())))
    assert {t for _, _, t in fr.fg_operands()} == {t for t, _ in fr.matrices()}
    rs = {r for r, _ in fr.normalize_operands()}
    outs = [x for d, e, _, _ in fr.de_results() for x in (d, e)]
    assert all(-2 * P < r < P for r in rs) and rs >= set(fr.DE_EDGES) | {0, min(outs), max(outs)}
    assert {s for _, s in fr.normalize_operands()} >= {0, -1}
    assert all(0 <= v < fr.R for v in fr.conversion_values())
    for part in fr.PARTS:  # a record is what the part reads: the conversions are a round trip by construction
        rin, want = fr.records(part)
        assert rin.shape == want.shape and rin.shape[1] == 32 and rin.shape[0] >= 400
    assert np.array_equal(fr.records(5)[1], fr.records(6)[0]) and np.array_equal(fr.records(6)[1], fr.records(5)[0])


def test_the_whole_inversions_leave_the_middle_of_the_road():
    vals, ws = fr.inversion_values(), fr.inversion_walks()
    s = fr.summarize(ws)
    assert len([b for b in s["batches"] if b]) >= 3 and s["batches"][0] == 0  # three batch counts besides the lane that takes none
    assert s["eta"][0] <= -200 and s["eta"][1] >= 200
    assert s["zero_batches_after_first"] >= 100
    assert all(w["result"] == fr.inverse(x) for w, x in zip(ws, vals))
    order = fr.interleaved_order()
    assert set(order) == set(vals) and len(order) > 64
    batches = dict(zip(vals, (w["batches"] for w in ws)))
    most = max(batches.values())
    fewest = min(b for b in batches.values() if b)
    assert batches[0] == 0 and batches[1] >= fewest  # only x = 0 leaves at once: x = 1 still has p to bring down
    for w in range(0, len(order) - 63, 64):  # every full wavefront: x = 0 and x = 1 next to the longest, then most and fewest alternating
        wave = order[w: w + 64]
        assert wave[0] == 0 and wave[2] == 1 and batches[wave[1]] == most and batches[wave[3]] == most
        assert batches[wave[5]] == fewest and batches[wave[4]] > fewest
    srt = fr.sorted_order()
    assert sorted(srt) == sorted(vals) and [batches[x] for x in srt] == sorted(batches.values())


# ---- the host build against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", sorted(fr.PARTS))
def test_every_part_of_the_host_build_equals_the_definition(part):
    rin, want = fr.records(part)
    got = host_part(part, rin)
    assert fr.differing(got, want, rin) == [], f"{fr.PARTS[part]}: the host build differs from the definition"
    if part in (2, 3, 4):  # stated on its own: limbs 0..7 of every result are canonical
        low = np.delete(got[:, :18], [8, 17], axis=1)
        assert low.min() >= 0 and low.max() < fr.B30


@pytest.mark.parametrize("op", [21, 22, 23])
def test_the_whole_inverse_on_the_edge_operands(op):
    """22, 23: plain integers, both step forms; 21: Montgomery in and out around the variable-time form, fed the values themselves so
    that the walk inside is the listed one: (x)^-1 R^2"""
    vals = fr.inversion_values()
    want = [fr.inverse(x) * (fr.R * fr.R if op == 21 else 1) % P for x in vals]
    got = host_arith(op, vals)
    assert [(hex(x), hex(g), hex(w)) for x, g, w in zip(vals, got, want) if g != w][:4] == []


def test_an_unknown_part_is_refused():
    from provekit_amd._lib import lib

    rin = np.zeros((2, 32), dtype=np.int32)
    rin[:, 1] = 1
    out = np.zeros_like(rin)
    for part in (-1, 7, 44, 1 << 20):
        assert lib.pk_selftest_inv30(part, rin.ctypes.data, out.ctypes.data, 2) != 0
    assert lib.pk_selftest_inv30(0, None, out.ctypes.data, 2) != 0 and lib.pk_selftest_inv30(0, rin.ctypes.data, None, 2) != 0
    assert lib.pk_selftest_inv30(0, rin.ctypes.data, out.ctypes.data, 0) == 0


# ---- the same parts under the sanitizers ---------------------------------------------------------------------------------------------
def test_parts_0_to_4_under_the_sanitizers_equal_the_definition(tmp_path):
    """signed overflow in md, me, the 64-bit columns and the top limbs at the ends of the ranges would be a UBSan report (exit != 0)"""
    assert os.path.exists(ASAN), "provekit_amd/lib/pk_feinv_asan is missing: make -C provekit_amd/csrc asan"
    parts = [0, 1, 2, 3, 4]
    fin, fout = tmp_path / "records.bin", tmp_path / "results.bin"
    with open(fin, "wb") as f:
        for part in parts:
            rin = fr.records(part)[0]
            f.write(np.array([part, rin.shape[0]], dtype="<i4").tobytes() + rin.astype("<i4").tobytes())
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    p = subprocess.run([ASAN, str(fin), str(fout)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    n = sum(fr.records(part)[0].shape[0] for part in parts)
    assert p.stdout.splitlines() == [f"feinv parts ok: {len(parts)} groups, {n} records"]
    got = np.fromfile(fout, dtype="<i4").reshape(-1, 32)
    assert got.shape[0] == n
    at = 0
    for part in parts:
        rin, want = fr.records(part)
        assert fr.differing(got[at: at + rin.shape[0]], want, rin) == [], fr.PARTS[part]
        at += rin.shape[0]
    # an unknown part and a truncated file are refused
    bad = tmp_path / "bad.bin"
    bad.write_bytes(np.array([9, 1] + [0] * 32, dtype="<i4").tobytes())
    assert subprocess.run([ASAN, str(bad), str(fout)], capture_output=True, env=env, timeout=60).returncode == 1
    bad.write_bytes(np.array([0, 2] + [1] * 32, dtype="<i4").tobytes())
    assert subprocess.run([ASAN, str(bad), str(fout)], capture_output=True, env=env, timeout=60).returncode == 1
