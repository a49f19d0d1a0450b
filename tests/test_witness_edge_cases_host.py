"""CPU: the lists of tests/witness_edge_cases.py are what tests/test_gpu_witness_edges.py assumes.  Each one runs through the
sequential solver (oracle/witness_ref.py) and through the library's decoder and leveller (pk_witness_builders_inspect, and the lab's
pk_probe_witness_phases for the items per phase): levels, items, phase widths, how many witnesses stay None, where the oracle
panics.  The refusal of builders that read what they write (witness section) is a host matter and is tested here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import witness_ref as R  # noqa: E402
import witness_edge_cases as E  # noqa: E402


def _shape(builders):
    from tools.pk_probes import witness_phases

    from provekit_amd.witness import encode_witness_builders, inspect_witness_builders

    blob = encode_witness_builders(builders)
    info = inspect_witness_builders(blob)
    assert info["n_builders"] == len(builders) and info["consumed"] == len(blob)
    ph = witness_phases(blob)
    assert len(ph["widths"]) == 2 * info["n_levels"] and sum(ph["widths"]) == info["n_items"]
    assert [sum(row) for row in ph["ops"]] == ph["widths"]
    return info, ph


def _check_shape(case, acir=None):
    """the oracle solves the list; the levelled program has the expected shape -> (oracle witnesses, probe output)"""
    want = R.solve_witness_vec(case.builders, case.acir if acir is None else acir, [], case.nw)
    info, ph = _shape(case.builders)
    x = case.expect
    assert info["n_acir"] == len(case.acir) and info["n_witnesses"] <= case.nw
    assert info["n_levels"] == x["n_levels"]
    if "n_items" in x:
        assert info["n_items"] == x["n_items"]
    if "widths" in x:
        assert ph["widths"] == x["widths"]
    if "blocks_before" in x:
        assert ph["blocks_before"] == x["blocks_before"]
    if "blocks" in x:
        assert sum(ph["blocks_before"]) >= x["blocks"] and sum(b[0] == 12 for b in case.builders) == x["blocks"]
    if "n_none" in x:
        assert sum(v is None for v in want) == x["n_none"]
    return want, ph


def test_the_thresholds_are_the_ones_the_cases_straddle():
    from tools.pk_probes import lib, witness_thresholds

    assert witness_thresholds() == {"NARROW": 1024, "SUM_HEAVY": 128, "SUM_CHUNK": 1024}
    assert (E.NARROW, E.SUM_HEAVY, E.SUM_CHUNK) == (1024, 128, 1024) and lib.pk_probe_witness_n_ops() == len(E.OPS)


def test_the_probe_reports_the_library_reason_for_a_refused_list():
    from tools.pk_probes import witness_phases

    from provekit_amd.witness import WitnessBuilder as WB, encode_witness_builders

    with pytest.raises(ValueError, match="before it is solved"):
        witness_phases(encode_witness_builders([WB.Constant(0, 1), WB.Product(2, 0, 1)]))
    ph = witness_phases(encode_witness_builders([WB.Constant(0, 1), WB.Acir(1, 0), WB.Product(2, 0, 1)]))
    assert ph["widths"] == [2, 0, 1, 0] and ph["ops"][0][E.OP["CONST"]] == 1 and ph["ops"][0][E.OP["ACIR"]] == 1 and ph["ops"][2][E.OP["PRODUCT"]] == 1


@pytest.mark.parametrize("name", list(E.PHASE_CASES))
def test_phase_width_cases(name):
    case = E.PHASE_CASES[name]()
    _, ph = _check_shape(case)
    w = ph["widths"]
    if name.startswith("products_"):
        n = int(name.split("_")[1])
        assert w[2] == w[4] == n and (n <= E.NARROW) == (name != "products_1025")
    elif name.startswith("run_cut_by"):
        # every phase is narrow, so only the block before phase 5 ends the run that starts at phase 0; phase 5 is not empty: the
        # next run starts on an odd phase
        assert max(w) <= E.NARROW and w[5] > 0 and ph["blocks_before"][5] == 1 and w[4] > 0 and w[6] > 0
        assert sum(b[0] == (12 if name.endswith("spice") else 2) and (b[0] == 12 or len(b[2]) == E.SUM_HEAVY + 1) for b in case.builders) == 1
    elif name == "wide_histogram_narrow_counts":
        assert w[2] == E.NARROW + 1 and ph["ops"][2][E.OP["HIST_RANGE"]] == w[2] and 0 < w[3] <= E.NARROW and ph["ops"][3][E.OP["COUNT_OUT"]] == 256
    elif name == "narrow_histogram_wide_counts":
        assert 0 < w[2] <= E.NARROW and ph["ops"][2][E.OP["HIST_BINOP"]] == 10 and w[3] == 65536 > E.NARROW
    else:
        assert ph["ops"][2][E.OP["HIST_RANGE"]] == 300 and ph["ops"][2][E.OP["HIST_BINOP"]] == 10 and w[2] <= E.NARROW < w[3]


@pytest.mark.parametrize("name", list(E.HISTOGRAM_CASES))
def test_histogram_cases(name):
    case = E.HISTOGRAM_CASES[name]()
    want, ph = _check_shape(case)
    x = case.expect
    if name in E.RANGE_KINDS:
        bins, n = x["bins"], ph["widths"][2]
        assert want[x["table"] : x["table"] + 256] == bins and sum(bins) == n == ph["ops"][2][E.OP["HIST_RANGE"]]
        if name == "one_wavefront_one_value":
            assert n == E.WAVE and bins[7] == E.WAVE
        elif name == "4096_of_one_value":
            assert max(bins) == 4096 > E.NARROW
        elif name == "two_values_alternating":
            assert sorted(b for b in bins if b) == [E.WAVE, E.WAVE] and n == 2 * E.WAVE
        elif name == "tail_of_two_lanes":
            assert n % E.WAVE == 2
        elif name == "256_distinct_witnesses":
            assert bins == [1] * 256 and len(set(case.builders[-2][3])) == 256
        else:
            assert bins[7] == 3 and bins[8] == 1 and sum(v is not None and v >> 64 != 0 and v & 0xFFFFFFFFFFFFFFFF == 7 for v in want) == 2
    elif name == "three_tables_in_one_level":
        ops = ph["ops"][2]
        assert ops[E.OP["HIST_RANGE"]] == x["hist_range"] and ops[E.OP["HIST_BINOP"]] == x["hist_binop"]
        # the first table's lookups end, and the bin-op lookups begin, in the middle of a wavefront
        assert 100 % E.WAVE and x["hist_range"] % E.WAVE and (x["hist_range"] + x["hist_binop"]) % E.WAVE
        assert any(op[0] == "c" for pair in case.builders[-3][2] for op in pair)
    else:
        assert want[x["bin"]] == x["count"] and max(case.acir) == (1 << 56) + 3


@pytest.mark.parametrize("name", list(E.SPICE_CASES))
def test_spice_cases(name):
    case = E.SPICE_CASES[name]()
    want, ph = _check_shape(case)
    x = case.expect
    if name not in ("none_handling", "address_above_2_64"):  # the never-written witnesses of the value pool, at the least
        assert sum(v is None for v in want) >= 2
    # the sum one level above the last block reads outputs only: it is the last builder and every witness it reads is set
    assert case.builders[-1][0] == 2 and all(want[w] is not None for _, w in case.builders[-1][2])
    if name.startswith("ops_"):
        n = x["n_ops"]
        assert len(x["ops"]) == n
        keys = sorted((case.acir[[b for b in case.builders if b[0] == 1 and b[1] == op[1]][0][2]], k) for k, op in enumerate(x["ops"]))
        if n > 256:  # sorted position 256 opens the second workgroup of spice_resolve_kernel: its left neighbour has its address
            assert keys[255][0] == keys[256][0]
        if n == 256:
            assert keys[254][0] == keys[255][0]
    elif name == "none_handling":
        assert all(want[w] is None for w in x["none_at"])
    elif name == "address_above_2_64":
        assert want[x["ts_of_second"]] == 1 and max(case.acir[:2]) == (1 << 64) + 3
    elif name in ("one_cell", "one_address_of_many"):
        addr = {case.acir[[b for b in case.builders if b[0] == 1 and b[1] == op[1]][0][2]] for op in x["ops"]}
        assert len(addr) == 1 and len(x["ops"]) == x["n_ops"]
    elif name.startswith("two_blocks"):
        lens = [len(b[3]) for b in case.builders if b[0] == 12]
        assert lens == ([300, 7] if name.endswith("then_7") else [7, 300])


@pytest.mark.parametrize("name", list(E.DIGIT_CASES))
def test_digit_cases(name):
    case = E.DIGIT_CASES[name]()
    want, ph = _check_shape(case)
    bases, vals = E.DIGIT_BASES[name], case.expect["values"]
    total = sum(bases)
    assert ph["ops"][2][E.OP["DIGIT"]] == len(bases) * len(vals) and ph["ops"][2][E.OP["DIGIT_CHECK"]] == len(vals)
    assert {0, 1} <= set(vals) and len(vals) >= 7 and all(v < min(R.P, 1 << total) for v in vals)
    k = 0
    for lb in bases[:-1]:  # every inner slice boundary: 2^k - 1 and 2^k are among the values
        k += lb
        assert ((1 << k) - 1 in vals or (1 << k) - 1 >= R.P) and ((1 << k) in vals or (1 << k) >= R.P)
    if total >= 254:
        assert R.P - 1 in vals
    # the digits recompose to the value
    first, n = len(vals), len(vals)
    for i, v in enumerate(vals):
        acc, shift = 0, 0
        for d, lb in enumerate(bases):
            acc += want[first + d * n + i] << shift
            shift += lb
        assert acc == v


@pytest.mark.parametrize("name", list(E.SELF_DEPENDENT_CASES))
def test_builders_that_read_what_they_write_are_refused(name):
    """the sequential solver runs such a list (a later operation sees what an earlier one of the same builder wrote); the library's
    lanes would race on it, so build_program refuses it and names the builder and the witness"""
    from tools.pk_probes import witness_phases

    from provekit_amd import ProveKitHipError
    from provekit_amd.witness import encode_witness_builders, inspect_witness_builders

    case = E.SELF_DEPENDENT_CASES[name]()
    want = R.solve_witness_vec(case.builders, case.acir, [], case.nw)
    assert want[case.expect["witness"]] is not None
    blob = encode_witness_builders(case.builders)
    msg = f"builder {case.expect['builder']} reads witness {case.expect['witness']} that it also writes"
    with pytest.raises(ProveKitHipError, match=msg) as e:
        inspect_witness_builders(blob)
    assert e.value.code == -1 if hasattr(e.value, "code") else True
    with pytest.raises(ValueError, match=msg):
        witness_phases(blob)


def test_self_dependent_spice_lists_mean_something_else_in_order():
    """why the refusal matters: in each Spice list the later operation's result depends on the earlier operation's write"""
    case = E.SELF_DEPENDENT_CASES["spice_value_is_an_earlier_old_value"]()
    want = R.solve_witness_vec(case.builders, case.acir, [], case.nw)
    block = case.builders[case.expect["builder"]]
    rv = block[4]
    assert want[rv + 1] == want[case.expect["witness"]] is not None  # cell 1 ends with the old value operation 1 wrote
    case = E.SELF_DEPENDENT_CASES["digits_written_over_a_value"]()
    want = R.solve_witness_vec(case.builders, case.acir, [], case.nw)
    first = case.builders[-1][4]
    assert want[first : first + 6] == [1, 2, 2, 0, 3, 0]  # value 1 was overwritten by digit 1 of value 0 before it was decomposed


def test_single_item_and_multiplicity_builders_may_read_what_they_write():
    from provekit_amd.witness import WitnessBuilder as WB

    case = E.range_table_reads_its_own_output_range()
    want, _ = _check_shape(case)
    t = case.expect["table"]
    assert want[t : t + 4] == case.expect["counts"]
    info, _ = _shape([WB.Acir(0, 0), WB.Acir(1, 1), WB.Sum(1, [(None, 1), (5, 0)]), WB.Product(2, 1, 1)])
    assert info["n_levels"] == 3


@pytest.mark.parametrize("name", list(E.ERROR_CASES))
def test_error_cases(name):
    case = E.ERROR_CASES[name]()
    # the oracle panics exactly at the expected builder: the list up to it solves, the list including it does not
    R.solve_witness_vec(case.builders[: case.panic_builder], case.acir, [], case.nw)
    with pytest.raises(R.SolverPanic):
        R.solve_witness_vec(case.builders[: case.panic_builder + 1], case.acir, [], case.nw)
    _, ph = _check_shape(case, acir=case.acir_good)
    if name == "two_inverses":
        assert case.builders[40][0] == 7 and case.builders[60][0] == 7 and case.acir[0] == 0
        with pytest.raises(R.SolverPanic):  # builder 60 fails as well, on level 1
            R.solve_witness_vec(case.builders[:40] + case.builders[41:], case.acir, [], case.nw)
        assert ph["ops"][2][E.OP["INVERSE"]] == 1 and ph["ops"][62][E.OP["INVERSE"]] == 1
    elif name == "range_value_mid_wavefront":
        look = case.builders[case.panic_builder][3]
        pos = [i for i, w in enumerate(look) if case.acir[case.builders[w][2]] >= 256]
        assert pos == [100] and pos[0] % E.WAVE not in (0, E.WAVE - 1) and len(look) == 201
    elif name.startswith("digit_overflow"):
        total = sum(E.DIGIT_OVERFLOW_BASES[name[len("digit_overflow_"):]])
        assert case.acir[:2] == [(1 << total) - 1, 1 << total] and case.acir_good[:2] == [(1 << total) - 1] * 2 and (1 << total) < R.P
    else:
        M = case.builders[case.panic_builder][1]
        assert case.acir[:2] == [M - 1, M] and case.acir_good[:2] == [M - 1, M - 1]


def test_reuse_case():
    builders, vectors, nw, at = E.reuse_program()
    kinds = {b[0] for b in builders}
    assert {4, 14, 12} <= kinds and any(b[0] == 2 and len(b[2]) > E.SUM_HEAVY for b in builders)
    first = R.solve_witness_vec(builders, vectors[0], [], nw)
    third = R.solve_witness_vec(builders, vectors[2], [], nw)
    R.solve_witness_vec(builders[:at], vectors[1], [], nw)
    with pytest.raises(R.SolverPanic):
        R.solve_witness_vec(builders[: at + 1], vectors[1], [], nw)
    table = builders[at][1]
    assert first[table : table + 256] != third[table : table + 256] and sum(first[table : table + 256]) == sum(third[table : table + 256]) == 150
    info, ph = _shape(builders)
    assert info["n_levels"] == 5 and sum(ph["blocks_before"]) == 2  # the long sum and the Spice block


def test_the_oracle_shifts_the_binop_index_on_u64():
    """witness_builder.rs:184: `(lhs.0[0] << 8) + rhs.0[0]` on u64: lhs = 2^56 + 3 loses its top bit and counts in bin 3 * 256 + 5"""
    from provekit_amd.witness import WitnessBuilder as WB

    b = [WB.Acir(0, 0), WB.Acir(1, 1), WB.MultiplicitiesForBinOp(2, [(("w", 0), ("w", 1))])]
    w = R.solve_witness_vec(b, [(1 << 56) + 3, 5], [], 2 + 65536)
    assert w[2 + 3 * 256 + 5] == 1 and sum(w[2:]) == 1
    with pytest.raises(R.SolverPanic, match="index out of bounds"):  # 2^55 + 3 keeps a bit above the table after the shift
        R.solve_witness_vec(b, [(1 << 55) + 3, 5], [], 2 + 65536)
