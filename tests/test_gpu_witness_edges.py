"""GPU: csrc/witness.hip at the places where it changes path -- the NARROW phase width, runs of narrow phases cut by a Spice block or
a long sum, the wave-aggregated histogram (count_one), the Spice sort's workgroup seams and its None handling, the digit slices'
word boundaries, the error record, a program solved again.  The lists are tests/witness_edge_cases.py's (their shape is checked on
the host by test_witness_edge_cases_host.py); every witness and every is_set byte is compared with the sequential solver
(oracle/witness_ref.py) the way test_gpu_witness._check does."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import witness_edge_cases as E  # noqa: E402
from test_gpu_witness import _check, _mont  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def thresholds():
    """the cases straddle these values: a retune of csrc/witness_shape.hpp must fail here, not quietly un-aim them"""
    from tools.pk_probes import witness_thresholds

    assert witness_thresholds() == {"NARROW": 1024, "SUM_HEAVY": 128, "SUM_CHUNK": 1024}
    assert (E.NARROW, E.SUM_HEAVY, E.SUM_CHUNK) == (1024, 128, 1024)


def _compare(oracle, prog, builders, acir, nw):
    """_check on a program that already exists (a second solve of it): every witness and the is_set pattern against the oracle"""
    import witness_ref as R

    want = R.solve_witness_vec(builders, acir, [], nw)
    w, is_set = prog.solve_witness_vec(_mont(oracle, acir), np.zeros((0, 4), np.uint64), nw)
    assert [bool(x) for x in is_set] == [x is not None for x in want]
    got = oracle.limbs_to_ints(oracle.from_mont(w))
    for i, x in enumerate(want):
        assert got[i] == (x if x is not None else 0), f"witness {i}"
    return want


@pytest.mark.parametrize("name", list(E.PHASE_CASES))
def test_phase_widths_around_the_narrow_threshold(ctx, oracle, name):
    """1. phases of NARROW - 1, NARROW, NARROW + 1 items with a consumer per producer; narrow runs cut by a long sum / a Spice block
    and restarted on an odd phase; a wide histogram before narrow counts and the reverse; both multiplicity builders in one level"""
    case = E.PHASE_CASES[name]()
    want = _check(ctx, oracle, case.builders, case.acir, [], case.nw)
    assert sum(x is None for x in want) == case.expect["n_none"]


@pytest.mark.parametrize("name", list(E.HISTOGRAM_CASES))
def test_histograms_count_like_the_reference(ctx, oracle, name):
    """2. count_one: a full wavefront (and 4096 lookups) on one counter, two values per wavefront, a tail wavefront of two lanes, 256
    distinct witnesses, values whose high limbs are set, the wavefronts in which one table's lookups end and another's (or the
    bin-op table's) begin, and the bin-op index with lhs = 2^56 + 3 (witness_builder.rs:184: the u64 shift drops the top bit)"""
    case = E.HISTOGRAM_CASES[name]()
    want = _check(ctx, oracle, case.builders, case.acir, [], case.nw)
    if "bins" in case.expect:
        t = case.expect["table"]
        assert want[t : t + 256] == case.expect["bins"]
    if "bin" in case.expect:
        assert want[case.expect["bin"]] == case.expect["count"]


@pytest.mark.parametrize("name", list(E.SPICE_CASES))
def test_spice_blocks_at_their_edges(ctx, oracle, name):
    """3. 0, 1, 255, 256, 257 operations; one cell; one address of many; two blocks in one level (300 and 7 operations, both orders)
    and in two levels; None cells and a None left by a load; an address of 2^64 + 3.  A sum one level up reads every set output"""
    case = E.SPICE_CASES[name]()
    want = _check(ctx, oracle, case.builders, case.acir, [], case.nw)
    assert sum(x is None for x in want) == case.expect["n_none"]


@pytest.mark.parametrize("name", list(E.DIGIT_CASES))
def test_digit_slices_at_word_boundaries(ctx, oracle, name):
    """4. slices of 32 / 64 / 33 bits, starts at bits 31 / 32 / 63, an end at bit 254, a zero-width digit, 256 one-bit digits, over
    0, 1, 2^k - 1 and 2^k on every boundary, p - 1 and random values"""
    case = E.DIGIT_CASES[name]()
    _check(ctx, oracle, case.builders, case.acir, [], case.nw)


@pytest.mark.parametrize("name", list(E.SELF_DEPENDENT_CASES))
def test_builders_that_read_what_they_write_are_refused(ctx, oracle, name):
    """5. a Spice block or a decomposition that reads a witness it writes is refused when the program is created; the context then
    solves an ordinary list"""
    from provekit_amd import ProveKitHipError
    from provekit_amd.witness import WitnessProgram

    case = E.SELF_DEPENDENT_CASES[name]()
    with pytest.raises(ProveKitHipError, match=f"builder {case.expect['builder']} reads witness {case.expect['witness']} that it also writes"):
        WitnessProgram(ctx, case.builders)
    ok = E.range_table_reads_its_own_output_range()  # a multiplicity table may: it writes one phase after it reads
    want = _check(ctx, oracle, ok.builders, ok.acir, [], ok.nw)
    t = ok.expect["table"]
    assert want[t : t + 4] == ok.expect["counts"]


@pytest.mark.parametrize("name", list(E.ERROR_CASES))
def test_errors_name_the_builder_the_sequential_solver_reaches_first(ctx, oracle, name):
    """6. two failing inverses, the lower-indexed one on the deeper level; an out-of-table value in the middle of a wavefront whose
    other lanes count; 2^total against 2^total - 1 for the digits; a Spice address of memory_length against memory_length - 1.
    The same program then solves inputs that do not fail"""
    from provekit_amd import ProveKitHipError
    from provekit_amd.witness import WitnessProgram

    case = E.ERROR_CASES[name]()
    prog = WitnessProgram(ctx, case.builders)
    with pytest.raises(ProveKitHipError, match=case.panic_msg) as e:
        prog.solve_witness_vec(_mont(oracle, case.acir), np.zeros((0, 4), np.uint64), case.nw)
    assert f"witness builder {case.panic_builder}:" in str(e.value)
    _compare(oracle, prog, case.builders, case.acir_good, case.nw)
    prog.close()


def test_a_program_is_solved_again_after_other_inputs_and_after_an_error(ctx, oracle):
    """7. a range table, a bin-op table, a long sum and a Spice block: three solves of one program, the second failing; the first
    and the third equal the oracle (no count, error or partial sum carries over)"""
    from provekit_amd import ProveKitHipError
    from provekit_amd.witness import WitnessProgram

    builders, vectors, nw, at = E.reuse_program()
    prog = WitnessProgram(ctx, builders)
    first = _compare(oracle, prog, builders, vectors[0], nw)
    with pytest.raises(ProveKitHipError, match="multiplicity table") as e:
        prog.solve_witness_vec(_mont(oracle, vectors[1]), np.zeros((0, 4), np.uint64), nw)
    assert f"witness builder {at}:" in str(e.value)
    third = _compare(oracle, prog, builders, vectors[2], nw)
    assert first != third
    _compare(oracle, prog, builders, vectors[0], nw)
    prog.close()
