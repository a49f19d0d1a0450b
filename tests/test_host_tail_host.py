"""CPU: the prover's host tail (csrc/host_tail.hpp) under AddressSanitizer + UBSan, as a program of its own (make -C provekit_amd/csrc asan):
every function against a naive restatement -- direct sums over the pairs, eq by its product formula, the other host multiplier -- at lengths
1, 2, 3, 4, 256 and 2^11, entries and challenges drawn from 0, 1, p - 1 and random values, 0, 1 and 110 points for the weights; every table
in a heap block of exactly its size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pk_host_tail_asan")


def test_every_host_function_equals_its_naive_restatement_under_the_sanitizers():
    assert os.path.exists(ASAN), "provekit_amd/lib/pk_host_tail_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    p = subprocess.run([ASAN], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert p.stdout.splitlines() == ["accumulator ok", "quadratic rounds ok", "cubic rounds ok", "equality weights ok", "dot products ok", "host tail ok"]
