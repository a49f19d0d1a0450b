"""CPU: the host restatement of a short WHIR commitment and opening (csrc/host_whir.hpp: the blinding polynomial's, on the prover's thread)
under AddressSanitizer + UBSan, as a program of its own (make -C provekit_amd/csrc asan).  Every function against a naive restatement: the
codeword as direct Horner evaluations at the domain points the device layout prescribes, the tree by plain recursion, every opening walked
back to the root, the grinder against a linear scan that also confirms no smaller nonce is valid.  n = 4, 5, 6, 8
variables at fold 4 and rate 1/2 (2, 4, 8, 32 leaves), batch 1 and 2, the round shape (n = 4, rate 1/16),
entries from 0, 1, p - 1 and random, grinding at 0, 1, 4, 6 and 8 bits, index lists with repeats and with every leaf opened; every table in
a heap block of exactly its size."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN = os.path.join(ROOT, "provekit_amd", "lib", "pk_host_whir_asan")


def test_every_host_function_equals_its_naive_restatement_under_the_sanitizers():
    assert os.path.exists(ASAN), "provekit_amd/lib/pk_host_whir_asan is missing: make -C provekit_amd/csrc asan"
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    p = subprocess.run([ASAN], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert p.stdout.splitlines() == ["commitments and openings ok", "folds and evaluations ok", "grinder ok", "host whir ok"]
