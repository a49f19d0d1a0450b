"""GPU parity of the RS-encode at the shapes of WHIR's rounds, where the first NTT pass reads the caller's polynomials itself (the
de-interleave fused into its load) and, when only one to three of its rows are nonzero, is folded into the next pass's load
(ntt.hip, ntt_plan / PassParams::pre_terms).  Every shape against the CPU oracle; the smaller ones also through pk_commit's root,
whose codeword is held in the hash-ready encoding where the size allows it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOLD = 4


def round_shapes(m, n_rounds):
    """(n_vars, log_inv_rate) of the re-commits of WHIR rounds 1..n_rounds at m variables, fold 16, starting rate 1/2"""
    return [(m - FOLD * i, 1 + (FOLD - 1) * i) for i in range(1, n_rounds + 1)]


# m = 21 and 23: 4 rounds, m = 25: 5 (scheme.WhirConfig.derive); the 2^21-row re-commit of m = 25 is left to the dense tests
SHAPES = sorted({s for m, r in ((21, 4), (23, 4), (25, 5)) for s in round_shapes(m, r) if s[0] + s[1] - FOLD <= 20} | {(21, 1)})


def log_rows(n_vars, rho):
    return n_vars + rho - FOLD


def pass1_stride(lr):
    """natural-index distance between the rows of pass 1's DFT (ntt.hip ntt_plan)"""
    if lr <= 18:
        return 1 << (lr - (lr + 1) // 2)
    l1 = (lr + 2) // 3
    return 1 << (lr - l1)


def encode_and_check(ctx, oracle, batch, n_vars, rho, seed):
    from provekit_amd.field import random_field
    from provekit_amd.rs import rs_encode

    coeffs = random_field(batch << n_vars, seed).reshape(batch, 1 << n_vars, 4)
    got = rs_encode(coeffs, n_vars, rho, FOLD, ctx=ctx)
    exp = oracle.rs_encode(coeffs.reshape(-1, 4), batch, n_vars, rho, FOLD)
    assert np.array_equal(got, exp), (batch, n_vars, rho)
    return coeffs, exp


# batch 2 up to 2^18 rows (the batch axis of the larger ones is covered at the smaller shapes)
@pytest.mark.parametrize("batch,n_vars,rho", [(b, n, r) for n, r in SHAPES for b in (1, 2) if b == 1 or log_rows(n, r) <= 18])
def test_rs_encode_round_shapes(ctx, oracle, batch, n_vars, rho):
    encode_and_check(ctx, oracle, batch, n_vars, rho, 7 * n_vars + rho + batch)


# nonzero = 2^(n_vars - fold) coefficients per column against the stride of pass 1, for a two-pass (2^14, 2^16) and a three-pass (2^19)
# transform: one nonzero row of pass 1 (including a single nonzero input), two (the direct two-term sum), four and more (pass 1 kept)
@pytest.mark.parametrize("lr", [14, 16, 19])
@pytest.mark.parametrize("rows_nonzero", ["one", "half", "stride", "2stride", "4stride"])
def test_rs_encode_nonzero_around_pass1_stride(ctx, oracle, lr, rows_nonzero):
    s = pass1_stride(lr)
    L = {"one": 1, "half": s // 2, "stride": s, "2stride": 2 * s, "4stride": 4 * s}[rows_nonzero]
    n_vars = L.bit_length() - 1 + FOLD
    rho = lr - n_vars + FOLD
    assert rho >= 1 and (1 << (n_vars - FOLD)) == L
    for batch in (1, 2):
        encode_and_check(ctx, oracle, batch, n_vars, rho, 1000 + lr * 16 + n_vars + batch)


@pytest.mark.parametrize("n_vars,rho", [(5, 13), (9, 10), (9, 7), (11, 5), (13, 3), (12, 6)])
@pytest.mark.parametrize("batch", [1, 2])
def test_commit_root_round_shapes(ctx, oracle, batch, n_vars, rho):
    """pk_commit (the hash-ready codeword where the size allows it) against the oracle's Merkle root over its own encode"""
    from provekit_amd.field import random_field
    from provekit_amd.whir import commit_batch

    coeffs = random_field(batch << n_vars, 500 + n_vars * 8 + rho + batch).reshape(batch, 1 << n_vars, 4)
    exp = oracle.rs_encode(coeffs.reshape(-1, 4), batch, n_vars, rho, FOLD)
    com = commit_batch(ctx, [ctx.upload(coeffs[b]) for b in range(batch)], n_vars, rho, FOLD)
    try:
        assert np.array_equal(np.frombuffer(com.root, dtype=np.uint64), oracle.merkle_commit(exp)[1]), (batch, n_vars, rho)
    finally:
        com.close()
