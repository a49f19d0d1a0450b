"""CPU: the reference's OWN proof (tooling/provekit-bench/benches/poseidon-1000.np, 268,756 transcript bytes) walked by the
restated verifier in its read order -- root, OOD answers, blinding commitment, 20 x 4 sumcheck coefficients, sums, the
blinding WHIR proof, `claimed_evaluations`, the 4-round witness WHIR proof with every `stir_answers` / `merkle_proof` hint,
PoW nonces, final coefficients, `deferred_weight_evaluations` -- with the scheme shape this library uses for that size class.
The walk must consume the transcript exactly, every hint must have the shape the verifier expects, and all 218 Merkle
openings must reach their roots (Skyscraper v1: the fixture predates v2).  Challenge-dependent relations are skipped: the
reference's domain-separator labels live in un-vendored crates, so its Fiat-Shamir challenges cannot be reproduced here.
Since pk_prove's proofs are accepted by the same verifier in full mode, this pins the prover's wire layout to the reference's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "poseidon-1000.np")  # the reference's own proof, kept as a golden fixture


def test_reference_proof_walks_in_our_read_order():
    import verifier as V
    from provekit_amd.file import read_np
    from provekit_amd.scheme import WhirConfig, blinding_config_for

    t = read_np(FIXTURE)
    assert len(t) == 268756
    m, m_0 = 21, 20

    def vcfg(c):
        return V.WhirConfig(c.n_vars, c.batch_size, c.folding_factor, c.starting_log_inv_rate, c.num_queries, c.ood_samples, c.pow_bits,
                            c.final_queries, c.final_pow_bits, c.commitment_ood_samples, c.final_folding_pow_bits)

    cfg_w, cfg_b = vcfg(WhirConfig.for_size(m)), vcfg(blinding_config_for(m_0))
    assert cfg_b.n_vars == 8 and len(cfg_b.num_queries) == 1  # next_power_of_two(4 * 20) + 1 variables, one round + final
    assert V.verify(t, b"", m, m_0, cfg_w, cfg_b, structure_only=True, hash_version=1)
    # ... and it performs exactly the operations this library's IO pattern declares for the scheme (absorb / squeeze / hint counts
    # in order, spongefish's own check; the labels -- hence the IV and the challenges -- are what stays unpinned)
    from provekit_amd.scheme import create_io_pattern

    pattern = create_io_pattern(m_0, WhirConfig.for_size(m), blinding_config_for(m_0))
    assert V.verify(t, pattern, m, m_0, cfg_w, cfg_b, structure_only=True, hash_version=1)
    with pytest.raises(V.VerifyError, match="IO pattern"):
        V.verify(t, pattern.replace(b"\0Hclaimed_evaluations", b"", 1), m, m_0, cfg_w, cfg_b, structure_only=True, hash_version=1)
    # the walk is sensitive to the shape: a different round count, m_0 or OOD count must not parse
    import copy

    for tweak in ("m_0", "rounds", "ood", "nopow"):
        cw, cb, mm0 = copy.deepcopy(cfg_w), copy.deepcopy(cfg_b), m_0
        if tweak == "m_0":
            mm0 = 19
        elif tweak == "rounds":
            cw.num_queries, cw.ood_samples, cw.pow_bits = cw.num_queries[:3], cw.ood_samples[:3], cw.pow_bits[:3]
        elif tweak == "ood":
            cw.ood_samples = [2] * 4
        else:
            cw.pow_bits = [0.0] * 4
        with pytest.raises(Exception):
            V.verify(t, b"", m, mm0, cw, cb, structure_only=True, hash_version=1)
    # ... and with the v2 hash no opening verifies
    with pytest.raises(V.VerifyError):
        V.verify(t, b"", m, m_0, cfg_w, cfg_b, structure_only=True, hash_version=2)
