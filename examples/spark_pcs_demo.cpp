// spark_pcs_demo.cpp -- a sparse-matrix evaluation proof over committed columns, end to end, no Python in the loop.  Build a small
// R1CS (three CSR matrices over one interner, column 0 -- the constant-one witness -- in every row of A); flatten it into ONE stacked
// entry list (provekit::Spark::entries_from_r1cs, include/provekit_spark.hpp); build the matrix's columns on the device and commit them
// ONCE with WHIR (provekit::WhirPcs): {row, col, val} as one batch, m_row and m_col.  Then a query: a point ((u, rx), ry), the
// per-query columns {e_row, e_col} gathered (Spark::begin) and committed, all four roots bound, the proof (Spark::prove), the host
// verifier with the value expected (Spark::verify), the nine evaluations opened at the five points -- {row, col, val} and {e_row, e_col}
// at z_V, z_R and z_C with one opening each -- and the claims checked on the values the openings bind (Spark::check_claims).  Then the
// two refusals: a wrong v, a tampered e_row.
//
//   spark_pcs_demo [s = 5] [t = 6] [seed = 7]        2^s constraints' room, 2^t witnesses' room; the query's statement is (s + 4, s + 2, t)
#include <cstdio>
#include <cstdlib>

#include "provekit_spark.hpp"
#include "provekit_whir.hpp"

using namespace provekit;

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// canonical values -> a device vector of their Montgomery images, by the library's own conversion
static DeviceVec montgomery(const Context& ctx, const std::vector<FieldElement>& canonical) {
    DeviceVec d(ctx, canonical);
    ctx.check(pk_fe_to_mont(ctx.get(), d.data(), d.data(), canonical.size()));
    return d;
}
// a root, a canonical digest, as the field element a transcript absorbs
static FieldElement as_element(const Context& ctx, const std::array<uint8_t, 32>& root) {
    FieldElement c;
    std::memcpy(c.data(), root.data(), 32);
    return montgomery(ctx, {c}).to_host()[0];
}

struct Csr {
    std::vector<uint32_t> starts, cols, values;
};

int main(int argc, char** argv) {
    const unsigned s = argc > 1 ? std::atoi(argv[1]) : 5, t = argc > 2 ? std::atoi(argv[2]) : 6;
    uint64_t rng = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 7;
    try {
        if (s < 2 || s > 20 || t < 3 || t > 24) throw Error(PK_ERR_BAD_ARG, "s is 2 .. 20, t is 3 .. 24");
        Context ctx(0);
        const unsigned n = s + 4, rows_bits = s + 2;  // at most 3 entries in each of 3 2^s rows: below 2^(s+4)
        const size_t nc = ((size_t)1 << s) - 1, nw = ((size_t)1 << t) - 3, N = (size_t)1 << n;
        // the R1CS: an interner of 8 distinct values (1 and 0 among them) and three matrices of 1 .. 3 entries a row
        std::vector<FieldElement> canonical(8);
        for (size_t i = 0; i < canonical.size(); i++) canonical[i] = {i == 0 ? 1 : i == 1 ? 0 : splitmix(rng) >> 1, 0, 0, 0};
        const std::vector<FieldElement> interner = montgomery(ctx, canonical).to_host();
        Csr m[3];
        for (int g = 0; g < 3; g++)
            for (size_t r = 0; r < nc; r++) {
                m[g].starts.push_back((uint32_t)m[g].cols.size());
                uint32_t c = g == 0 ? 0 : (uint32_t)(splitmix(rng) % nw);  // A reads the constant-one witness in every row
                const unsigned count = 1 + (unsigned)(splitmix(rng) % 3);
                for (unsigned e = 0; e < count && c < nw; e++, c += 1 + (uint32_t)(splitmix(rng) % 5))
                    m[g].cols.push_back(c), m[g].values.push_back((uint32_t)(splitmix(rng) % interner.size()));
            }
        pk_sparse_matrix mats[3];
        for (int g = 0; g < 3; g++) mats[g] = pk_sparse_matrix{m[g].starts.data(), m[g].cols.data(), m[g].values.data(), m[g].cols.size()};
        const SparkEntries entries = Spark::entries_from_r1cs(nc, nw, mats, interner, n, s, t);

        // the matrix, once: its columns on the device, committed before any query exists
        Spark prover(ctx, n, rows_bits, t, 4);
        const DeviceVec d_row_idx = Spark::indices(ctx, entries.row_idx), d_col_idx = Spark::indices(ctx, entries.col_idx), d_val(ctx, entries.val);
        DeviceVec d_row(ctx, N), d_col(ctx, N), d_m_row(ctx, (size_t)1 << rows_bits), d_m_col(ctx, (size_t)1 << t);
        prover.matrix(d_row_idx, d_col_idx, d_row, d_col, d_m_row, d_m_col);
        const WhirConfig cfg_mat = WhirConfig::for_size(n, 8.0, 3), cfg_mr = WhirConfig::for_size(rows_bits, 8.0, 1), cfg_mc = WhirConfig::for_size(t, 8.0, 1),
                         cfg_e = WhirConfig::for_size(n, 8.0, 2);
        WhirPcs pcs_mat(ctx, cfg_mat), pcs_mr(ctx, cfg_mr), pcs_mc(ctx, cfg_mc), pcs_e(ctx, cfg_e);
        const PcsCommitment com_mat = pcs_mat.commit({&d_row, &d_col, &d_val}), com_mr = pcs_mr.commit({&d_m_row}), com_mc = pcs_mc.commit({&d_m_col});

        // a query: in a verifier of pk_prove's proofs u is drawn after the three deferred values are fixed, rx and ry are alpha and the
        // point of the proof.  Here: any point
        auto point = [&](unsigned count) {
            std::vector<FieldElement> p(count);
            for (FieldElement& x : p) x = {splitmix(rng), splitmix(rng), splitmix(rng), splitmix(rng) >> 4};
            return p;
        };
        const std::vector<FieldElement> rx = point(rows_bits), ry = point(t);
        DeviceVec d_e_row(ctx, N), d_e_col(ctx, N);
        prover.begin(d_row_idx, d_col_idx, rx, ry, d_e_row, d_e_col);
        const PcsCommitment com_e = pcs_e.commit({&d_e_row, &d_e_col});  // bound before any challenge is drawn
        const std::vector<FieldElement> bind{as_element(ctx, com_mat.root()), as_element(ctx, com_mr.root()), as_element(ctx, com_mc.root()), as_element(ctx, com_e.root())};
        const SparkColumns cols{&d_row, &d_col, &d_val, &d_m_row, &d_m_col, &d_e_row, &d_e_col};
        const SparkProof proof = prover.prove(cols, rx, ry, bind);

        const SparkVerdict ok = Spark::verify(prover.statement(), proof.proof, rx, ry, bind, &proof.value);
        if (!ok) throw Error(-200, "a valid Spark proof was rejected: " + ok.message);
        const SparkClaims& cl = ok.claims;
        if (cl.value != proof.value || cl.z_val != proof.claims.z_val || cl.z_row != proof.claims.z_row || cl.z_col != proof.claims.z_col || cl.y_row != proof.claims.y_row ||
            cl.y_col != proof.claims.y_col)
            throw Error(-201, "the verifier derived other claims than the prover returned");

        // accepted PROVIDED the nine evaluations hold: the commitment scheme gives them, with one opening per commitment
        size_t opening_bytes = 0;
        auto opened = [&](const WhirPcs& pcs, const WhirConfig& cfg, const PcsCommitment& com, const std::vector<Point>& points, const char* what) {
            const PcsOpening opening = pcs.open(com, points);
            const std::array<uint8_t, 32> root = com.root();
            std::vector<FieldElement> bound;  // [polynomial][point]
            const PcsVerdict v = WhirPcs::verify(cfg, points, opening.proof, &root, &bound);
            if (!v) throw Error(-202, std::string("a valid opening of ") + what + " was rejected: " + v.message);
            opening_bytes += opening.proof.size();
            return bound;
        };
        const std::vector<Point> three{cl.z_val, cl.z_row, cl.z_col};
        const std::vector<FieldElement> mat = opened(pcs_mat, cfg_mat, com_mat, three, "the matrix's columns"), e = opened(pcs_e, cfg_e, com_e, three, "the query's columns"),
                                        mr = opened(pcs_mr, cfg_mr, com_mr, {cl.y_row}, "m_row"), mc = opened(pcs_mc, cfg_mc, com_mc, {cl.y_col}, "m_col");
        // mat[3 polynomial + point]: row at z_R, col at z_C, val at z_V; e[3 polynomial + point]: e_row at z_V and z_R, e_col at z_V and z_C
        const std::vector<FieldElement> val_evals{mat[6], e[0], e[3]}, row_evals{mat[1], e[1]}, col_evals{mat[5], e[5]};
        const int which = Spark::check_claims(prover.statement(), cl, val_evals, row_evals, mr[0], col_evals, mc[0]);
        if (which != PKX_CLAIM_NONE) throw Error(-203, "the committed columns do not take the claimed values: claim " + std::to_string(which));
        std::vector<FieldElement> other = row_evals;
        other[1][0] ^= 1;  // one evaluation changed: its claim fails
        if (Spark::check_claims(prover.statement(), cl, val_evals, other, mr[0], col_evals, mc[0]) != PKX_CLAIM_ROW) throw Error(-204, "a changed evaluation passed the claims");
        std::printf("ok n=%u s=%u t=%u nnz=%zu proof_bytes=%zu opening_bytes=%zu commitments=4 openings=4 claims=hold\n", n, rows_bits, t,
                    m[0].cols.size() + m[1].cols.size() + m[2].cols.size(), proof.proof.size(), opening_bytes);

        // a wrong v: the verifier that expects another value rejects the honest proof at the sumcheck's first element
        FieldElement wrong = proof.value;
        wrong[0] ^= 1;
        const SparkVerdict no = Spark::verify(prover.statement(), proof.proof, rx, ry, bind, &wrong);
        if (no || no.check != PKS_CHECK_SUM || no.side != PKX_SIDE_VAL) throw Error(-205, "a wrong value was accepted");
        std::printf("a wrong v: rejected check=%s side=%d offset=%llu (%s)\n", no.check_name(), no.side, (unsigned long long)no.offset, no.message.c_str());

        // a tampered e_row: the prover refuses, naming the side and the entry; after it the same prover proves the good columns again
        {
            std::vector<FieldElement> tampered = d_e_row.to_host();
            tampered[N / 3][0] ^= 1;
            const DeviceVec d_bad(ctx, tampered);
            SparkColumns bad = cols;
            bad.e_row = &d_bad;
            try {
                prover.prove(bad, rx, ry, bind);
                throw Error(-206, "a tampered e_row was taken");
            } catch (const Error& err) {
                if (err.code != PK_ERR_UNSATISFIED) throw;
                std::printf("one e_row changed: refused rc=%d (%s)\n", err.code, err.what());
            }
            if (prover.prove(cols, rx, ry, bind).proof != proof.proof) throw Error(-207, "the prover did not stay usable");
        }
        return 0;
    } catch (const Error& e) {
        std::fprintf(stderr, "provekit::Error %d: %s\n", e.code, e.what());
        return 1;
    }
}
