// sparse.hpp -- SPARSE weights of a linear statement (include/provekit_whir_sparse.h): the host's view of the index/value lists
// and its rules, the chunked eq tables both sides evaluate a sparse weight with, and the launches of sparse.hip for pcs.cpp
// (pkw_open_sparse runs them on the scheme's stream with arena scratch) and for tools/probes.  The inline part is host code with
// no HIP call: the sanitizer build of the host verifier takes it alone.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../transcript.hpp"
#include "linear.hpp"
#include "linear_tile.hpp"

namespace pkw {

// l weights CSR-style: weight i owns entries offsets[i] .. offsets[i + 1] of index / value.  offsets is a HOST array of l + 1;
// index / value are device arrays for the prover's entry points and host arrays for the verifier's
struct SparseWeights {
    const uint64_t* offsets = nullptr;
    const uint32_t* index = nullptr;
    const uint64_t* value = nullptr;
    unsigned l = 0;
    size_t begin(unsigned i) const { return (size_t)offsets[i]; }
    size_t nnz(unsigned i) const { return (size_t)(offsets[i + 1] - offsets[i]); }
    size_t total() const { return l ? (size_t)offsets[l] : 0; }
};

// SPARSE_CHUNK_BITS, SPARSE_EVAL_STEPS and SPARSE_TILE_B are choices nobody has measured yet (EXPERIMENTS round 15)
constexpr unsigned SPARSE_CHUNK_BITS = 8;  // eq(index, point) = one factor per chunk of 8 index bits: at most 4 tables of 2^8 entries
constexpr unsigned SPARSE_MAX_CHUNKS = 4;  // n_vars <= 30
constexpr unsigned SPARSE_THREADS = 256;   // lanes of a workgroup = entries it takes per step, in all of sparse.hip's kernels
constexpr unsigned SPARSE_PASS = 8;        // weights per launch of the sums and the evaluation: their partials lie in rows of it
constexpr unsigned SPARSE_EVAL_STEPS = 8;  // steps a workgroup of the evaluation takes before the grid grows: its prologue builds the tables
constexpr unsigned SPARSE_MAX_BATCH = WSUM_MAX_BATCH;
constexpr unsigned SPARSE_TILE_B = 2;      // polynomials per lane of the sums kernel; more take further slices of the grid

// the lane's accumulators of the sums kernel: one entry's value against its position in B polynomials, dot29's grouping
// (linear_tile.hpp: one Montgomery reduction per DOT29_GROUP products, the column bound documented there)
template <int B>
using SparseTile = WsumTile<B, 1>;
// one entry: the gathered elements f (any 256-bit values) against the entry's value (< p).  The elements are reduced below p first:
// dot29's RUNNING sum is sized for first factors below p (a group of four then adds < 1.76 p to it); eight entries in a row of
// 2^256 - 1 against p - 1 carry it past what reduce_almost29 takes (tests/test_whir_pcs_sparse_host.py runs exactly that), and a
// gather cannot rule such a run out.  Three conditional subtractions per element, against 81 multiply-adds per product
template <int B>
PK_HD void sparse_tile_step(SparseTile<B>& t, const pk::fe (&f)[B], const pk::fe& value) {
    pk::fe g[B], w[1] = {value};
#pragma unroll
    for (int u = 0; u < B; u++) g[u] = pk::fe_reduce_any(f[u]);
    wsum_tile_step(t, g, w);
}

inline unsigned sparse_chunks(unsigned n_vars) { return (n_vars + SPARSE_CHUNK_BITS - 1) / SPARSE_CHUNK_BITS; }
// index bits of chunk c: min(8, n_vars - 8 c)
inline unsigned sparse_chunk_bits(unsigned n_vars, unsigned c) {
    const unsigned done = c * SPARSE_CHUNK_BITS;
    return n_vars - done < SPARSE_CHUNK_BITS ? n_vars - done : SPARSE_CHUNK_BITS;
}

inline bool below_p(const pk::fe& x) { return pk::fe_eq(x, pk::fe_reduce_any(x)); }

// the offsets' rule: offsets[0] = 0, non-decreasing, no weight longer than 2^n_vars
inline bool sparse_offsets_ok(const uint64_t* offsets, unsigned l, unsigned n_vars, std::string& why) {
    if (offsets[0] != 0) {
        why = "offsets[0] must be 0 (weight 0, entry 0)";
        return false;
    }
    for (unsigned i = 0; i < l; i++) {
        if (offsets[i + 1] < offsets[i]) {
            why = "offsets decrease at weight " + std::to_string(i) + " (entry " + std::to_string(offsets[i]) + " of the lists)";
            return false;
        }
        if (offsets[i + 1] - offsets[i] > ((uint64_t)1 << n_vars)) {
            why = "weight " + std::to_string(i) + " has more entries than the table has positions (entry " + std::to_string((uint64_t)1 << n_vars) + ")";
            return false;
        }
    }
    return true;
}
// the reason for the first offending entry k of the concatenated lists (prev: index[k - 1], read only inside a weight)
inline std::string sparse_index_reason(const SparseWeights& w, size_t k, uint32_t at, uint32_t prev, unsigned n_vars) {
    unsigned i = 0;
    while (i + 1 < w.l && k >= w.offsets[i + 1]) i++;
    const size_t e = k - w.begin(i);
    std::string s = "weight " + std::to_string(i) + ", entry " + std::to_string(e) + ": index " + std::to_string(at);
    if (((uint64_t)at >> n_vars) != 0) return s + " is not below 2^" + std::to_string(n_vars);
    return s + " is not above the entry before it (" + std::to_string(prev) + "): indexes increase strictly within a weight";
}

// ---- the host's evaluation: sum_k value[k] * eq(index[k], point) with one product per chunk and entry -----------------------------
// tables for eq(., point) over n_vars variables, variable 0 <-> the most significant index bit: table c holds the eq factor of
// index bits [8 c, 8 c + 8) for each of their values, built by doubling (2^bits products per table)
struct SparseEqTables {
    unsigned n_vars = 0, chunks = 0;
    std::vector<pk::fe> t[SPARSE_MAX_CHUNKS];
    SparseEqTables(const pk::fe* point, unsigned n) : n_vars(n), chunks(sparse_chunks(n)) {
        for (unsigned c = 0; c < chunks; c++) {
            const unsigned bits = sparse_chunk_bits(n, c);
            std::vector<pk::fe>& tab = t[c];
            tab.assign((size_t)1 << bits, pk::fe_one());
            for (unsigned j = 0; j < bits; j++) {  // index bit 8 c + j <-> variable n - 1 - (8 c + j)
                const pk::fe r = point[n - 1 - (c * SPARSE_CHUNK_BITS + j)], nr = pk::h_sub(pk::fe_one(), r);
                for (size_t x = 0; x < ((size_t)1 << j); x++) {
                    tab[x + ((size_t)1 << j)] = pk::h_mul(tab[x], r);
                    tab[x] = pk::h_mul(tab[x], nr);
                }
            }
        }
    }
    pk::fe eq(uint32_t index) const {
        pk::fe acc = pk::fe_one();
        for (unsigned c = 0; c < chunks; c++) {
            const pk::fe& f = t[c][(index >> (c * SPARSE_CHUNK_BITS)) & ((1u << SPARSE_CHUNK_BITS) - 1)];
            acc = c ? pk::h_mul(acc, f) : f;
        }
        return acc;
    }
    // values Montgomery, < p
    pk::fe weight_at(const uint32_t* index, const uint64_t* value, size_t nnz) const {
        pk::fe acc = pk::fe_zero();
        for (size_t k = 0; k < nnz; k++) acc = pk::h_add(acc, pk::h_mul(eq(index[k]), pk::h_load(value + 4 * k)));
        return acc;
    }
};

// ---- sparse.hip --------------------------------------------------------------------------------------------------------------------
// the grids: the sums take one step per workgroup until the dense kernel's grid is reached, the evaluation SPARSE_EVAL_STEPS; neither
// grid exceeds wsum_grid(n_vars), so a pass's partials (rows * SPARSE_PASS * grid elements) fit where a dense pass's do
unsigned sparse_grid(unsigned n_vars, size_t max_nnz, unsigned steps);
size_t sparse_partial_fes(unsigned batch, unsigned n_vars);
// The validation pass over index[0 .. offsets[l]): index < 2^n_vars, strictly increasing within a weight.  d_slot: 8 bytes of
// device scratch.  Blocks on `stream`.  PK_OK with *bad = ~0 when every entry is good, else *bad = the first offending entry of the
// concatenated lists and *at / *prev the index there and before it (sparse_index_reason makes the message)
int sparse_validate(pk_ctx* ctx, hipStream_t stream, const SparseWeights& w, unsigned n_vars, uint64_t* d_slot, size_t* bad, uint32_t* at, uint32_t* prev);
// The launches trust the lists: validated, offsets checked.  Enqueue on `stream`:
// d_out[b * l + i] = sum_k value_i[k] * d_evals[b][index_i[k]]; grid = 0: sparse_grid's; any grid up to wsum_grid(n_vars) gives the same bits
int sparse_sums_launch(hipStream_t stream, const uint64_t* const* d_evals, unsigned batch, unsigned n_vars, const SparseWeights& w, uint64_t* d_partial,
                       uint64_t* d_out, unsigned grid = 0);
// d_table[index_i[k]] += scales[i] * value_i[k]; scales: l HOST elements (Montgomery, < p); the table's elements < p.  One launch
// per weight in stream order: inside a launch the indexes are distinct, so no position has two writers
int sparse_accumulate_launch(hipStream_t stream, uint64_t* d_table, const SparseWeights& w, const uint64_t* scales);
// d_out[i] = sum_k value_i[k] * eq(index_i[k], d_point); d_point: n_vars elements on the device
int sparse_evaluate_launch(hipStream_t stream, unsigned n_vars, const SparseWeights& w, const uint64_t* d_point, uint64_t* d_partial, uint64_t* d_out);

}  // namespace pkw
