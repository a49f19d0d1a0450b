"""Shared by test_whir_pcs_sparse_host.py and test_gpu_whir_pcs_sparse.py: deterministic sparse weights (index/value lists as
canonical ints), the dense tables they stand for, and Python-int definitions of the three operations on them.  The openings come
from whir_pcs_linear_cases.oracle_linear_opening over the DENSIFIED weights: a sparse weight is another way to write the same
statement down, so the oracle's transcript of the dense statement is the reference for the sparse one."""
import numpy as np

import whir_pcs_cases as K
import whir_pcs_linear_cases as L

P = K.P


def densify(n_vars, weight):
    """(indexes, values) -> the table of 2^n_vars canonical ints that is values[k] at indexes[k] and 0 elsewhere"""
    idx, val = weight
    table = [0] * (1 << n_vars)
    for i, v in zip(idx, val):
        table[i] = v
    return table


def random_weight(n_vars, nnz, seed):
    """nnz distinct positions in increasing order with random values"""
    N = 1 << n_vars
    rng = np.random.default_rng(seed)
    idx = sorted(int(x) for x in rng.choice(N, size=min(nnz, N), replace=False))
    return idx, K.random_ints(len(idx), seed + 1)


def weights(n_vars, l, seed=33):
    """l weights, by position: 0 a random list with the values 0, 1 and p - 1 planted; 1 no entry at all; 2 one entry at index 0;
    3 one entry at index 2^n - 1; 4 every position (nnz = 2^n); 5 the indexes of weight 0 with other values; then random lists
    of growing length"""
    N = 1 << n_vars
    out = []
    for i in range(l):
        if i == 0:
            idx, val = random_weight(n_vars, max(3, N // 8), seed)
            for k, special in enumerate((0, 1, P - 1)):
                if k < len(val):
                    val[k] = special
        elif i == 1:
            idx, val = [], []
        elif i == 2:
            idx, val = [0], K.random_ints(1, seed + 2)
        elif i == 3:
            idx, val = [N - 1], [P - 1]
        elif i == 4:
            idx, val = list(range(N)), K.random_ints(N, seed + 4)
        elif i == 5:
            idx, val = list(out[0][0]), K.random_ints(len(out[0][0]), seed + 5)
        else:
            idx, val = random_weight(n_vars, 1 + (i * N) // 20, seed + 10 * i)
        out.append((idx, val))
    return out


def pack(oracle, ws):
    """-> provekit_amd.whir_pcs.SparseWeights with Montgomery values"""
    from provekit_amd import whir_pcs

    return whir_pcs.SparseWeights([(np.array(idx, dtype=np.uint32), L.mont(oracle, val) if val else np.zeros((0, 4), dtype=np.uint64)) for idx, val in ws])


# ---- the three operations, in Python ints ------------------------------------------------------------------------------------------
def sums(polys, ws):
    """[b][i] = sum_k value_i[k] * poly_b[index_i[k]]"""
    return [[sum(v * f[i] for i, v in zip(idx, val)) % P for idx, val in ws] for f in polys]


def accumulate(table, ws, scales):
    """table[index_i[k]] += scales[i] * value_i[k], weight after weight"""
    out = list(table)
    for (idx, val), s in zip(ws, scales):
        for i, v in zip(idx, val):
            out[i] = (out[i] + s * v) % P
    return out


def eq_at(n_vars, index, point):
    """eq(index, point): variable 0 <-> the most significant index bit"""
    acc = 1
    for j in range(n_vars):
        r = point[j]
        acc = acc * (r if (index >> (n_vars - 1 - j)) & 1 else (1 - r)) % P
    return acc


def evaluate(n_vars, ws, point):
    """[i] = sum_k value_i[k] * eq(index_i[k], point)"""
    return [sum(v * eq_at(n_vars, i, point) for i, v in zip(idx, val)) % P for idx, val in ws]
