"""Data of the sparse-batch tests (tests/test_gpu_sparse_batches.py; its claims are checked on the CPU
by tests/test_sparse_batches_host.py).  Every matrix has empty rows, empty columns and one row that is
dense in every column block; every batch list is shuffled, and the lists of the view tests hold one
batch with a repeated row.  Built once per process.

case(name) -> (A: scipy CSR with sorted rows and no duplicate entries, y, x0, batches)
  partial         N = 1500, m = 96, about 8 entries per row; shuffled batches of 400 (the last one 300
                  rows), batch 1 with one row twice, and a batch of empty rows only (nnz_b = 0)
  two_col_blocks  N = 2100, m = 16384 + 130, 6 entries per row: two column blocks in the row copy;
                  batches of 1, 63, 64, 65, 1024 and 1025 rows (the slice kernel's wave of 64 rows and
                  workgroup of SPB_ROWS = 1024 rows, and their neighbours)
  two_row_blocks  N = 40000, m = 48, 3 entries per row; one batch of 16384 + 40 rows: two row blocks in
                  the batch's column copy
  wide            N = 8192, m = 131072, 8 entries per row; two batches of 4096 rows
"""
import functools

import numpy as np
import scipy.sparse as sp

BLOCK = 1 << 14        # SPB_MAXSHIFT: the widest LDS block (sparse.hip)
WAVE, SPB_ROWS = 64, 1024
SIZES_COL_BLOCKS = (1, 63, 64, 65, 1024, 1025)


def _csr(N, m, per_row, rng, empty_rows, dense_row, empty_cols):
    """`per_row` distinct random columns per row (one from each of per_row equal strata of the columns,
    so they are distinct and ascending), rows in empty_rows without entries, columns in empty_cols
    without entries (none of them the last of a stratum: a hit moves one column up), dense_row with
    every other column"""
    w = m // per_row
    cols = np.arange(per_row)[None, :] * w + rng.integers(0, w, size=(N, per_row))
    cols[np.isin(cols, empty_cols)] += 1
    full = np.setdiff1d(np.arange(m), empty_cols)
    lens = np.full(N, per_row, dtype=np.int64)
    lens[list(empty_rows)] = 0
    lens[dense_row] = full.size
    indptr = np.zeros(N + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.empty(indptr[-1], dtype=np.int64)
    for r in range(N):
        if r == dense_row:
            indices[indptr[r]:indptr[r + 1]] = full
        elif lens[r]:
            indices[indptr[r]:indptr[r + 1]] = np.sort(cols[r])
    data = rng.standard_normal(indices.size) * 3.0
    A = sp.csr_matrix((data, indices, indptr), shape=(N, m))
    A.sort_indices()
    return A


def _finish(A, rng, batches):
    N, m = A.shape
    y = rng.standard_normal(N)
    x0 = rng.standard_normal(m) * 0.3
    return A, y, x0, [np.asarray(b, dtype=np.int64) for b in batches]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "partial":
        N, m = 1500, 96
        rng = np.random.default_rng(101)
        A = sp.random(N, m, density=0.08, random_state=3, format="lil") * 3.0
        empty = list(range(10)) + [777, N - 1]
        for r in empty:
            A[r, :] = 0.0
        A[700, :] = rng.standard_normal(m)                   # the dense row
        for c in (5, 50, m - 1):                             # empty columns (the dense row included)
            A[:, c] = 0.0
        A = A.tocsr()
        A.eliminate_zeros()
        A.sort_indices()
        perm = rng.permutation(N)
        batches = [perm[i:i + 400].copy() for i in range(0, N, 400)]
        batches[1][7] = batches[1][3]                        # one row twice
        batches.append(rng.permutation(empty[:10]))          # rows without entries only
        return _finish(A, rng, batches)
    if name == "two_col_blocks":
        N, m = 2100, BLOCK + 130
        rng = np.random.default_rng(102)
        A = _csr(N, m, 6, rng, empty_rows=range(0, N, 97), dense_row=1000, empty_cols=(2, m - 3))
        batches = [rng.choice(N, n, replace=False) for n in SIZES_COL_BLOCKS]
        batches[2][5] = batches[2][2]                        # one row twice (the 64-row batch)
        for k in (3, 5):                                     # the dense row in the 65- and the 1025-row batch
            if 1000 not in batches[k]:
                batches[k][1] = 1000
        # entries on both sides of the block edge in the smallest batches too
        A = A.tolil()
        A[int(batches[0][0]), BLOCK - 1] = 1.5
        A[int(batches[0][0]), BLOCK] = -2.5
        A = A.tocsr()
        A.sort_indices()
        return _finish(A, rng, batches)
    if name == "two_row_blocks":
        N, m = 40000, 48
        rng = np.random.default_rng(103)
        A = _csr(N, m, 3, rng, empty_rows=range(3, N, 101), dense_row=5, empty_cols=(2, m - 2))
        rows = rng.choice(N, BLOCK + 40, replace=False)
        if 5 not in rows:
            rows[BLOCK + 7] = 5                              # the dense row, in the second row block
        return _finish(A, rng, [rows])
    if name == "wide":
        N, m = 8192, 131072
        rng = np.random.default_rng(104)
        A = _csr(N, m, 8, rng, empty_rows=range(0, N, 113), dense_row=4000, empty_cols=(2, m - 3))
        perm = rng.permutation(N)
        return _finish(A, rng, [perm[:4096], perm[4096:]])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def int_traj_data():
    """The pattern of test_sparse_minibatches_gathered_dense (N = 1500, m = 96, density 0.08) with small
    integer values, integer y and x0 and the loss constant 2^-8: every product and sum of the loss is
    exact in either form of it (tests/test_gpu_samplewise.py's data rule).  -> (S, y, x0, perm, c8)"""
    N, m = 1500, 96
    rng = np.random.default_rng(19)
    S = sp.random(N, m, density=0.08, random_state=3, format="csr")
    S.data = rng.integers(1, 4, size=S.data.size).astype(np.float64) * rng.choice([-1.0, 1.0], size=S.data.size)
    S.sort_indices()
    y = rng.integers(-5, 6, size=N).astype(np.float64)
    x0 = rng.integers(-2, 3, size=m).astype(np.float64)
    return S, y, x0, np.random.default_rng(4).permutation(N), 2.0 ** -8
