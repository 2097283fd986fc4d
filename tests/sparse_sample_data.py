"""Data of the sparse sample-space tests (tests/test_gpu_sparse_sample.py; its claims are checked on the
CPU by tests/test_sparse_sample_host.py), and a NumPy restatement of what scs_set_sparse_sample builds
and sums: the Gram-blocked copy of the CSC and P = A diag(h) Aᵀ in the walk's order.

gram_case(n, m, per_row, integer) -> Case: a CSR as it is handed to the device door (`raw`: a row with
unsorted entries and a duplicated column) and as the door stores it (`stored`: every row sorted by
column, stably, duplicates kept in storage order), the weights h, and which rows / columns carry the
edges.  Every data set with n >= 3 rows holds
  * an empty row (row 0) and an empty column (column 1),
  * a dense column (column 0: an entry in every row but the empty one), so with n > 65 a segment longer
    than 64 entries, i.e. longer than one trip of the plain walk and of the packed walk,
  * a dense row (row 1: every column but the empty one, m - 1 > 64 entries: several trips of 64 row
    entries),
  * a row (row 2) whose entries are handed over unsorted and with one column twice.
One row cannot be empty, dense and duplicated at once: n = 1 holds the dense row alone, given a
duplicated column and scrambled; n = 2 is not used.

Integer data (integer=True): entries in {-3..3} \\ {0}, h in {1/4, 1/2, 1, 2, 4}: every product and
every partial sum is an integer multiple of 1/4 below 2^53, so any summation order gives the same
bits and NumPy's P is the reference.  integer=False: normal entries, positive real h -- for bitwise
comparisons between arms, shifts and contexts.
"""
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

P_SIZES = (1, 63, 64, 65, 127, 128, 129, 300)   # samples at m = 512, SCS_SPARSE_GRAM_SHIFT = 7
P_M = 512
BIG_N, BIG_M, BIG_PER_ROW = 4096 + 40, 4200, 8   # the default shift: two blocks of 4096, n + 1 <= m
EMPTY_ROW, DENSE_ROW, DUP_ROW = 0, 1, 2
DENSE_COL, EMPTY_COL = 0, 1


@dataclass(frozen=True)
class Case:
    n: int
    m: int
    raw: tuple      # (indptr, indices, data) as handed to the device door
    stored: tuple   # (indptr, indices, data) as the door stores them: rows sorted by column, stably
    h: np.ndarray
    dup_col: int    # the column DUP_ROW (or, n = 1, the dense row) holds twice

    def scipy(self):
        """the matrix (duplicates summed)"""
        ip, ix, dv = self.stored
        return sp.csr_matrix((dv, ix, ip), shape=(self.n, self.m))


def _values(rng, size, integer):
    if integer:
        return rng.integers(1, 4, size=size).astype(np.float64) * rng.choice([-1.0, 1.0], size=size)
    return rng.standard_normal(size) * 2.0


@functools.lru_cache(maxsize=None)
def gram_case(n, m=P_M, per_row=8, integer=True, seed=0):
    rng = np.random.default_rng(1000 * n + m + seed)
    others = np.arange(2, m)
    rows = []
    dup_col = -1
    for r in range(n):
        if n == 1 or r == DENSE_ROW:
            c = np.setdiff1d(np.arange(m), [EMPTY_COL])
            if n == 1:   # the only row: dense, one column twice, scrambled
                dup_col = int(c[70])
                c = rng.permutation(np.concatenate([c, [dup_col]]))
        elif r == EMPTY_ROW:
            c = np.zeros(0, dtype=np.int64)
        else:
            c = np.concatenate([[DENSE_COL], np.sort(rng.choice(others, per_row - 1, replace=False))])
            if r == DUP_ROW:
                dup_col = int(c[3])
                c = np.concatenate([c[::-1], [dup_col]])   # descending, and one column once more
        rows.append((c.astype(np.int64), _values(rng, c.size, integer)))
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([c.size for c, _ in rows])
    raw = (indptr, np.concatenate([c for c, _ in rows]), np.concatenate([v for _, v in rows]))
    srt = [np.argsort(c, kind="stable") for c, _ in rows]
    stored = (indptr, np.concatenate([c[o] for (c, _), o in zip(rows, srt)]),
              np.concatenate([v[o] for (_, v), o in zip(rows, srt)]))
    h = (2.0 ** rng.integers(-2, 3, size=m)) if integer else rng.random(m) + 0.25
    return Case(n, m, raw, stored, h, dup_col)


def big_case(integer=True):
    return gram_case(BIG_N, BIG_M, BIG_PER_ROW, integer)


# ---- what the library builds, restated --------------------------------------------------------------
def csc_of(stored, n, m):
    """The door's transposition: the columns with their entries in ascending row order, the entries of
    one row (duplicates) in storage order -> (colptr, rowidx, valT)."""
    ip, ix, dv = stored
    rows = np.repeat(np.arange(n), np.diff(ip))
    o = np.argsort(ix, kind="stable")   # the rows are visited in order, so this is stable in (row, storage)
    colptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(colptr, ix + 1, 1)
    return np.cumsum(colptr), rows[o], dv[o]


def gram_blocked_columns(colptr, rowidx, valT, n, m, shift):
    """The Gram-blocked copy of the CSC: segment (b, j) = the entries of column j whose row lies in block
    b of 2^shift rows, unpadded, at ptr[b·m + j]; local row indices -> (ptr, lidx, val, nblk)."""
    nblk = max(-(-n // (1 << shift)), 1)
    cols = np.repeat(np.arange(m), np.diff(colptr))
    blk = rowidx >> shift
    key = blk * m + cols
    cnt = np.bincount(key, minlength=nblk * m)
    ptr = np.zeros(nblk * m + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(cnt)
    o = np.argsort(key, kind="stable")
    return ptr, (rowidx[o] & ((1 << shift) - 1)).astype(np.uint16), valT[o], nblk


def sample_gram_walk(stored, n, m, h, shift):
    """P in the order of the walk: item (sample i, block b <= i >> shift) adds, for row i's entries
    (j, a_ij) in stored order, (h_j a_ij) · a_kj over column j's segment in block b, in segment order,
    into an accumulator of 2^shift slots; column i of the upper triangle, symmetrized."""
    ip, ix, dv = stored
    colptr, rowidx, valT = csc_of(stored, n, m)
    ptr, lidx, val, nblk = gram_blocked_columns(colptr, rowidx, valT, n, m, shift)
    BS = 1 << shift
    P = np.zeros((n, n))
    for i in range(n):
        for b in range((i >> shift) + 1):
            acc = np.zeros(BS)
            for p in range(ip[i], ip[i + 1]):
                j = ix[p]
                s = h[j] * dv[p]
                s0, s1 = ptr[b * m + j], ptr[b * m + j + 1]
                np.add.at(acc, lidx[s0:s1], s * val[s0:s1])   # unbuffered, in segment order
            lo = b * BS
            hi = min(lo + BS, i + 1)
            P[lo:hi, i] = acc[:hi - lo]
    return np.triu(P) + np.triu(P, 1).T


def dense_gram(case):
    """A diag(h) Aᵀ by scipy's sparse product (exact on the integer cases)"""
    S = case.scipy()
    return np.asarray((S.multiply(case.h[None, :]).tocsr() @ S.T.tocsr()).todense())


# ---- batch data of the view tests --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def view_case(name):
    """-> (A: scipy CSR, sorted rows, no duplicates; y in {0, 1}; x0; batches), every batch n_b + 1 <= m.
      partial  N = 1500, m = 512, about 8 entries per row, empty rows, a dense row, empty columns;
               shuffled batches of 400 (the last one 300 rows), batch 1 with one row twice, and a batch
               of empty rows only (P = 0: the system is the identity plus the λ·gr border)
      big      N = 6000, m = 4200, 8 entries per row; one batch of 4096 + 40 rows: two sample blocks at
               the default shift and the branch edge n_b + 1 <= m"""
    if name == "partial":
        N, m = 1500, 512
        rng = np.random.default_rng(201)
        A = sp.random(N, m, density=8.0 / m, random_state=11, format="lil") * 3.0
        empty = list(range(10)) + [777, N - 1]
        for r in empty:
            A[r, :] = 0.0
        A[700, :] = rng.standard_normal(m)                   # the dense row
        for c in (5, 50, m - 1):                             # empty columns (the dense row included)
            A[:, c] = 0.0
        A = A.tocsr()
        perm = rng.permutation(N)
        batches = [perm[i:i + 400].copy() for i in range(0, N, 400)]
        batches[1][7] = batches[1][3]                        # one row twice
        batches.append(rng.permutation(empty[:10]))          # rows without entries only
    elif name == "big":
        N, m = 6000, BIG_M
        rng = np.random.default_rng(202)
        w = m // BIG_PER_ROW
        cols = np.arange(BIG_PER_ROW)[None, :] * w + rng.integers(0, w, size=(N, BIG_PER_ROW))
        A = sp.csr_matrix((rng.standard_normal(cols.size) * 2.0, cols.ravel(),
                           np.arange(0, cols.size + 1, BIG_PER_ROW)), shape=(N, m))
        batches = [rng.choice(N, BIG_N, replace=False)]
    else:
        raise KeyError(name)
    A.eliminate_zeros()
    A.sort_indices()
    y = (rng.random(N) < 0.5).astype(np.float64)
    x0 = rng.standard_normal(m) * 0.3
    return A, y, x0, [np.asarray(b, dtype=np.int64) for b in batches]
