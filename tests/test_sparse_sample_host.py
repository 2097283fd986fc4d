"""CPU: the data of tests/test_gpu_sparse_sample.py holds the edges it claims, and the NumPy restatement
of the sparse sample-space Gram (tests/sparse_sample_data.py: the Gram-blocked copy of the CSC and the
walk's summation order) gives A diag(h) Aᵀ -- exactly on the integer cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_sample_data as D  # noqa: E402


def _rows(t, r):
    ip, ix, dv = t
    return ix[ip[r]:ip[r + 1]], dv[ip[r]:ip[r + 1]]


@pytest.mark.parametrize("n", D.P_SIZES + (D.BIG_N,))
def test_edges_are_in_the_data(n):
    c = D.gram_case(n) if n != D.BIG_N else D.big_case()
    m = c.m
    assert n + 1 <= m                                              # the sample-space branch
    if n == D.BIG_N:
        assert (n - 1) >> 12 == 1 and n + 1 <= m < n + 128         # two blocks of 4096, close to the branch edge
    cnt_col = np.bincount(c.stored[1], minlength=m)
    lens = np.diff(c.stored[0])
    assert cnt_col[D.EMPTY_COL] == 0
    # the raw rows hold the same entries as the stored ones; the stored ones are sorted, stably
    for r in range(n):
        ci, vi = _rows(c.raw, r)
        cs, vs = _rows(c.stored, r)
        o = np.argsort(ci, kind="stable")
        assert np.array_equal(ci[o], cs) and np.array_equal(vi[o], vs) and np.all(np.diff(cs) >= 0)
    if n == 1:   # the one row: dense (more than 64 entries: a second trip), one column twice, unsorted
        ci, _ = _rows(c.raw, 0)
        assert lens[0] == m and np.sum(ci == c.dup_col) == 2 and np.any(np.diff(ci) < 0)
        return
    assert lens[D.EMPTY_ROW] == 0
    assert lens[D.DENSE_ROW] == m - 1 > 64                         # more than one trip of 64 row entries
    assert cnt_col[D.DENSE_COL] == n - 1                           # every row but the empty one
    if n > 65:
        assert cnt_col[D.DENSE_COL] > 64                           # a segment longer than one trip
    ci, _ = _rows(c.raw, D.DUP_ROW)
    assert np.sum(ci == c.dup_col) == 2 and np.any(np.diff(ci) < 0)
    cs, _ = _rows(c.stored, D.DUP_ROW)
    assert np.sum(np.diff(cs) == 0) == 1
    if n == 300:
        assert (n - 1) >> 7 == 2                                   # three sample blocks at shift 7
    if n in (127, 128, 129):
        assert -(-127 // 128) == 1 and -(-129 // 128) == 2         # the 128-row diagonal-tile edge


def test_integer_data_is_exact():
    for c in (D.gram_case(300), D.big_case()):
        ip, ix, dv = c.stored
        assert np.all(dv == np.round(dv)) and np.all(np.abs(dv) <= 3) and np.all(dv != 0)
        assert np.all(np.isin(c.h, [0.25, 0.5, 1.0, 2.0, 4.0]))
        # |P| <= 4 · 9 · (entries of a row + 1): far below 2^53 quarter-units
        assert 4 * 36 * (np.diff(ip).max() + 1) < 2 ** 40


@pytest.mark.parametrize("shift", [7, 12])
@pytest.mark.parametrize("n", D.P_SIZES)
def test_blocked_copy_and_walk(n, shift):
    c = D.gram_case(n)
    m = c.m
    colptr, rowidx, valT = D.csc_of(c.stored, n, m)
    assert colptr[-1] == c.stored[1].size
    for j in (D.DENSE_COL, c.dup_col):   # ascending rows; the duplicated entry twice, in storage order
        assert np.all(np.diff(rowidx[colptr[j]:colptr[j + 1]]) >= 0)
    ptr, lidx, val, nblk = D.gram_blocked_columns(colptr, rowidx, valT, n, m, shift)
    assert nblk == max(-(-n // (1 << shift)), 1) and ptr[-1] == colptr[-1] and lidx.size == val.size == ptr[-1]
    # the segments of a column, block after block, are the column
    for j in (D.DENSE_COL, D.EMPTY_COL, c.dup_col, m - 1):
        seg = [(b << shift) + lidx[ptr[b * m + j]:ptr[b * m + j + 1]].astype(np.int64) for b in range(nblk)]
        assert np.array_equal(np.concatenate(seg), rowidx[colptr[j]:colptr[j + 1]])
        assert all(np.all(s >> shift == b) for b, s in enumerate(seg))
    P = D.sample_gram_walk(c.stored, n, m, c.h, shift)
    assert np.array_equal(P, D.dense_gram(c))     # integer data: exact
    A = c.scipy().toarray()
    assert np.array_equal(P, (A * c.h) @ A.T)


def test_walk_on_the_two_block_case():
    c = D.big_case()
    P = D.sample_gram_walk(c.stored, c.n, c.m, c.h, 12)
    assert np.array_equal(P, D.dense_gram(c))


def test_walk_on_real_values():
    c = D.gram_case(129, integer=False)
    P7 = D.sample_gram_walk(c.stored, c.n, c.m, c.h, 7)
    P12 = D.sample_gram_walk(c.stored, c.n, c.m, c.h, 12)
    assert np.array_equal(P7, P12)                # the block width changes no summation order
    np.testing.assert_allclose(P7, D.dense_gram(c), rtol=1e-12, atol=1e-12)


def test_view_cases_take_the_sample_branch():
    A, y, x0, batches = D.view_case("partial")
    m = A.shape[1]
    assert [len(b) for b in batches] == [400, 400, 400, 300, 10] and all(len(b) + 1 <= m for b in batches)
    assert len(np.unique(batches[1])) == 399
    assert A[batches[4]].nnz == 0 and A[700].nnz == m - 3
    assert set(np.unique(y)) == {0.0, 1.0}
    A, y, x0, batches = D.view_case("big")
    assert [len(b) for b in batches] == [D.BIG_N] and D.BIG_N + 1 <= A.shape[1]
    assert np.all(np.diff(A.indptr) == D.BIG_PER_ROW)
