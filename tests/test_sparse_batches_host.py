"""CPU side of the sparse batch views (scs_set_sparse_batches):

* the shapes of tests/test_gpu_sparse_batches.py (tests/sparse_batch_data.py) really have the edges
  they are chosen for: block counts, every batch-size class, empty rows and columns, the dense row,
  the repeated row;
* a NumPy restatement of the row-side argument: the blocked row copy of A[rows, :] is the
  concatenation, block by block and in batch order, of the rows' segments of A's blocked row copy --
  sorted and padded already -- for both slot widths;
* the views' bookkeeping (csrc/batch_plan.h) under the host sanitizers, against a Python statement of
  the rule.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_batch_data as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "batch_plan_check.cpp")
BLOCK, PAD = D.BLOCK, D.BLOCK     # the widest block; the pad index is the zero slot past it


def nblocks(ncols):
    shift = 0
    while shift < 14 and (1 << shift) < ncols:
        shift += 1
    return -(-ncols // (1 << shift)), shift


def _common(A, batches):
    N, m = A.shape
    lens = np.diff(A.indptr)
    assert A.has_sorted_indices and (lens == 0).any()                       # empty rows
    assert (np.bincount(A.indices, minlength=m) == 0).any()                 # empty columns
    nb, shift = nblocks(m)
    dense = [r for r in np.flatnonzero(lens >= nb) if
             len(set(A.indices[A.indptr[r]:A.indptr[r + 1]] >> shift)) == nb and lens[r] >= m - 4]
    assert dense, "one row dense in every column block"
    held = np.concatenate(batches)
    assert np.intersect1d(held, dense).size, "the dense row is stepped on"
    assert (lens[held] == 0).any(), "an empty row is stepped on"
    for b in batches:
        assert not np.array_equal(b, np.sort(b)) or b.size == 1             # shuffled
    return nb, shift


def test_partial_case():
    A, y, x0, batches = D.case("partial")
    assert A.shape == (1500, 96) and y.shape == (1500,) and x0.shape == (96,)
    nb, _ = _common(A, batches)
    assert nb == 1
    assert [b.size for b in batches] == [400, 400, 400, 300, 10]           # a partial last loader batch
    assert np.unique(batches[1]).size == 399                                # one row twice
    assert np.diff(A.indptr)[batches[4]].sum() == 0                         # nnz_b = 0
    assert all(nblocks(b.size)[0] == 1 for b in batches)


def test_two_col_blocks_case():
    A, _, _, batches = D.case("two_col_blocks")
    assert A.shape == (2100, 16384 + 130)
    nb, shift = _common(A, batches)
    assert (nb, shift) == (2, 14)
    assert tuple(b.size for b in batches) == (1, D.WAVE - 1, D.WAVE, D.WAVE + 1, D.SPB_ROWS, D.SPB_ROWS + 1)
    assert np.unique(batches[2]).size == D.WAVE - 1                         # one row twice
    assert abs(A.nnz / 2100 - 6) < 8.5                                      # ~6 per row beside the dense row
    for b in batches:                                                       # both blocks take part in every batch
        blk = np.unique(A[b].indices >> shift)
        assert blk.size == 2 or b.size < 64
    assert np.unique(A[batches[0]].indices >> shift).size == 2
    assert A[:, BLOCK - 1].nnz and A[:, BLOCK].nnz                          # both sides of the x-slice edge


def test_two_row_blocks_case():
    A, _, _, batches = D.case("two_row_blocks")
    assert A.shape == (40000, 48)
    _common(A, batches)
    (b,) = batches
    assert b.size == 16384 + 40 and nblocks(b.size) == (2, 14)              # two row blocks in the batch's bcsc
    assert np.unique(b).size == b.size
    assert int(np.flatnonzero(b == 5)[0]) >= 0
    csc = A[b].tocsc()
    assert ((csc.indices >> 14) == 1).any() and ((csc.indices >> 14) == 0).any()


def test_wide_case():
    A, _, _, batches = D.case("wide")
    assert A.shape == (8192, 131072) and [b.size for b in batches] == [4096, 4096]
    assert np.array_equal(np.sort(np.concatenate(batches)), np.arange(8192))
    _common(A, batches)
    # the layout's arithmetic: the sparse view is a few MB against the dense view's 4 GiB
    n, m = 4096, 131072
    entries = 4 * (A[batches[0]].nnz + 8 * n)             # every (row, block) segment padded to a 4-entry slot, at most
    view = 2 * entries * 10 + 8 * 8 * n + 8 * (m + 1) + 8 * (8 + 6) * n + 8 * m
    assert view < 32 << 20 < n * m * 8 // 16


def test_int_traj_data_is_exact():
    S, y, x0, perm, c8 = D.int_traj_data()
    assert S.shape == (1500, 96) and abs(S.nnz / (1500 * 96) - 0.08) < 1e-3
    for a in (S.data, y, x0):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 5
    assert c8 == 2.0 ** -8 and np.array_equal(np.sort(perm), np.arange(1500))


# ---- the row-side argument ---------------------------------------------------------------------------
def blocked(A, slot):
    """The LDS-blocked row copy of a row-sorted CSR (sparse.hip): for block b (2^shift columns) and row r
    the row's entries in that block, local indices, padded to whole slots with (PAD, 0); segments in
    block-major order.  -> ptr (nblk·N + 1), lidx, val"""
    N, m = A.shape
    nb, shift = nblocks(m)
    ptr, lidx, val = [0], [], []
    for b in range(nb):
        for r in range(N):
            c = A.indices[A.indptr[r]:A.indptr[r + 1]]
            v = A.data[A.indptr[r]:A.indptr[r + 1]]
            k = (c >> shift) == b
            n = int(k.sum())
            padn = -n % slot
            lidx += list(c[k] & ((1 << shift) - 1)) + [PAD] * padn
            val += list(v[k]) + [0.0] * padn
            ptr.append(len(lidx))
    return np.array(ptr), np.array(lidx, dtype=np.int64), np.array(val)


def slice_blocked(full, N, rows, nb):
    """What blk_slice_size / blk_scan / blk_slice_copy do: whole segments, copied verbatim"""
    ptr, lidx, val = full
    optr, oidx, oval = [0], [], []
    for b in range(nb):
        for r in rows:
            s, e = ptr[b * N + r], ptr[b * N + r + 1]
            oidx += list(lidx[s:e])
            oval += list(val[s:e])
            optr.append(len(oidx))
    return np.array(optr), np.array(oidx, dtype=np.int64), np.array(oval)


@pytest.mark.parametrize("slot", [4, 8])
def test_slice_of_the_blocked_copy_is_the_blocked_copy_of_the_slice(slot):
    rng = np.random.default_rng(5)
    N, m = 37, 2 * BLOCK + 9                          # three column blocks
    rows_cols = [np.sort(rng.choice(m, n, replace=False)) for n in rng.integers(0, 12, size=N)]
    rows_cols[3] = np.array([], dtype=np.int64)
    rows_cols[11] = np.sort(np.concatenate([np.arange(BLOCK - 5, BLOCK + 6), [2 * BLOCK, m - 1]]))
    indptr = np.concatenate([[0], np.cumsum([c.size for c in rows_cols])])
    indices = np.concatenate(rows_cols)
    A = sp.csr_matrix((rng.standard_normal(indices.size), indices, indptr), shape=(N, m))
    full = blocked(A, slot)
    assert (full[0] % slot == 0).all()                # segments start slot-aligned
    for rows in ([11], [3, 3], rng.permutation(N)[:20], np.array([5, 11, 5, 0, 36, 3, 11])):
        rows = np.asarray(rows)
        got = slice_blocked(full, N, rows, 3)
        want = blocked(A[rows], slot)                 # scipy keeps batch order and a repeated row twice
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


# ---- the bookkeeping under the sanitizers -------------------------------------------------------------
def model(budget, batches, epochs):
    """The rule of DESIGN §2f: a view is kept, in the order built, while the kept bytes stay within the
    budget; the others share one refillable slot per size, rebuilt when it holds another batch."""
    slots, kept_bytes, builds = [], 0, 0       # slot: [n, batch, bytes, kept]
    for _ in range(epochs):
        for b, (n, nbytes) in enumerate(batches):
            if any(s[1] == b for s in slots):
                continue
            builds += 1
            if kept_bytes + nbytes <= budget:
                slots.append([n, b, nbytes, True])
                kept_bytes += nbytes
                continue
            for s in slots:
                if not s[3] and s[0] == n:
                    s[1], s[2] = b, nbytes
                    break
            else:
                slots.append([n, b, nbytes, False])
    where = [next((i for i, s in enumerate(slots) if s[1] == b), -1) for b in range(len(batches))]
    return builds, len(slots), kept_bytes, sum(s[2] for s in slots), where


SCENARIOS = {4: [(400, 1000), (400, 1010), (400, 990), (300, 800)], 40: [(1, 8 * 96 + 64)] * 40,
             7: [(64, 500), (65, 500), (64, 700), (1, 100), (65, 100), (1, 100), (64, 10)]}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "batch_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 10 * 3 * 3
    seen_hit_loss = False
    for ln in lines:
        head, tail = ln.split(":")
        budget, nb, epochs, builds, nslots, kept, total = (int(v) for v in head.split())
        where = [int(v) for v in tail.split()]
        assert (builds, nslots, kept, total, where) == model(budget, SCENARIOS[nb], epochs), ln
        if nb == 4 and epochs == 3:
            if budget >= 3800:
                assert builds == 4              # every view kept: built once
            if budget == 0:
                assert builds > 4 and nslots == 2
                seen_hit_loss = True
        if nb == 40:                            # one-row batches: the budget bounds what they hold
            assert kept <= budget and total <= max(budget, 0) + 8 * 96 + 64
    assert seen_hit_loss
