"""Shared data of the sparse multi-output minibatch tests (test_multi_sparse_batches_host.py,
test_gpu_multi_sparse_batches.py), built on multi_sparse_data.py (the sparse generator and the exact integer
cases) and multi_batches_data.py (the oracle, the shuffle, the branch rule): the row lists of the exact
product tests with their per-batch bounds, the trajectory cases, the oracle runs on A.toarray() (computed
once per process and shared) and the NumPy restatement of a sparse K-column view."""
import functools

import numpy as np

import multi_batches_data as B
import multi_output_data as M
import multi_sparse_data as S
from multi_batches_data import O

LIMIT = S.LIMIT
PAD = 1 << 14          # the blocked layouts' padding index (the zero slot)

# ---- the exact products on a view -------------------------------------------------------------------
# (N, d) of multi_sparse_data.exact_sparse_case -> the batches read from it, in order
EXACT_VIEW_SHAPES = [(700, 300), (300, 16500), (16500, 300)]
EXACT_K = S.EXACT_K


def exact_batches(N, d):
    """(700, 300): 300 unsorted rows with a repeated row, row N - 1 and an empty row (two 256-row workgroups,
    the second ragged).  (300, 16500): 33 rows and 1 row (two groups in A_b X from K = 3 on; 65 256-row
    workgroups with a ragged tail in A_bᵀ V).  (16500, 300): 1100 rows (two sub-blocks on the column side
    at K = 16, where multi_spmm_shift(1100, 16) = 10; five 256-row workgroups in A_b X, the last ragged)."""
    rng = np.random.default_rng(97 * N + d)
    if (N, d) == (700, 300):
        r = rng.permutation(N)[:300]
        r[7] = r[211]                      # a repeated row
        r[299] = N - 1
        r[100] = 5                         # an empty row of exact_sparse_case
        r[3] = N // 3                      # the dense row
        return [r.astype(np.int64)]
    if (N, d) == (300, 16500):
        r = rng.permutation(N)[:33]
        r[0] = N // 3
        r[32] = N - 1
        return [r.astype(np.int64), np.array([N // 3], dtype=np.int64)]
    if (N, d) == (16500, 300):
        r = rng.permutation(N)[:1100]
        r[1] = r[1000]
        r[1099] = N - 1
        r[500] = N // 3
        return [r.astype(np.int64)]
    raise KeyError((N, d))


@functools.lru_cache(maxsize=None)
def exact_view_case(N, d, K):
    """exact_sparse_case(N, d, K) with, per batch of exact_batches(N, d): the rows, an integer V_b (n_b x K,
    ±1000) and the int64 references S[rows_b] X and S[rows_b]ᵀ V_b.  Asserts Σ|terms| < 2^53 per batch -- a
    repeated row counts twice (scipy's row indexing keeps it twice), so the full case's bound does not carry
    over."""
    c = S.exact_sparse_case(N, d, K)
    Xi = c.X.astype(np.int64)
    out = []
    for k, rows in enumerate(exact_batches(N, d)):
        Sb = c.S[rows]
        Vb = np.random.default_rng(13 * N + d + 7 * K + k).integers(-1000, 1001, size=(rows.size, K), dtype=np.int64)
        absS = abs(Sb)
        bound = max(int(np.asarray(absS @ np.abs(Xi)).max()), int(np.asarray(absS.T @ np.abs(Vb)).max()))
        assert bound < LIMIT, f"batch {k}: max Σ|terms| = {bound} >= 2^53"
        AX = np.asarray(Sb @ Xi).astype(np.float64)
        ATV = np.asarray(Sb.T @ Vb).astype(np.float64)
        Vf = Vb.astype(np.float64)
        for a in (AX, ATV, Vf):
            a.setflags(write=False)
        out.append((rows, Vf, AX, ATV, bound))
    return c, out


# ---- trajectories ------------------------------------------------------------------------------------
# ((N, d, K), batch_size, batch sizes, ProxGGNSCORE's branch per batch) on multi_sparse_data.SHAPES
CASES = [
    ((300, 130, 3), 137, (137, 137, 26), "FFS"),
    # (batches of 100: on shuffled batches of 50 or 67 rows of this generator -- column 3 empty, density 0.15 --
    # the oracle's own softmax Gram methods reach obj ~ 1e84)
    ((200, 17, 7), 100, (100, 100), "FF"),           # odd K, two equal batches: one pool view re-gathered
    ((520, 129, 2), 260, (260, 260), "FF"),          # K = 2: the loop arm by default
    ((40, 33, 16), 17, (17, 17, 6), "SSS"),
]
assert [c[0] for c in CASES] == S.SHAPES
NSCORE_CASES = [c for c in CASES if min(c[2]) >= c[0][1]]
perm_of = B.perm_of
branches = B.branches


@functools.lru_cache(maxsize=None)
def oracle_run(kind, method, shape, batch_size, lam=2e-3, max_epoch=6, test=False, shuffle=True):
    """The oracle's minibatch loop on sparse_problem(shape).toarray() over shuffled batches of batch_size
    (perm_of(N)) or, shuffle=False, the rows in order.  Treat the result as read-only."""
    N, d, K = shape
    A, Y, x0 = S.sparse_problem(N, d, K)
    kw = {}
    if test:
        At, Yt, _ = S.sparse_problem(77, d, K, soft=True)
        kw = dict(Atest=At.toarray(), ytest=Yt)
    om = O.Problem(A.toarray(), Y, x0, M.oracle_loss(O, kind, d, K, 1.0 / N), lam, **kw)
    if shuffle:
        batches = O.loader_batches(N, batch_size, shuffle_batch=True, perm=perm_of(N))
    else:
        batches = O.loader_batches(N, batch_size, shuffle_batch=False)
    return O.iterate(B.OMETHODS[method](), om, "l1", O.PHuberSmootherL1L2(0.5), max_epoch=max_epoch, batches=batches)


# ---- the NumPy restatement of a sparse K-column view ---------------------------------------------------
def kp_of(K):
    return 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16


def blk_shift(ncols):
    """spmv_blk_shift: the smallest shift <= 14 with 2^shift >= ncols."""
    s = 0
    while s < 14 and (1 << s) < ncols:
        s += 1
    return s


def multi_shift(ncols, K):
    """multi_spmm_shift: the sub-block width W = 2^shift with W·KP <= 16384."""
    return min(blk_shift(ncols), 14 - (kp_of(K).bit_length() - 1))


def blocked(A, shift, slot):
    """The LDS-blocked row copy of a row-sorted scipy CSR cut at `shift`: for sub-block b and row r the row's
    entries in that sub-block as local indices, padded to whole slots with (PAD, 0); segments in sub-block-major
    order.  -> (ptr of nblk·N + 1 entries, lidx, val, nblk)"""
    N, m = A.shape
    nb = max(-(-m // (1 << shift)), 1)
    ptr, lidx, val = [0], [], []
    for b in range(nb):
        for r in range(N):
            c = A.indices[A.indptr[r]:A.indptr[r + 1]]
            v = A.data[A.indptr[r]:A.indptr[r + 1]]
            k = (c >> shift) == b
            padn = -int(k.sum()) % slot
            lidx += list(c[k] & ((1 << shift) - 1)) + [PAD] * padn
            val += list(v[k]) + [0.0] * padn
            ptr.append(len(lidx))
    return np.array(ptr), np.array(lidx, dtype=np.int64), np.array(val), nb


def slice_blocked(full, N, rows):
    """blk_slice_size / blk_scan / blk_slice_copy: the rows' whole segments of every sub-block, in batch order."""
    ptr, lidx, val, nb = full
    optr, oidx, oval = [0], [], []
    for b in range(nb):
        for r in rows:
            s, e = ptr[b * N + r], ptr[b * N + r + 1]
            oidx += list(lidx[s:e])
            oval += list(val[s:e])
            optr.append(len(oidx))
    return np.array(optr), np.array(oidx, dtype=np.int64), np.array(oval), nb


def blocked_product(blk, Xop, K, shift, nrows):
    """What the one-pass kernel and its reduction compute from a blocked copy: out[r, l] = Σ_groups Σ_entries
    val · Xop[(sub-block << shift) + lidx, l], the pad index reading the zero row; also the number of
    partials (groups of KP sub-blocks)."""
    ptr, lidx, val, nb = blk
    kp = kp_of(K)
    out = np.zeros((nrows, K))
    for b in range(nb):
        for r in range(nrows):
            s, e = ptr[b * nrows + r], ptr[b * nrows + r + 1]
            for j, v in zip(lidx[s:e], val[s:e]):
                if j != PAD:
                    out[r] += v * Xop[(b << shift) + j]
    return out, -(-nb // kp)
