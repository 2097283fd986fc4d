"""Shared data of the multi-output minibatch tests (test_multi_batches_host.py, test_gpu_multi_batches.py):
the trajectory cases with the branch ProxGGNSCORE takes on each batch, the oracle runs (computed once
per process and shared), and the row lists of the exact gather test."""
import functools
import os
import sys

import numpy as np

import multi_output_data as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402

# ((N, d, K), batch_size, batch sizes, the branch per batch: "F" feature (n_b K + 1 > d K), "S" sample space)
CASES = [
    ((300, 130, 3), 137, (137, 137, 26), "FFS"),    # one epoch mixes both branches; two column panels
    ((200, 17, 7), 50, (50, 50, 50, 50), "FFFF"),   # odd K, four equal batches: one pool view re-gathered
    ((520, 129, 2), 260, (260, 260), "FF"),         # one column past a panel
    ((129, 260, 2), 48, (48, 48, 33), "SSS"),       # n_b < d on every batch: the shape minibatches mostly have
    ((40, 33, 16), 17, (17, 17, 6), "SSS"),         # the largest K
]
# ProxNSCORE: every batch has n_b >= d (with fewer rows the batch Hessian is rank-deficient, and on
# (40, 33, 16) / 17 the oracle itself reaches obj ~ 2.7e56 with the softmax loss)
NSCORE_CASES = [c for c in CASES if min(c[2]) >= c[0][1]]
OMETHODS = {"ggn": O.ProxGGNSCORE, "nscore": O.ProxNSCORE, "lqn": lambda **kw: O.ProxLQNSCORE(m=5, **kw)}


def perm_of(N):
    return np.random.default_rng(3).permutation(N)


def branches(batches, d, K):
    """The oracle's rule (ggn_score_step_general: the sample branch when size(Q, 1) + 1 <= m) per batch."""
    return "".join("S" if len(r) * K + 1 <= d * K else "F" for r in batches)


@functools.lru_cache(maxsize=None)
def oracle_run(kind, method, shape, batch_size, lam=2e-3, max_epoch=6, test=False, loader=None):
    """The oracle's trajectory on shuffled batches of batch_size (perm_of(N)), or on the loader given as a
    tuple of (keyword, value) pairs for O.loader_batches.  Treat the result as read-only."""
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    kw = {}
    if test:
        At, Yt, _ = M.problem(77, d, K, soft=True)
        kw = dict(Atest=At, ytest=Yt)
    om = O.Problem(A, Y, x0, M.oracle_loss(O, kind, d, K, 1.0 / N), lam, **kw)
    if loader is None:
        batches = O.loader_batches(N, batch_size, shuffle_batch=True, perm=perm_of(N))
    else:
        batches = O.loader_batches(N, **dict(loader))
    return O.iterate(OMETHODS[method](), om, "l1", O.PHuberSmootherL1L2(0.5), max_epoch=max_epoch, batches=batches)


# ---- the exact gather: N = 100 rows (no multiple of 16), integer data ------------------------------
GATHER_N = 100
GATHER_D = (1, 127, 128, 129, 260)
GATHER_K = (2, 3, 16)


def gather_lists():
    """Row lists of n_b = 33, 16, 16, 17, 15, 1 rows in the order they are read: row N - 1, a repeated
    row, unsorted lists, two batches of 16 in turn (one pool view gathered twice), smaller batches after
    larger ones."""
    rng = np.random.default_rng(11)
    N = GATHER_N
    b33 = rng.permutation(N)[:33]
    b33[5] = b33[20]                       # a repeated row
    b33[32] = N - 1
    b16a = rng.permutation(N)[:16]
    b16b = np.sort(rng.permutation(N)[:16])[::-1].copy()
    b17 = rng.permutation(N)[:17]
    b15 = rng.permutation(N)[:15]
    b15[0] = b15[14]
    b1 = np.array([N - 1])
    lists = [b33, b16a, b16b, b17, b15, b1]
    assert [len(r) for r in lists] == [33, 16, 16, 17, 15, 1]
    assert any(np.any(np.diff(r) < 0) for r in lists)
    return [np.asarray(r, dtype=np.int64) for r in lists]


def gather_data(d, K, f32):
    """Integer A (±8191: exact in fp32 too) and integer Y."""
    rng = np.random.default_rng(1000 * d + K)
    A = rng.integers(-8191, 8192, size=(GATHER_N, d)).astype(np.float32 if f32 else np.float64)
    Y = rng.integers(-9, 10, size=(GATHER_N, K)).astype(np.float64)
    return A, Y


def gather_all(scsopt, losses, d, K, f32):
    """Every list of gather_lists() read back through get_batch_data, in order, from one context holding
    gather_data(d, K, f32): [(A_b, Y_b), ...] and the references [(A[rows_b], Y[rows_b]), ...]."""
    A, Y = gather_data(d, K, f32)
    lists = gather_lists()
    f, of = M.device_losses(losses, "multi_least_squares", K, 1.0)
    p = scsopt.Problem(A, Y, np.zeros(d * K), f, 1e-3, out_fn=of, dense_f32=f32, multi_batches=True)
    assert p.data_info()[0] == (4 if f32 else 8)
    p.set_batches(lists)
    got = [p.get_batch_data(b) for b in range(len(lists))]
    got.append(p.get_batch_data(1))        # the pool view of 16 rows holds batch 2 now: gathered again
    p.ctx.close()
    A64 = A.astype(np.float64)
    ref = [(A64[r], Y[r]) for r in lists] + [(A64[lists[1]], Y[lists[1]])]
    return got, ref
