"""Shared data of the sparse multi-output tests (test_multi_sparse_host.py, test_gpu_multi_sparse.py):
the problem generator on a sparse A, the integer generator of the exact tests, and the derived bounds
of the softmax system (restated from the dense test: a test module is not imported).

x = vec(X), X d x K column-major; Y is N x K; the losses and closures are tests/multi_output_data.py's."""
import functools
from types import SimpleNamespace

import numpy as np

import multi_output_data as M

EPS = 2.0 ** -52
LIMIT = 1 << 53

# the trajectory shapes (N, d, K) and the exact shapes (N, d) of test_gpu_multi_sparse.py
SHAPES = [(300, 130, 3), (200, 17, 7), (520, 129, 2), (40, 33, 16)]
EXACT_SHAPES = [(1, 1), (65, 1), (700, 300), (300, 4200), (300, 16500), (16500, 300)]
EXACT_K = (2, 3, 16)
PLACEMENT_SHAPES = [(300, 129, 2), (300, 260, 3)]


def sparse_problem(N, d, K, density=0.15, soft=False):
    """(A as scipy CSR, Y, x0), default_rng(31): a Bernoulli(density) mask on randn / √(density·d); row 5
    empty (where N > 5), row N // 3 dense (set after the empty row: at N = 17 both are row 5 and the
    dense row stands), column 3 empty (where d > 3; emptied last, so the dense row skips it).  Labels
    as multi_output_data.problem makes them: one-hot argmax(A W + 0.3·noise), soft: label-smoothed rows
    scaled by a per-sample weight in [0.5, 1.5]; x0 = 0.2·randn (default_rng(5)), not zero."""
    import scipy.sparse as sp
    rng = np.random.default_rng(31)
    A = rng.standard_normal((N, d)) / np.sqrt(density * d)
    A *= rng.random((N, d)) < density
    dense_row = rng.standard_normal(d) / np.sqrt(density * d)
    if N > 5:
        A[5] = 0.0
    A[N // 3] = dense_row
    if d > 3:
        A[:, 3] = 0.0
    W = rng.standard_normal((d, K))
    lab = np.argmax(A @ W + 0.3 * rng.standard_normal((N, K)), axis=1)
    Y = np.eye(K)[lab]
    if soft:
        Y = (0.9 * Y + 0.1 / K) * (0.5 + rng.random((N, 1)))
    x0 = 0.2 * np.random.default_rng(5).standard_normal(d * K)
    return sp.csr_matrix(A), Y, x0


@functools.lru_cache(maxsize=None)
def exact_sparse_case(N, d, K, seed=None):
    """A user matrix in COO form with integer values (exact_data.sparse_case's construction: unsorted
    entries, 200 duplicates, empty rows and columns, one row dense in every block; values in ±4000, so the
    sum of the few duplicates of a position stays far below 2^24 and is exact in fp32), integer X (d x K) and
    V (N x K) in ±1000,
    and the int64 references A X, Aᵀ V.  The dense d x d Gram is not formed.  Asserts Σ|terms| < 2^53:
    every partial sum of any order is then an integer double.  Cached: the arms share one reference."""
    import scipy.sparse as sp
    rng = np.random.default_rng(1000003 * d + 17 * N + K if seed is None else seed)
    nnz = int(0.03 * N * d)
    rows = rng.integers(0, N, nnz)
    cols = rng.integers(0, d, nnz)
    dense_row = N // 3
    ndup = min(200, nnz)
    # ... and one entry in the last row (the ragged tail of the last wave / chunk is not an empty row)
    rows = np.concatenate([rows, np.full(d, dense_row), rows[:ndup], [N - 1]])
    cols = np.concatenate([cols, np.arange(d), cols[:ndup], [0]])
    vals = rng.integers(-4000, 4001, rows.size, dtype=np.int64)
    vals[vals == 0] = 7
    empty_rows = (5, N - 2) if N > 6 else ()
    empty_cols = (20, d - 2) if d > 22 else ()
    keep = ~np.isin(rows, empty_rows) & ~np.isin(cols, empty_cols)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    perm = rng.permutation(rows.size)
    rows, cols, vals = rows[perm], cols[perm], vals[perm]
    coo = sp.coo_matrix((vals.astype(np.float64), (rows, cols)), shape=(N, d))
    Si = sp.coo_matrix((vals, (rows, cols)), shape=(N, d)).tocsr()
    Si.sum_duplicates()
    if ndup:
        assert len(set(zip(rows.tolist(), cols.tolist()))) < rows.size      # duplicates are present
    Xi = rng.integers(-1000, 1001, size=(d, K), dtype=np.int64)
    Vi = rng.integers(-1000, 1001, size=(N, K), dtype=np.int64)
    absS = abs(Si)
    bound = max(int(np.asarray(absS @ np.abs(Xi)).max()), int(np.asarray(absS.T @ np.abs(Vi)).max()))
    assert bound < LIMIT, f"max Σ|terms| = {bound} >= 2^53"
    AX = np.asarray(Si @ Xi)
    ATV = np.asarray(Si.T @ Vi)
    out = SimpleNamespace(N=N, d=d, K=K, coo=coo, S=Si, X=Xi.astype(np.float64), V=Vi.astype(np.float64),
                          AX=AX, ATV=ATV, bound=bound, empty_rows=empty_rows, empty_cols=empty_cols,
                          dense_row=dense_row)
    for a in (out.X, out.V, out.AX, out.ATV):
        a.setflags(write=False)
    return out


def placement_case(N, d, K):
    """Integer sparse A (N x d small: the dense int64 AᵀA is formed), Y in ±5, x in {-1, 0, 1}."""
    c = exact_sparse_case(N, d, K)
    Ai = np.asarray(c.S.todense()).astype(np.int64)
    rng = np.random.default_rng(7 * d + K)
    Y = rng.integers(-5, 6, size=(N, K)).astype(np.float64)
    x = rng.integers(-1, 2, size=d * K).astype(np.float64)
    absA = np.abs(Ai)
    assert int((absA.T @ absA).max()) < LIMIT
    # the residual side: |A X - Y| <= Σ_j |A_ij| + 5, its square summed over N K entries
    rmax = int(absA.sum(axis=1).max()) + 5
    assert N * K * rmax * rmax < LIMIT and int(absA.sum(axis=0).max()) * rmax < LIMIT
    return SimpleNamespace(coo=c.coo, Ai=Ai, Y=Y, x=x, G=(Ai.T @ Ai))


def softmax_bounds(A, Y, X, c):
    """Bounds for f, R, vec(AᵀR) and the system of the softmax loss, derived (not fitted); A dense.
    z: the device sums A X in another order than NumPy: |δz_ik| <= 1e-13·(|A||X|)_ik, the project's
    product bound; τ_i = 2 max_k |δz_ik| + (K + 8) ε covers exp of a shifted logit (argument error |δz|
    twice: the logit and the row maximum; 1 ulp of exp; K additions and one division for P).  So
    |δP_ik| <= P_ik τ_i, |δlog P_ik| <= τ_i + 4 ε |log P_ik|, and
      R = c (s P - Y):           |δR_ik| <= c (s_i P_ik + |Y_ik|) (τ_i + 4 ε)
      f = -c Σ Y log P:          |δf|    <= c Σ |Y_ik| (τ_i + (4 + 2 log2(N K)) ε |log P_ik|)
      g = vec(AᵀR):              |δg_jl| <= 1e-13 (|A|ᵀ|R|)_jl + (|A|ᵀ|δR|)_jl
      w_kl = c s (δ_kl P_k - P_k P_l): |δw| <= w̄_kl (2 τ_i + 6 ε), w̄_kl = c s (δ_kl P_k + P_k P_l)
      G_kl = Aᵀ diag(w_kl) A:    |δG|    <= (1e-13 + 2 τ + 6 ε) |A|ᵀ diag(w̄_kl) |A|, τ = max τ_i
    (1e-13·Σ|terms| is the project's Gram bound).  Returns R, dR, df, dg, τ, P, s."""
    N, K = Y.shape
    Z = A @ X
    absA = np.abs(A)
    dz = 1e-13 * (absA @ np.abs(X))
    tau = 2.0 * dz.max(axis=1) + (K + 8) * EPS
    P = M.probs(Z)
    L = M.log_probs(Z)
    s = Y.sum(axis=1)
    R = c * (s[:, None] * P - Y)
    dR = c * (s[:, None] * P + np.abs(Y)) * (tau[:, None] + 4 * EPS)
    df = c * float(np.sum(np.abs(Y) * (tau[:, None] + (4 + 2 * np.log2(N * K + 1)) * EPS * np.abs(L))))
    dg = 1e-13 * (absA.T @ np.abs(R)) + absA.T @ dR
    return R, dR, df, dg, float(tau.max()), P, s


def system_bound(A, P, s, c, tau, k, l):
    """The bound of block (k, l) of the system (softmax_bounds' last line)."""
    absA = np.abs(A)
    wbar = c * s * ((P[:, k] if k == l else 0.0) + P[:, k] * P[:, l])
    return (1e-13 + 2 * tau + 6 * EPS) * (absA.T @ (wbar[:, None] * absA))
