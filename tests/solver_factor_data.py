"""Deterministic cases for the direct tests of the Cholesky and Householder QR factors
(tests/test_solver_factors_host.py asserts their preconditions with LAPACK on the host,
tests/test_gpu_solver_factors.py holds the device's factors to LAPACK's on them).

Every builder is cached and returns read-only arrays: a case is computed once and shared.

SPD families        M = Q diag(s) Qᵀ symmetrized, s = logspace(0, -dec, n): cond₂ = 10^dec (1 at n = 1).
Pivot placement     an SPD M = UᵀU with M[p, p] -= 1.5 U[p, p]² (pivot p is -0.5 U[p, p]² < 0), or with
                    row and column p zeroed (pivot p is exactly 0): dpotrf's info is p + 1.
QR families         "gauss": Gaussian; "sample": I + Gaussian/√n (the sample-space shape qr(I + A));
                    "negdiag": Gaussian/√n + diag(±3), half of the signs negative (alpha < 0 in many columns).
Exact QR cases      upper triangular A with a mixed-sign diagonal (every tau is 0, R = A), and signed
                    power-of-two-scaled permutations (every intermediate is 0 or one signed power of two, so
                    any summation order gives the same doubles; R from `perm_R` below).
"""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.linalg import lapack

U64 = 2.0 ** -53   # unit roundoff of fp64

CHOL_ORDERS = (1, 2, 15, 16, 17, 127, 128, 129, 257, 511, 512, 513, 640, 1025, 1153)
CHOL_DECS = (2, 6, 10)
CHOL_GRID = tuple((n, dec) for n in CHOL_ORDERS for dec in CHOL_DECS if not (dec == 10 and n < 16))
CHOL_ARMS = (2304, 6)   # 18 blocks: the lookahead's bulk stream runs (the switches' bit-identity case)

INFO_N = 700
INFO_PIVOTS = (0, 15, 16, 127, 128, 143, 511, 512, 699)
INFO_SEMIDEF_P = 300

QR_ORDERS = (1, 2, 5, 127, 128, 129, 255, 257, 300, 1000)
QR_FAMILIES = ("gauss", "sample", "negdiag")
QR_GRID = tuple((fam, n) for fam in QR_FAMILIES for n in QR_ORDERS)
EXACT_ORDERS = (5, 129, 300)

# seeds that replace the default one of a (family, n) case whose draw missed a precondition of the host
# tests (cond₂ <= 1e4, min |R_cc| >= 1e-3 ‖A‖_F / √n): another draw, never a looser number
QR_SEED_OVERRIDE = {}


def gamma(k):
    """γ_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, §3.1)."""
    return k * U64 / (1.0 - k * U64)


def chol_rho_bound(n):
    """Componentwise backward error of a Cholesky factor, |UᵀU - M|_jk <= γ_{3n+1} sqrt(M_jj M_kk)
    (Higham Thm 10.4 with (|Uᵀ||U|)_jk <= sqrt(M_jj M_kk) up to the same γ; the bound
    test_gpu_full_size.py states), plus γ_n for the host's fp64 product UᵀU that measures it."""
    return gamma(3 * n + 1) + gamma(n)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def spd_case(n, dec):
    """M (n x n SPD, cond₂ = 10^dec), a right-hand side b, and cond₂ from M's eigenvalues."""
    rng = np.random.default_rng([n, dec, 20261])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -float(dec), n)
    M = (Q * s) @ Q.T
    M = 0.5 * (M + M.T)
    b = rng.standard_normal(n)
    ev = np.linalg.eigvalsh(M)
    _ro(M, b)
    return SimpleNamespace(n=n, dec=dec, M=M, b=b, cond=float(ev[-1] / ev[0]))


def rho(U, M):
    """max_jk |UᵀU - M|_jk / sqrt(M_jj M_kk)."""
    d = np.sqrt(np.diag(M))
    return float(np.max(np.abs(U.T @ U - M) / np.outer(d, d)))


def eta(M, x, b):
    """Normwise backward error ‖Mx - b‖∞ / (‖M‖∞ ‖x‖∞)."""
    return float(np.linalg.norm(M @ x - b, np.inf) / (np.linalg.norm(M, np.inf) * np.linalg.norm(x, np.inf)))


def lapack_chol(M):
    """dpotrf (upper): (U with a zeroed strict lower triangle, info)."""
    U, info = lapack.dpotrf(M, lower=0, clean=1)
    return U, int(info)


def lapack_chol_solve(U, b):
    x, info = lapack.dpotrs(U, b, lower=0)
    assert info == 0
    return x


@functools.lru_cache(maxsize=None)
def info_case(p):
    """n = INFO_N; p >= 0: the first non-positive pivot is p (negative); p = -1: the semidefinite case,
    row and column INFO_SEMIDEF_P zero (pivot exactly 0)."""
    base = spd_case(INFO_N, 2)
    M = base.M.copy()
    if p < 0:
        M[INFO_SEMIDEF_P, :] = 0.0
        M[:, INFO_SEMIDEF_P] = 0.0
        want = INFO_SEMIDEF_P + 1
    else:
        U, info = lapack_chol(base.M)
        assert info == 0
        M[p, p] -= 1.5 * U[p, p] ** 2
        want = p + 1
    _ro(M)
    return SimpleNamespace(n=INFO_N, M=M, b=base.b, info=want)


@functools.lru_cache(maxsize=None)
def qr_case(family, n):
    seed = QR_SEED_OVERRIDE.get((family, n), 0)
    rng = np.random.default_rng([n, QR_FAMILIES.index(family), seed, 20262])
    G = rng.standard_normal((n, n))
    if family == "gauss":
        A = G
    elif family == "sample":
        A = np.eye(n) + G / np.sqrt(n)
    elif family == "negdiag":
        sg = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)   # n = 1: the one diagonal entry is negative
        A = G / np.sqrt(n) + np.diag(3.0 * rng.permutation(sg))
    else:
        raise ValueError(family)
    A = np.ascontiguousarray(A)
    b = rng.standard_normal(n)
    _ro(A, b)
    return SimpleNamespace(n=n, family=family, A=A, b=b)


def lapack_qr(A):
    """dgeqrf: (the factored array with the reflectors below the diagonal, tau, R)."""
    qr, tau, _, info = lapack.dgeqrf(A)
    assert info == 0
    return qr, tau, np.triu(qr)


def lapack_qr_solve(A, b):
    """x = R⁻¹ Qᵀ b from dgeqrf's factors (dormqr, dtrtrs)."""
    qr, tau, _ = lapack_qr(A)
    c = np.asfortranarray(np.asarray(b, dtype=np.float64).reshape(-1, 1))
    cq, _, info = lapack.dormqr("L", "T", qr, tau, c, max(64 * A.shape[0], 1))
    assert info == 0
    x, info = lapack.dtrtrs(qr, cq, lower=0)
    assert info == 0
    return x[:, 0]


def qr_r_measure(R, A):
    """‖RᵀR - AᵀA‖_F: independent of cond(A) and of Q; with the signs of diag R it pins R (the Cholesky
    factor of AᵀA is unique up to row signs)."""
    return float(np.linalg.norm(R.T @ R - A.T @ A))


@functools.lru_cache(maxsize=None)
def upper_case(n):
    """Upper triangular, small-integer entries, a nonzero diagonal of mixed sign: every column is already
    zero below its diagonal, so every tau is 0 and R = A exactly."""
    rng = np.random.default_rng([n, 20263])
    A = np.triu(rng.integers(-4, 5, size=(n, n)).astype(np.float64))
    d = rng.integers(1, 9, size=n).astype(np.float64) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    d[0] = -abs(d[0])
    d[-1] = abs(d[-1]) if n > 1 else d[-1]
    A[np.arange(n), np.arange(n)] = d
    b = rng.integers(-8, 9, size=n).astype(np.float64)
    _ro(A, b)
    return SimpleNamespace(n=n, A=A, b=b, R=A)


def perm_R(perm, s):
    """R of the Householder QR (dlarfg's conventions) of A with A[perm[j], j] = s[j], all else +0.

    Column c of the running matrix holds one nonzero v at row r >= c.  r = c: x = 0, tau = 0, R_cc = v.
    r > c: alpha = +0, beta = -sign(+0)·|v| = -|v|, tau = 1 and the reflector exchanges rows c and r,
    each times -sign(v): R_cc = -|v|, and the column whose nonzero sat in row c now has it in row r,
    times -sign(v).  R is diagonal; tau is 0 or 1."""
    n = len(perm)
    row = np.array(perm, dtype=np.int64)
    val = np.array(s, dtype=np.float64)
    col_of_row = np.empty(n, dtype=np.int64)
    col_of_row[row] = np.arange(n)
    R = np.zeros(n)
    tau = np.zeros(n)
    for c in range(n):
        r = row[c]
        if r == c:
            R[c] = val[c]
            continue
        R[c] = -abs(val[c])
        tau[c] = 1.0
        q = col_of_row[c]            # its nonzero moves from row c to row r
        val[q] *= -np.sign(val[c])
        row[q] = r
        col_of_row[r] = q
        row[c] = c
        col_of_row[c] = c
    return np.diag(R), tau


@functools.lru_cache(maxsize=None)
def perm_case(n):
    """A signed permutation scaled by powers of two 2^e, e in [-20, 20]; b small integers, so
    x[j] = b[perm[j]] / s[j] exactly."""
    rng = np.random.default_rng([n, 20264])
    # column 0 a fixed point (tau = 0 and R_00 = s[0] > 0, where every beta is < 0); the others one random
    # cycle, so no other column starts on its diagonal
    order = 1 + rng.permutation(n - 1)
    perm = np.zeros(n, dtype=np.int64)
    perm[order] = np.roll(order, -1)
    s =np.ldexp(1.0, rng.integers(-20, 21, size=n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    s[0] = abs(s[0])
    A = np.zeros((n, n))
    A[perm, np.arange(n)] = s
    b = rng.integers(-8, 9, size=n).astype(np.float64)
    b[b == 0.0] = 1.0
    R, tau = perm_R(perm, s)
    x = b[perm] / s
    _ro(A, b, R, tau, x)
    return SimpleNamespace(n=n, A=A, b=b, R=R, tau=tau, x=x, perm=perm, s=s)
