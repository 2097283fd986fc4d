"""The sample-space system of a single-output ProxGGNSCORE step (prox-GGN-SCORE.jl:124-127, N + 1 <= m),
restated in NumPy, with the cases and the error bounds of tests/test_gpu_sample_system.py.  NumPy only:
tests/test_sample_system_host.py checks this file against the oracle without a GPU.

With J = diag(s) A, Q = diag(q), h = 1 ./ Hr, lgr = λ gr, P = A diag(h) Aᵀ and u = A (h ∘ lgr):

    M[i][j] = δ_ij + q_i s_i s_j P_ij      M[i][N] = q_i s_i u_i      M[N][·] = e_N      b = [r; 1]
    M B = b,   d = -h ∘ (Aᵀ (s ∘ B[:N]) + lgr B[N])
"""
import numpy as np

EPS = 2.0 ** -52
PROD = 1e-13          # the project's product bound: |δ Σ terms| <= 1e-13 Σ |terms| (tests/test_gpu_parity.py)

# (N, m): order 2 | one row against a second panel of columns | order 3 | N + 1 = m = 128, no padding of the
# padded order | N + 1 = 128, m one column over a panel | N = 128: the padded order jumps to 256, P keeps 128 |
# the same with a third panel of columns | two P tiles per side | N one short of 256, three column panels |
# the largest trajectory shape
SHAPES = [(1, 2), (1, 130), (2, 3), (127, 128), (127, 129), (128, 129), (128, 300), (129, 130), (255, 257),
          (300, 1000)]
KINDS = ("logistic", "least_squares")
ROUTES = ("dense", "dense_f32", "sparse_sample", "sparse_mirror")
HARD_LAM, HARD_MU = 0.5, 1.0
EASY_LAM, EASY_MU = 1e-3, 1.0


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def huber(x, mu):
    """gr, Hr of PHuberSmootherL1L2(mu) (phuber-smooth.jl:31-36)."""
    t = mu * mu + x * x
    return x * np.power(t, -0.5), (mu * mu) * np.power(t, -1.5)


def parts(kind, A, y, x, c):
    """(s, r, q, z) of prox-GGN-SCORE.jl:44-56 in the closed forms of the loss kinds (J = diag(s) A)."""
    z = A @ x
    if kind == "least_squares":
        n = z.shape[0]
        return np.ones(n), (z - y) * c, np.full(n, c), z
    e = np.exp(-z)
    yh = 1.0 / (1.0 + e)
    s = e / ((1.0 + e) * (1.0 + e))
    r = -c * (y / yh - (1.0 - y) / (1.0 - yh))
    q = c * (y / (yh * yh) + (1.0 - y) / ((1.0 - yh) * (1.0 - yh)))
    return s, r, q, z


def system(A, s, r, q, lgr, Hr):
    """(M, b) of the formula above; M of order N + 1."""
    N = A.shape[0]
    h = 1.0 / Hr
    P = (A * h[None, :]) @ A.T
    u = A @ (h * lgr)
    M = np.zeros((N + 1, N + 1))
    M[:N, :N] = np.eye(N) + q[:, None] * (s[:, None] * s[None, :] * P)
    M[:N, N] = q * (s * u)
    M[N, N] = 1.0
    return M, np.concatenate([r, [1.0]])


def direction(A, s, lgr, Hr, B):
    """d = -h ∘ (Aᵀ (s ∘ B[:N]) + lgr B[N])."""
    N = A.shape[0]
    return -((1.0 / Hr) * (A.T @ (s * B[:N]) + lgr * B[N]))


def system_bounds(kind, A, y, x, c, lgr, Hr):
    """Entrywise bounds (dM, db) on |device - system(...)|, to first order, derived and not fitted.

    ε = 2^-52 is twice the unit roundoff: one ε per elementwise operation covers its rounding on the
    device and in NumPy.  h = 1 ./ Hr and h ∘ lgr are formed from the values handed in by the roundings
    the device applies, so they carry no error.  The three products obey the project's product bound:
      z = A x:            |δz_i|  <= 1e-13 (|A| |x|)_i                       =: dz
      P = A diag(h) Aᵀ:   |δP_ij| <= 1e-13 (|A| diag(h) |A|ᵀ)_ij             =: dp
      u = A (h ∘ lgr):    |δu_i|  <= 1e-13 (|A| |h ∘ lgr|)_i                 =: du
    Least squares: s = 1 and q = c are exact (ρs = ρq = 0); r = (z - y) c has one subtraction and one
    product: |δr| <= c (dz + 2 ε (|z| + |y|)).
    Logistic (e = exp(-z), a = 1 + e, ŷ = 1 / a, w = 1 - ŷ = e / a):
      e:  relative error τ = dz + 2 ε (the argument error, 1 ulp of the device's exp, 1 ulp of libm's)
      a:  (e / a) τ + ε            ŷ:  ρ1 = (e / a) τ + 2 ε
      w:  computed as 1 - ŷ, it inherits ŷ's absolute error: ρ0 = (ŷ / w) ρ1 + ε = ŷ τ + (1 + 2 / e) ε --
          the cancellation at large z, which both sides perform
      s = e / (a a):  ρs = τ + 2 ((e / a) τ + ε) + 2 ε <= 3 τ + 4 ε
      r = -c (t1 - t2), t1 = y / ŷ, t2 = (1 - y) / w:   |δr| <= c (|t1| (ρ1 + 3 ε) + |t2| (ρ0 + 4 ε))
          (a division, for t2 the subtraction 1 - y, then the subtraction and the product with c)
      q = c (y / ŷ² + (1 - y) / w²):                     |δq| <= c (|y| / ŷ² (2 ρ1 + 4 ε) + |1 - y| / w² (2 ρ0 + 5 ε))
    With ρq = |δq| / |q|, the entry M_ij = δ_ij + q_i (s_i s_j P_ij) is a product of four factors with
    three roundings and one addition:
      |δM_ij| <= |q_i s_i s_j| ((|P_ij| + dp_ij) (ρq_i + ρs_i + ρs_j + 3 ε) + dp_ij) + ε (δ_ij + |q_i s_i s_j P_ij|)
      |δM_iN| <= |q_i s_i| ((|u_i| + du_i) (ρq_i + ρs_i + 2 ε) + du_i)
    The last row and b[N] are exact."""
    N = A.shape[0]
    absA = np.abs(A)
    h = 1.0 / Hr
    s, r, q, z = parts(kind, A, y, x, c)
    dz = PROD * (absA @ np.abs(x))
    P = (A * h[None, :]) @ A.T
    dp = PROD * ((absA * h[None, :]) @ absA.T)
    u = A @ (h * lgr)
    du = PROD * (absA @ np.abs(h * lgr))
    if kind == "least_squares":
        rs = np.zeros(N)
        rq = np.zeros(N)
        dr = c * (dz + 2 * EPS * (np.abs(z) + np.abs(y)))
    else:
        e = np.exp(-z)
        a = 1.0 + e
        yh = 1.0 / a
        w = e / a
        tau = dz + 2 * EPS
        rho1 = (e / a) * tau + 2 * EPS
        rho0 = yh * tau + (1.0 + 2.0 / e) * EPS
        rs = 3 * tau + 4 * EPS
        t1, t2 = np.abs(y) / yh, np.abs(1.0 - y) / w
        dr = c * (t1 * (rho1 + 3 * EPS) + t2 * (rho0 + 4 * EPS))
        dq = c * (np.abs(y) / (yh * yh) * (2 * rho1 + 4 * EPS) + np.abs(1.0 - y) / (w * w) * (2 * rho0 + 5 * EPS))
        rq = dq / np.abs(q)
    qss = np.abs(q * s)[:, None] * np.abs(s)[None, :]
    dM = np.zeros((N + 1, N + 1))
    dM[:N, :N] = (qss * ((np.abs(P) + dp) * (rq[:, None] + rs[:, None] + rs[None, :] + 3 * EPS) + dp)
                  + EPS * (np.eye(N) + qss * np.abs(P)))
    dM[:N, N] = np.abs(q * s) * ((np.abs(u) + du) * (rq + rs + 2 * EPS) + du)
    return dM, np.concatenate([dr, [0.0]])


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
class Case:
    """One problem: A, y, x0, the loss scale c, λ and the smoother's μ."""

    def __init__(self, kind, N, m, hard, A, y, x0, c, lam, mu):
        self.kind, self.N, self.m, self.hard = kind, N, m, hard
        self.A, self.y, self.x0, self.c, self.lam, self.mu = A, y, x0, c, lam, mu

    def stored(self, route):
        """The values the route holds: an fp32-stored A is rounded first."""
        if route == "dense_f32":
            return self.A.astype(np.float32).astype(np.float64)
        return self.A

    def system_at(self, x, route="dense", Hr=None, gr=None):
        """(M, b, dM, db, s, lgr, Hr) at x on the route's stored values (gr, Hr: the caller's, or huber's)."""
        A = self.stored(route)
        if Hr is None:
            gr, Hr = huber(x, self.mu)
        lgr = self.lam * gr
        s, r, q, _ = parts(self.kind, A, self.y, x, self.c)
        M, b = system(A, s, r, q, lgr, Hr)
        dM, db = system_bounds(self.kind, A, self.y, x, self.c, lgr, Hr)
        return M, b, dM, db, s, lgr, Hr


# With one or two rows a draw often misses hard_preconditions (a last-column entry >= 1, an interchange at
# N = 2): the first seed shift that meets them, found by running hard_preconditions over 0, 1, 2, ...
_SEED_SHIFT = {("logistic", 1, 2): 3, ("logistic", 1, 130): 4, ("logistic", 2, 3): 3,
               ("least_squares", 1, 2): 4, ("least_squares", 1, 130): 3, ("least_squares", 2, 3): 1}


def _seed(kind, N, m, hard):
    shift = _SEED_SHIFT.get((kind, N, m), 0) if hard else 0
    return 1000003 * N + 101 * m + 7 * KINDS.index(kind) + (3 if hard else 0) + 1009 * shift


def case(kind, N, m, hard):
    """Easy: the trajectory tests' kind -- c = 1/N, rows N(0,1)/√m, x0 ~ 0.3 N(0,1).
    Hard: scale 1, rows N(0, 2²), x0 ~ N(0,1)·0.75/√m, λ = 0.5, PHuberSmootherL1L2(1.0)."""
    rng = np.random.default_rng(_seed(kind, N, m, hard))
    G = rng.standard_normal((N, m))
    g = rng.standard_normal(m)
    if hard:
        A, x0, c, lam, mu = 2.0 * G, g * (0.75 / np.sqrt(m)), 1.0, HARD_LAM, HARD_MU
    else:
        A, x0, c, lam, mu = G / np.sqrt(m), 0.3 * g, 1.0 / N, EASY_LAM, EASY_MU
    if kind == "logistic":
        y = (rng.random(N) < 0.5).astype(np.float64)
    else:
        y = rng.standard_normal(N)
    return Case(kind, N, m, hard, A, y, x0, c, lam, mu)


def interchanges(M):
    """Row interchanges of LAPACK's getrf on M."""
    import scipy.linalg as sla
    _, piv = sla.lu_factor(M)
    return int(np.sum(piv != np.arange(piv.size)))


def hard_preconditions(cs):
    """The figures the hard cases must meet, asserted (the recipe, not the limits, gives way):
    max |A x0| <= 8 (q far from overflow); 1e3 <= cond(M) <= 1e6 for N >= 127; max |M[:N, N]| >= 1; for
    the logistic loss at least one row interchange in getrf -- for N >= 2: the last row of M is e_N, so the
    order-2 system of N = 1 has a zero below its first pivot and cannot interchange.  Returns the figures."""
    assert cs.hard
    M, b, _, _, _, _, _ = cs.system_at(cs.x0)
    zmax = float(np.max(np.abs(cs.A @ cs.x0)))
    cond = float(np.linalg.cond(M))
    last = float(np.max(np.abs(M[:cs.N, cs.N])))
    swaps = interchanges(M)
    assert zmax <= 8.0, (cs.kind, cs.N, cs.m, zmax)
    if cs.N >= 127:
        assert 1e3 <= cond <= 1e6, (cs.kind, cs.N, cs.m, cond)
    assert last >= 1.0, (cs.kind, cs.N, cs.m, last)
    if cs.kind == "logistic" and cs.N >= 2:
        assert swaps >= 1, (cs.kind, cs.N, cs.m, swaps)
    return dict(zmax=zmax, cond=cond, last=last, swaps=swaps, offdiag=float(np.max(np.abs(M - np.eye(cs.N + 1)))))


# ---------------------------------------------------------------------------------------------
# exact placement
# ---------------------------------------------------------------------------------------------
def exact_case(N, m, mu):
    """Least squares at x = 0 with scale 2⁻², integer A in ±8, integer y in ±5, PHuberSmootherL1L2(mu), mu a
    power of two: Hr = 1 / mu exactly and gr = 0, so M = I + 2⁻² mu A Aᵀ, the last column is +0.0 and
    b = [-y / 4; 1], every partial sum an integer multiple of a power of two below 2^53 in any order."""
    rng = np.random.default_rng(977 * N + m)
    Ai = rng.integers(-8, 9, size=(N, m), dtype=np.int64)
    yi = rng.integers(-5, 6, size=N, dtype=np.int64)
    assert mu == 2.0 ** round(np.log2(mu))
    assert int((np.abs(Ai) @ np.abs(Ai).T).max()) * max(mu, 1.0) * 4 < 2 ** 53      # Σ|terms| of P, in units of 2⁻² mu
    M = np.zeros((N + 1, N + 1))
    M[:N, :N] = np.eye(N) + 0.25 * mu * (Ai @ Ai.T).astype(np.float64)
    M[N, N] = 1.0
    b = np.concatenate([(0.0 - yi.astype(np.float64)) * 0.25, [1.0]])     # (z - y) c at z = +0: +0.0 where y = 0
    return Ai.astype(np.float64), yi.astype(np.float64), M, b
