"""Kernel-level edge tests of the length-m / length-N kernels of the SCORE step against the oracle.

csrc/vec.hip (smoothers, prox, get_reg, the SCORE tail, the L-BFGS update, Rosenbrock, the quadratic
loss's Hessian) and the loss epilogue of csrc/data.hip, at the branches, bound vectors and loop
strides the trajectory tests on benign data do not reach.  The reference of every comparison is
oracle/scsopt_oracle.py on identical inputs; the tolerances are the project's (test_gpu_parity.py):

  * prox outputs: bit-exact;
  * smoother grad / hess and the per-sample loss weights: rtol 1e-14 (device exp / pow vs libm);
  * sums of non-negative terms (f, get_reg, the GL smoothers' global dot): rel 1e-13;
  * lock-step steps: x_new rtol 1e-7 / atol 1e-10, pri_res_norm rel 1e-7;
  * trajectories: objective history rtol 1e-8, identical history length and epochs.

Where an output can be non-finite the NaN / +Inf / -Inf masks are compared first, then the finite
entries.  Every test that claims branches counts them on the CPU first (`_need`), so an edit of its
inputs cannot drop coverage unnoticed.
"""
import functools

import numpy as np
import pytest

import scsopt
import scsopt_oracle as O
from scsopt import losses
from scsopt.iterate import init_method, step

pytestmark = pytest.mark.gpu

INF = np.inf
TRIP = 256 * 256          # TAIL_G * TAIL_T: one trip of the multi-workgroup stride loops (vec.hip)
M_TWO_TRIPS = TRIP + 300  # the second trip covers the last 300 coordinates


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _need(**counts):
    """CPU precondition: every named branch / input class occurs at least once."""
    missing = [k for k, v in counts.items() if int(v) <= 0]
    assert not missing, f"inputs no longer reach: {missing} ({counts})"


def assert_same_nonfinite(got, ref):
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    ref = np.atleast_1d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape
    for name, fn in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        bad = np.nonzero(fn(got) != fn(ref))[0]
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], ref[bad[:8]])
    return np.isfinite(ref)


def assert_close_masked(got, ref, rtol, atol=0.0):
    """Identical non-finite masks, then the finite entries at rtol / atol."""
    fin = assert_same_nonfinite(got, ref)
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    ref = np.atleast_1d(np.asarray(ref, dtype=np.float64))
    np.testing.assert_allclose(got[fin], ref[fin], rtol=rtol, atol=atol)
    return fin


def _vec_problem(m, lam=0.3, **kw):
    """A context for the length-m kernels: one all-zero sample, so no data of size N x m matters."""
    return scsopt.Problem(np.zeros((1, m)), np.zeros(1), np.zeros(m), losses.least_squares(1.0), lam, **kw)


def _vec_model(m, lam=0.3, **kw):
    return O.Problem(np.zeros((1, m)), np.zeros(1), np.zeros(m), O.Loss("least_squares"), lam, **kw)


def _lockstep(dm, om_meth, p, om, reg, hm, ohm, nsteps, check=None):
    """Both sides step from the oracle's x (as test_prox_support_pattern_per_step); the project's
    lock-step tolerances.  check(it, x, xn_dev, dx_dev, xn_oracle) adds per-step assertions."""
    p.configure(reg, hm)
    init_method(dm, p)
    om_meth.init(om.x0)
    x = om.x0.copy()
    xp = x.copy()
    for it in range(1, nsteps + 1):
        xn_d, dx_d, pri_d = step(dm, p, reg, hm, x, xp, it, return_dx=True)
        with np.errstate(all="ignore"):
            xn_o, pri_o = O.step(om_meth, om, reg, ohm, x, xp, None, it)
        assert np.all(np.isfinite(xn_o)) and np.isfinite(pri_o)
        err = float(np.max(np.abs(xn_d - xn_o) / (1e-3 + np.abs(xn_o))))   # in units of rtol, atol / rtol = 1e-3
        print(f"step {it}: max |x_dev - x_oracle| / (1e-3 + |x_oracle|) = {err:.3e}, "
              f"pri rel = {abs(pri_d - pri_o) / abs(pri_o):.3e}")
        np.testing.assert_allclose(xn_d, xn_o, rtol=1e-7, atol=1e-10)
        assert pri_d == pytest.approx(pri_o, rel=1e-7)
        if check is not None:
            check(it, x, xn_d, dx_d, xn_o)
        xp, x = x, xn_o


def _eig_ratio(om, ohm, x):
    """|λ|max / |λ|min and λmin of the step's system H + λ·diag(Hr) (prox-N-SCORE.jl:177,204)."""
    M = om.hessx(x) + np.diag(om.lam * ohm.hess(None, x))
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    return float(np.abs(ev).max() / np.abs(ev).min()), float(ev.min())


# ---------------------------------------------------------------------------
# A. loss epilogue, per sample (data.hip: epilogue_kernel)
# ---------------------------------------------------------------------------
_A_CASES = [("logistic_margin", (-1.0, 1.0)), ("logistic_ce", (0.0, 1.0)), ("least_squares", None)]


@pytest.mark.parametrize("kind,labels", _A_CASES, ids=[c[0] for c in _A_CASES])
def test_epilogue_per_sample_gradient_weights(kind, labels):
    """A = I, x = z: gradx(x)[n] is epilogue_kernel's gout[n] itself (every other term of Aᵀg is
    0 * g_k with g_k finite), N = m = 37 so padded rows exist (EPI_GRAD / EPI_VAL of each closed
    form, data.hip epilogue_kernel; the n >= N rows of a partial 16-row / 256-thread block)."""
    N = m = 37
    assert N % 16 != 0 and N % 256 != 0
    z = np.linspace(-30.0, 30.0, N)
    z[17:20] = [-0.5, 0.0, 0.5]
    rng = np.random.default_rng(101)
    if labels is None:
        y = rng.standard_normal(N)
    else:
        y = np.where(np.arange(N) % 2 == 0, labels[0], labels[1])
        y[17:20] = [labels[1], labels[0], labels[1]]
        _need(lo_label=np.sum(y == labels[0]), hi_label=np.sum(y == labels[1]),
              neg_margin=np.sum((z < -20) & (y == labels[1])), pos_margin=np.sum((z > 20) & (y == labels[0])))
    _need(zero=np.sum(z == 0.0), half=np.sum(np.abs(z) == 0.5), far=np.sum(np.abs(z) == 30.0))
    c = 1.0 / N
    A = np.eye(N)
    p = scsopt.Problem(A, y, np.zeros(m), getattr(losses, kind)(c), 1e-3)
    om = O.Problem(A, y, np.zeros(m), O.Loss(kind, c), 1e-3)
    g_ref = om.gradx(z)
    f_ref = om.fx(z)
    assert np.all(np.isfinite(g_ref)) and np.isfinite(f_ref)
    g = p.gradx(z)
    f = p.fx(z)
    print(kind, "max rel grad err", float(np.max(np.abs(g - g_ref) / np.maximum(np.abs(g_ref), 1e-300))),
          "f rel err", abs(f - f_ref) / abs(f_ref))
    np.testing.assert_allclose(g, g_ref, rtol=1e-14, atol=0)
    assert f == pytest.approx(f_ref, rel=1e-13)


_SAT_Z = (30.0, -30.0, 40.0, -40.0, 800.0, -800.0)


def test_epilogue_saturation_parity():
    """The closed forms are the reference's naive ones (log(1 + exp(-y z)), log(1 - ŷ)): past
    1 + e == 1 (|z| ~ 36.7) and past exp overflow (709.78) they give Inf / NaN, and the device must
    give the same non-finite pattern as the oracle (a stable log1p rewrite or a fast-math flag
    would not).  N = m = 1, A = [[1]], x = [z]; ±30 finite, ±40 and ±800 well clear of both
    thresholds, so an ulp of the device exp cannot flip an outcome.  One context per (loss, y)."""
    seen = dict(nan=0, posinf=0, neginf=0, finite=0)
    ce_y1_z40 = None
    for kind, yv in (("logistic_margin", 1.0), ("logistic_margin", -1.0), ("logistic_ce", 0.0), ("logistic_ce", 1.0)):
        A, y = np.array([[1.0]]), np.array([yv])
        p = scsopt.Problem(A, y, np.zeros(1), getattr(losses, kind)(1.0), 1e-3)
        om = O.Problem(A, y, np.zeros(1), O.Loss(kind, 1.0), 1e-3)
        for z in _SAT_Z:
            x = np.array([z])
            with np.errstate(all="ignore"):
                f_ref, g_ref = om.fx(x), om.gradx(x)
            f, g = p.fx(x), p.gradx(x)
            print(f"{kind} y={yv} z={z}: f {f!r} / {f_ref!r}, g {g[0]!r} / {g_ref[0]!r}")
            assert_close_masked(f, f_ref, rtol=1e-13)
            assert_close_masked(g, g_ref, rtol=1e-13)
            for v in (f_ref, g_ref[0]):
                seen["nan"] += int(np.isnan(v))
                seen["posinf"] += int(np.isposinf(v))
                seen["neginf"] += int(np.isneginf(v))
                seen["finite"] += int(np.isfinite(v))
            if kind == "logistic_ce" and yv == 1.0 and z == 40.0:
                ce_y1_z40 = (f, f_ref)
    # the reference's 0 * log(0): ŷ == 1, (1 - y) * log(1 - ŷ) = 0 * -Inf
    assert ce_y1_z40 is not None and np.isnan(ce_y1_z40[1]) and np.isnan(ce_y1_z40[0])
    _need(nan=seen["nan"], inf=seen["posinf"] + seen["neginf"], finite=seen["finite"])


@pytest.mark.parametrize("N,m", [(37, 5), (300, 130)])
def test_nscore_logistic_ce_hessian_weight(N, m):
    """ProxNSCORE on logistic_ce without an out_fn: the EPI_HESS branch of SCS_LOSS_LOGISTIC_CE,
    hout = s*s*q + r*(s*(1 - 2ŷ)) (data.hip epilogue_kernel), which every other test bypasses
    (ProxGGNSCORE takes EPI_GGN).  Three lock-step steps; (300, 130): two column panels, N no
    multiple of 256.  Preconditions on the CPU: the r*s'' term is a visible part of the weight
    (so its sign matters at 1e-7) and the step's system is well conditioned (cond·ε << 1e-7)."""
    rng = np.random.default_rng(7 * N + m)
    A = rng.standard_normal((N, m)) / np.sqrt(m)   # |A x| stays O(1): clear of the saturation of A2
    xt = 3.0 * rng.standard_normal(m)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(A @ xt)))).astype(np.float64)
    x0 = 0.5 * rng.standard_normal(m)
    lam = 1e-3
    _need(y0=np.sum(y == 0.0), y1=np.sum(y == 1.0))
    p = scsopt.Problem(A, y, x0, losses.logistic_ce(1.0 / N), lam)
    om = O.Problem(A, y, x0, O.Loss("logistic_ce", 1.0 / N), lam)
    hm, ohm = scsopt.PHuberSmootherL1L2(1.0), O.PHuberSmootherL1L2(1.0)
    s, yh = O.sigmoid_jac(A @ x0)
    t1 = s * s * O.ce_q(y, yh, 1.0 / N)
    t2 = O.ce_r(y, yh, 1.0 / N) * (s * (1.0 - 2.0 * yh))
    assert np.max(np.abs(t2)) > 1e-2 * np.max(np.abs(t1))
    assert _eig_ratio(om, ohm, x0)[1] > 0.0

    def check(it, x, xn_d, dx_d, xn_o):
        ratio, _ = _eig_ratio(om, ohm, x)
        assert ratio <= 1e5, ratio

    _lockstep(scsopt.ProxNSCORE(), O.ProxNSCORE(), p, om, "l1", hm, ohm, 3, check)


# ---------------------------------------------------------------------------
# B. Rosenbrock (vec.hip: rosen_kernel) and the quadratic loss (half_sym_kernel)
# ---------------------------------------------------------------------------
_ROSEN_M = (3, 7, 1500)
_ROSEN_LAM = 1e-3


def _rosen_x0(m):
    return 1.0 + 0.05 * np.random.default_rng(300 + m).standard_normal(m)


@functools.lru_cache(maxsize=None)
def _rosen_newton_systems(m):
    """(ratio, λmin) of the oracle's ProxNSCORE systems over three steps from _rosen_x0(m)."""
    x0 = _rosen_x0(m)
    om = O.Problem(None, None, x0, O.Loss("rosenbrock"), _ROSEN_LAM)
    ohm = O.PHuberSmootherL1L2(1.0)
    meth = O.ProxNSCORE()
    x, xp, out = x0.copy(), x0.copy(), []
    for it in range(1, 4):
        out.append(_eig_ratio(om, ohm, x))
        xn, _ = O.step(meth, om, "l1", ohm, x, xp, None, it)
        xp, x = x, xn
    return tuple(out)


@pytest.mark.parametrize("m", _ROSEN_M)
def test_rosenbrock_chained_value_and_gradient(m):
    """rosen_kernel what = 0 / 1 in the chained form: the terms i > 0 and i + 1 < m, and for
    m = 1500 the i += VB loop (VB = 1024).  Value: a sum of non-negative terms, rel 1e-13;
    gradient: a three-term sum with cancellation per entry, rtol 1e-13 + 1e-13·max|g|."""
    x0 = _rosen_x0(m)
    _need(interior_terms=m - 2)
    p = scsopt.Problem(x0, losses.rosenbrock(), _ROSEN_LAM)
    f_ref, g_ref = O.rosen_f(x0), O.rosen_grad(x0)
    f, g = p.fx(x0), p.gradx(x0)
    print(m, "f rel", abs(f - f_ref) / abs(f_ref), "g err / max|g|", np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref)))
    assert f == pytest.approx(f_ref, rel=1e-13)
    np.testing.assert_allclose(g, g_ref, rtol=1e-13, atol=1e-13 * float(np.max(np.abs(g_ref))))


@pytest.mark.parametrize("m", _ROSEN_M)
def test_rosenbrock_chained_lqn_lockstep(m):
    """Three lock-step steps of ProxLQNSCORE (memory 3) on the chained Rosenbrock: rosen_kernel's
    gradient inside the step, at x and x_new.  L = 2000 keeps the fixed step (ss_type 1: min(1/L, 1))
    small against the curvature ~1e3, so the iterates stay near x0."""
    x0 = _rosen_x0(m)
    p = scsopt.Problem(x0, losses.rosenbrock(), _ROSEN_LAM, L=2000.0)
    om = O.Problem(None, None, x0, O.Loss("rosenbrock"), _ROSEN_LAM, L=2000.0)
    _lockstep(scsopt.ProxLQNSCORE(m=3), O.ProxLQNSCORE(m=3), p, om, "l1", scsopt.PHuberSmootherL1L2(1.0),
              O.PHuberSmootherL1L2(1.0), 3)


@pytest.mark.parametrize("m", _ROSEN_M)
def test_rosenbrock_chained_nscore_lockstep(m):
    """Three lock-step steps of ProxNSCORE: rosen_kernel what = 2 (the dense tridiagonal Hessian)
    and the m x m solve.  Precondition per step: |λ|max / |λ|min of H + λ·diag(Hr) <= 1e5, so
    cond·ε <= 2e-11 leaves the 1e-7 lock-step tolerance three orders of margin."""
    x0 = _rosen_x0(m)
    for ratio, _ in _rosen_newton_systems(m):
        assert ratio <= 1e5, ratio
    p = scsopt.Problem(x0, losses.rosenbrock(), _ROSEN_LAM)
    om = O.Problem(None, None, x0, O.Loss("rosenbrock"), _ROSEN_LAM)
    _lockstep(scsopt.ProxNSCORE(), O.ProxNSCORE(), p, om, "l1", scsopt.PHuberSmootherL1L2(1.0),
              O.PHuberSmootherL1L2(1.0), 3)


def test_rosenbrock_nscore_cases_reach_both_solver_paths():
    """CPU check of the cases above: among the systems of the three sizes at least one is
    indefinite (the Cholesky reports a pivot, the LU takes over) and at least one is SPD."""
    mins = [lmin for m in _ROSEN_M for _, lmin in _rosen_newton_systems(m)]
    _need(indefinite=sum(v < 0 for v in mins), spd=sum(v > 0 for v in mins))


def test_quadratic_loss_beyond_one_panel():
    """The quadratic loss at m = 200 (two 128-column panels): f, ∇f = ½(A + Aᵀ)x + y with a
    non-symmetric A, and half_sym_kernel's tiled_off(S, i, j) / (S, j, i) across panels inside
    ProxNSCORE (the run of test_reference_indbox, scaled up).  x0 lies outside the box, so the
    first objective is +Inf on both sides."""
    m = 200
    rng = np.random.default_rng(200)
    B = rng.standard_normal((m, m))
    A = B @ B.T / m + np.eye(m) + 0.3 * np.triu(rng.standard_normal((m, m)), 1) / np.sqrt(m)
    y = rng.standard_normal(m)
    x0 = 1.5 * rng.standard_normal(m)
    ev = np.linalg.eigvalsh(0.5 * (A + A.T))
    assert ev.min() > 0.5 and ev.max() / ev.min() < 50.0, (ev.min(), ev.max())
    assert np.max(np.abs(A - A.T)) > 1e-2 and m > 128
    _need(outside=np.sum(np.abs(x0) > 1.0), inside=np.sum(np.abs(x0) < 1.0))
    p = scsopt.Problem(A, y, x0, losses.quadratic(), 1e-4, C_set=[-1.0, 1.0])
    om = O.Problem(A, y, x0, O.Loss("quadratic"), 1e-4, C_set=[-1.0, 1.0])
    f_terms = 0.5 * float(np.abs(x0) @ (np.abs(A) @ np.abs(x0))) + float(np.abs(y) @ np.abs(x0))
    assert abs(p.fx(x0) - om.fx(x0)) <= 1e-13 * f_terms
    g_terms = 0.5 * (np.abs(A) @ np.abs(x0) + np.abs(A).T @ np.abs(x0)) + np.abs(y)
    assert np.all(np.abs(p.gradx(x0) - om.gradx(x0)) <= 1e-13 * g_terms)
    sol = scsopt.iterate(scsopt.ProxNSCORE(), p, "indbox", scsopt.PHuberSmootherIndBox(-1.0, 1.0, 0.6), alpha=0.8,
                         max_epoch=6, verbose=0)
    osol = O.iterate(O.ProxNSCORE(), om, "indbox", O.PHuberSmootherIndBox(-1.0, 1.0, 0.6), alpha=0.8, max_epoch=6)
    assert np.isposinf(osol.obj[0])
    assert sol.epochs == osol.epochs and len(sol.obj) == len(osol.obj)
    assert_close_masked(sol.obj, osol.obj, rtol=1e-8)
    np.testing.assert_allclose(sol.fval, osol.fval, rtol=1e-8)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-7, atol=1e-12)


@pytest.mark.parametrize("how", ["quadratic", "callback"])
def test_nscore_indefinite_hessian_in_leading_block(how):
    """The Hessians written straight into the leading m x m block of the padded system (the
    quadratic loss's half_sym_kernel, a callback's hess_fx; rosen_kernel above is the third) with an
    indefinite H: the Cholesky meets a non-positive pivot, runs on through NaN and the LU solves the
    copy; the padded columns it left NaN must not reach the next step's system (they did: every step
    after the first returned NaN).  m = 130: two panels, 126 padded rows / columns.  Three
    lock-step steps on one context."""
    m = 130
    rng = np.random.default_rng(130)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    d = np.where(np.arange(m) % 3 == 0, -1.0, 1.0) * rng.uniform(1.0, 3.0, m)
    H = Q @ (d[:, None] * Q.T)
    H = 0.5 * (H + H.T)
    y = rng.standard_normal(m)
    x0 = 0.5 * rng.standard_normal(m)
    lam = 1e-3
    ev = np.linalg.eigvalsh(H)
    _need(negative=np.sum(ev < 0), positive=np.sum(ev > 0), padded=(-m) % 128)
    hm, ohm = scsopt.PHuberSmootherL1L2(1.0), O.PHuberSmootherL1L2(1.0)
    if how == "quadratic":
        K = np.triu(rng.standard_normal((m, m)), 1) / np.sqrt(m)
        A = H + 0.3 * (K - K.T)                    # non-symmetric, symmetric part H
        p = scsopt.Problem(A, y, x0, losses.quadratic(), lam)
        om = O.Problem(A, y, x0, O.Loss("quadratic"), lam)
    else:
        fn = (lambda x: 0.5 * float(x @ (H @ x)) + float(y @ x), lambda x: H @ x + y, lambda x: H)
        p = scsopt.Problem(x0, losses.callback(*fn), lam)
        om = O.Problem(None, None, x0, O.CallbackLoss(*fn), lam)

    def check(it, x, xn_d, dx_d, xn_o):
        ratio, lmin = _eig_ratio(om, ohm, x)
        assert ratio <= 1e5 and lmin < 0, (ratio, lmin)

    _lockstep(scsopt.ProxNSCORE(), O.ProxNSCORE(), p, om, "l1", hm, ohm, 3, check)


# ---------------------------------------------------------------------------
# C. smoothers at branch edges, per-coordinate and infinite bounds, sizes (smooth_elem_kernel,
#    smooth_gl_kernel; scs_set_smoother's upload_bounds: ±Inf -> ∓1e32)
# ---------------------------------------------------------------------------
BOX_MU = 0.6
_BOX_LB = (-2.0, -1.0, -0.5, 0.0, 0.25, 0.5)
_BOX_W = (1.0, 2.0, 3.0, INF)
# ub = lb + width for a finite lb; for lb = -Inf the upper bounds are listed (-Inf + Inf is a NaN bound)
_BOX_COMBOS = tuple((a, a + w) for a in _BOX_LB for w in _BOX_W) + tuple((-INF, b) for b in (-1.0, 0.5, 3.0, INF))

# (lb, ub, x): twelve hand-picked coordinates that reach every branch, so that m = 12 does too
_BOX_HEAD = (
    (-2.0, -1.0, -3.0),        # below the box with -x < a false: the reference's eps() branch
    (-2.0, 1.0, 2.5),          # above, -x < a true
    (0.25, 1.25, -1.0),        # below, -x < a false
    (0.25, 3.25, 1.0),         # inside, -x < a true; neither LogExp edge
    (-2.0, 1.0, 1.5),          # above, -x < a false: the b branch of the gradient
    (-0.5, 0.5, -0.5),         # x == a
    (-1.0, 2.0, 2.0),          # x == b
    (-INF, 0.5, 0.0),          # infinite lower bound, +0
    (0.0, INF, -0.0),          # infinite upper bound, -0 == a
    (-INF, INF, 7.0),          # both infinite
    (-1.0, 2.0, -1.0 + BOX_MU),  # x == a + μ
    (-1.0, 2.0, 2.0 - BOX_MU),   # x == b - μ
)


def _sanitized(lb, ub):
    return np.where(lb == -INF, O.L_INF_CACHE, lb), np.where(ub == INF, O.U_INF_CACHE, ub)


def _box_points(a, b, mu):
    """The x values of one coordinate with raw bounds (a, b): at, next to and across every edge."""
    sa = O.L_INF_CACHE if a == -INF else a
    sb = O.U_INF_CACHE if b == INF else b
    if np.isfinite(a) and np.isfinite(b):
        inside = 0.5 * (a + b)
    elif np.isfinite(a):
        inside = a + 1.5
    elif np.isfinite(b):
        inside = b - 1.5
    else:
        inside = 0.3
    return [sa, sb, np.nextafter(sa, -INF), np.nextafter(sa, INF), np.nextafter(sb, -INF), np.nextafter(sb, INF),
            sa + mu, sb - mu, np.nextafter(sa + mu, INF), np.nextafter(sb - mu, -INF), inside, sa - 0.7, sb + 0.7,
            -sa, -sa + 0.125, -sa - 0.125, 0.0, -0.0]


@functools.lru_cache(maxsize=None)
def _box_inputs(m):
    """(lb, ub, x) of length m: the head, then the edge block of every bounds pair tiled (in a fixed
    shuffled order, so a partial tile is still a mixed sample), the rest random."""
    rng = np.random.default_rng(4242)
    blk = [(a, b, xv) for a, b in _BOX_COMBOS for xv in _box_points(a, b, BOX_MU)]
    blk = [blk[i] for i in rng.permutation(len(blk))]
    rows = list(_BOX_HEAD) + blk
    ntile = max(1, m // len(rows))
    rows = (rows * ntile)[:m]
    lb = np.array([r[0] for r in rows])
    ub = np.array([r[1] for r in rows])
    x = np.array([r[2] for r in rows])
    rest = m - len(rows)
    if rest > 0:
        pick = rng.integers(0, len(_BOX_COMBOS), rest)
        lb = np.concatenate([lb, [_BOX_COMBOS[k][0] for k in pick]])
        ub = np.concatenate([ub, [_BOX_COMBOS[k][1] for k in pick]])
        x = np.concatenate([x, rng.uniform(-4.0, 4.0, rest)])
    assert lb.shape == ub.shape == x.shape == (m,)
    assert not np.any(np.isnan(lb)) and not np.any(np.isnan(ub)) and np.all(lb < ub)
    for v in (lb, ub, x):
        v.setflags(write=False)
    return lb, ub, x


def _box_branch_counts(lb, ub, x, mu):
    a, b = _sanitized(lb, ub)
    g1 = -x < a
    g2 = ~g1 & ((x == a) | (x < b))
    c = dict(
        grad_a=np.sum(g1), grad_eps=np.sum(g2), grad_b=np.sum(~g1 & ~g2),
        negx_lt_a_while_x_gt_a=np.sum(g1 & (x > a)), negx_ge_a_while_x_lt_a=np.sum(~g1 & (x < a)),
        hess_a=np.sum(x <= a), hess_eps=np.sum((a < x) & (x < b)), hess_b=np.sum(x >= b),
        logexp_q_a=np.sum(x <= a + mu), logexp_q_b=np.sum(~(x <= a + mu) & (x >= b - mu)),
        logexp_q_none=np.sum(~(x <= a + mu) & ~(x >= b - mu)),
        logexp_l_a=np.sum(x < a), logexp_l_b=np.sum(~(x < a) & (x > b)), logexp_l_none=np.sum((x >= a) & (x <= b)),
        at_a=np.sum(x == a), at_b=np.sum(x == b), at_a_plus_mu=np.sum(x == a + mu), at_b_minus_mu=np.sum(x == b - mu),
        lb_inf=np.sum(lb == -INF), ub_inf=np.sum(ub == INF), pos_zero=np.sum((x == 0) & ~np.signbit(x)),
        neg_zero=np.sum((x == 0) & np.signbit(x)), distinct_lb=len(set(lb.tolist())) - 1,
        distinct_ub=len(set(ub.tolist())) - 1, asymmetric=np.sum(lb != -ub))
    return c


@pytest.mark.parametrize("m", [12, 257, 16385])
@pytest.mark.parametrize("kind", ["phuber_indbox", "logexp_indbox", "exp_indbox"])
def test_box_smoothers_vector_bounds(kind, m):
    """smooth_elem_kernel's three box kinds with length-m, asymmetric and partly infinite bound
    vectors (a[i] / b[i] per coordinate; ±Inf -> ∓1e32 in upload_bounds), x at and one ulp beside
    a, b, a + μ, b - μ, inside, below, above, on both sides of the reference's `-x < a` test
    (phuber-smooth.jl:83-98) and at ±0.  m = 12: less than a wave; 257: a second workgroup of one
    thread; 16385: 65 workgroups.  The exact branch values eps() and ±0 match bitwise."""
    lb, ub, x = _box_inputs(m)
    counts = _box_branch_counts(lb, ub, x, BOX_MU)
    _need(**counts)
    if m > 12:
        a, b = _sanitized(lb, ub)
        _need(ulp_below_a=np.sum(x == np.nextafter(a, -INF)), ulp_above_a=np.sum(x == np.nextafter(a, INF)),
              ulp_below_b=np.sum(x == np.nextafter(b, -INF)), ulp_above_b=np.sum(x == np.nextafter(b, INF)))
    ctor = {"phuber_indbox": "PHuberSmootherIndBox", "logexp_indbox": "LogExpSmootherIndBox",
            "exp_indbox": "ExponentialSmootherIndBox"}[kind]
    hm, ohm = getattr(scsopt, ctor)(lb, ub, BOX_MU), getattr(O, ctor)(lb, ub, BOX_MU)
    p = _vec_problem(m, C_set=[lb, ub])
    p.configure("indbox", hm)
    with np.errstate(all="ignore"):
        g_ref, h_ref = ohm.grad(None, x), ohm.hess(None, x)
    gr, Hr = p._smoother_eval(hm, x)
    for name, got, ref in (("grad", gr, g_ref), ("hess", Hr, h_ref)):
        fin = assert_close_masked(got, ref, rtol=1e-14, atol=1e-300)
        sel = fin & ((ref == O.EPS) | (ref == 0.0))
        assert np.array_equal(bits(got[sel]), bits(ref[sel])), (name, np.nonzero(bits(got) != bits(ref))[0][:8])
    if kind == "phuber_indbox":
        _need(eps_values=np.sum(g_ref == O.EPS))
        if m > 12:   # x at the sanitized -1e32 itself: the quadratic cancels to 0, pow(0, -1.5) = Inf
            _need(nonfinite_hess=np.sum(~np.isfinite(h_ref)))


@pytest.mark.parametrize("kind", ["phuber_l1l2", "osba_l1l2"])
def test_l1l2_smoothers_scale_extremes(kind):
    """smooth_elem_kernel's two bound-free kinds at m = 1025 (a fifth workgroup of one thread) over
    |x| from 1e-160 to 1e150: underflow of x², overflow of x⁵, and for Ostrovskii-Bach the 0/0 at
    x = 0 (one entry: NaN on both sides, as the reference gives)."""
    m = 1025
    rng = np.random.default_rng(1025)
    x = rng.standard_normal(m)
    x = np.where(np.abs(x) < 1e-3, 0.25, x)
    ext = np.array([s * v for v in (1e-160, 1e-8, 1.0, 1e8, 1e150) for s in (1.0, -1.0)])
    x[:ext.size] = ext
    if kind == "osba_l1l2":
        x[ext.size] = 0.0
        hm, ohm = scsopt.OsBaSmootherL1L2(0.4), O.OsBaSmootherL1L2(0.4)
        _need(zeros=np.sum(x == 0.0))
        assert np.sum(x == 0.0) == 1
    else:
        x[ext.size:ext.size + 2] = [0.0, -0.0]
        hm, ohm = scsopt.PHuberSmootherL1L2(0.3), O.PHuberSmootherL1L2(0.3)
    _need(tiny=np.sum(np.abs(x) == 1e-160), huge=np.sum(np.abs(x) == 1e150), neg=np.sum(x < 0), pos=np.sum(x > 0))
    p = _vec_problem(m)
    p.configure("l1", hm)
    with np.errstate(all="ignore"):
        g_ref, h_ref = ohm.grad(None, x), ohm.hess(None, x)
    gr, Hr = p._smoother_eval(hm, x)
    assert_close_masked(gr, g_ref, rtol=1e-14, atol=1e-300)
    assert_close_masked(Hr, h_ref, rtol=1e-14, atol=1e-300)
    if kind == "osba_l1l2":
        k = ext.size
        assert np.isnan(g_ref[k]) and np.isnan(h_ref[k]) and np.isnan(gr[k]) and np.isnan(Hr[k])


def _ragged_groups(m, rng):
    """3 x G ind (1-based start, end, Int weight 1..3) of ragged groups listed out of order, one of
    them of size 1 (built as in test_group_lasso_general_groups), and a permuted G."""
    if m == 1:
        cuts = [0, 1]
    else:
        inner = rng.choice(np.arange(2, m), size=min(max(m // 50, 1), m - 2), replace=False) if m > 2 else []
        cuts = sorted(set([0, 1, m] + [int(c) for c in inner]))   # [0, 1): the size-1 group
    groups = [(cuts[i] + 1, cuts[i + 1], 1 + i % 3) for i in range(len(cuts) - 1)]
    order = rng.permutation(len(groups))
    ind = np.array([[groups[g][0] for g in order], [groups[g][1] for g in order], [groups[g][2] for g in order]])
    return ind, rng.permutation(m) + 1


def _need_ragged(ind, m):
    sizes = ind[1] - ind[0] + 1
    if m > 1:
        _need(groups=ind.shape[1] - 1, ragged=len(set(sizes.tolist())) - 1, out_of_order=np.sum(np.diff(ind[0]) < 0),
              weights=len(set(ind[2].tolist())) - 2)
    _need(size_one=np.sum(sizes == 1))
    assert int(sizes.sum()) == m


@pytest.mark.parametrize("m", [1, 1025, 5000])
@pytest.mark.parametrize("kind", ["phuber_gl", "osba_gl"])
def test_gl_smoothers_past_one_pass(kind, m):
    """smooth_gl_kernel<false> / <true> (one workgroup of 1024 threads) at m = 1, one element past one
    pass (1025) and five passes (5000), with ragged groups listed out of order, Int weights 1..3
    and a group of size 1.  grad: rtol 1e-14.  hess: rtol 1e-13 -- it carries the global dot
    Σ Dg² (non-negative terms: the device's order and NumPy's are each within (⌈log₂ m⌉ + 2)·2⁻⁵³
    relative) and pow's 2 ulp through two compositions; 1e-13 leaves more than 20x margin.

    osba_gl runs at |x| >= 1 (μ = 0.5).  Nearer to 0 the input is ill-posed for a comparison of two
    libms: osba_val(x) is a difference of O(μ) terms, two of them logs, and osba_grad(w·val) cancels
    μ³-sized terms down to O(val⁴), so the rounding of that evaluation is a different draw for every
    input bit pattern.  Moving each log of osba_val by one ulp (NumPy, on the CPU) moves the
    reference's own gradient by 1.8e-7 relative at |x| in [0.05, 0.075], 7e-10 at 0.1, 1.8e-13 at
    0.3, 9e-15 at 0.5 and 1.6e-15 from 1.0 on; the device at |x| >= 0.05 differed from the oracle by
    1.5e-13 (m = 1025) and 1.5e-9 (m = 5000) in under 1 % of the entries, all others within 1e-14."""
    rng = np.random.default_rng(50 + m)
    ind, G = _ragged_groups(m, rng)
    _need_ragged(ind, m)
    x = rng.standard_normal(m)
    osba = kind == "osba_gl"
    if osba:   # away from 0 by 1.0: see the docstring (and 0/0 at x = 0 would poison the global dot)
        x = np.where(x < 0, -1.0, 1.0) * (1.0 + 0.8 * np.abs(x))
        if m > 1:
            _need(neg=np.sum(x < 0), pos=np.sum(x > 0))
    elif m > 1:
        x[m // 2] = 0.0
    p = _vec_problem(m, lam=[1e-3, 0.1], P=scsopt.get_P(m, G, ind))
    hm = scsopt.OsBaSmootherGL(0.5, p) if osba else scsopt.PHuberSmootherGL(0.5, p)
    p.configure("gl", hm)
    ohm = O.Smoother(kind, 0.5, *((O.OSBA_MH, O.OSBA_NU) if osba else (O.HUBER_MH, O.HUBER_NU)),
                     P=O.GroupP(m, ind, G))
    g_ref, h_ref = ohm.grad(None, x), ohm.hess(None, x)
    assert np.all(np.isfinite(g_ref)) and np.all(np.isfinite(h_ref))
    gr, Hr = p._smoother_eval(hm, x)
    print(kind, m, "grad", np.max(np.abs(gr - g_ref) / np.maximum(np.abs(g_ref), 1e-300)),
          "hess", np.max(np.abs(Hr - h_ref) / np.maximum(np.abs(h_ref), 1e-300)))
    np.testing.assert_allclose(gr, g_ref, rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(Hr, h_ref, rtol=1e-13, atol=1e-300)


# ---------------------------------------------------------------------------
# D. prox and get_reg, direct (prox_only_kernel / prox_block; reg_value_kernel, reg_part_kernel)
# ---------------------------------------------------------------------------
PROX_LAM, PROX_ALPHA = 0.5, 0.5   # α·λ = 0.25 exactly: with Hr = 1 the threshold t is 0.25 exactly


def _prox_inputs(m, reg):
    """(z, Hr): random values, then -- as far as m has room -- z exactly at the threshold (first,
    so m = 1 gets it), one ulp either side of it, ±0, ±1e-300 and far values."""
    rng = np.random.default_rng(900 + m)
    Hr = np.abs(rng.standard_normal(m)) + 0.05
    z = rng.standard_normal(m) * 0.8
    Hr[:2] = 1.0
    t = (PROX_ALPHA * PROX_LAM) / (1.0 / Hr)
    edge = t if reg == "l1" else np.sqrt(t)   # l1: |z| = t; l2: z² = t
    vals = [lambda k: edge[k], lambda k: -edge[k],
            lambda k: np.nextafter(edge[k], INF), lambda k: np.nextafter(edge[k], 0.0),
            lambda k: -np.nextafter(edge[k], INF), lambda k: -np.nextafter(edge[k], 0.0),
            lambda k: 0.0, lambda k: -0.0, lambda k: 1e-300, lambda k: -1e-300, lambda k: 2.0, lambda k: -2.0,
            lambda k: edge[k] * 0.5, lambda k: -edge[k] * 1.5]
    for k, fn in enumerate(vals[:m]):
        z[k] = fn(k)
    return z, Hr, t


@pytest.mark.parametrize("m", [1, 1025, 20001])
@pytest.mark.parametrize("reg", ["l1", "l2", "indbox"])
def test_prox_bit_exact_at_sizes(reg, m):
    """prox_only_kernel / prox_block (one workgroup, i += 1024) at one element, one element past a
    pass and 20 passes: bit-exact against the oracle (IEEE +,-,*,/ only), z at the threshold and
    one ulp either side, ±0, ±1e-300; indbox with per-coordinate bounds that include raw ±Inf
    (the prox and get_reg read C_set unsanitized)."""
    if reg == "indbox":
        lb, ub, z = _box_inputs(m)
        Hr = np.ones(m)
        if m > 1:
            _need(lb_inf=np.sum(lb == -INF), ub_inf=np.sum(ub == INF), below=np.sum(z < lb), above=np.sum(z > ub),
                  inside=np.sum((z > lb) & (z < ub)), at_lb=np.sum(z == lb), at_ub=np.sum(z == ub),
                  neg_zero_at_zero_lb=np.sum((z == 0) & np.signbit(z) & (lb == 0.0)))
        p = _vec_problem(m, C_set=[lb, ub])
        p.configure("indbox", scsopt.PHuberSmootherIndBox(lb, ub, BOX_MU))
        ref = O.prox_indbox(_vec_model(m, C_set=[lb, ub]), z)
    else:
        z, Hr, t = _prox_inputs(m, reg)
        with np.errstate(all="ignore"):
            ratio = t / np.abs(z) if reg == "l1" else t / (z * z)
        _need(at_threshold=np.sum(ratio == 1.0))
        if m > 1:
            _need(shrunk_to_zero=np.sum(ratio > 1.0), kept=np.sum(ratio < 1.0), zeros=np.sum(z == 0.0),
                  neg_zero=np.sum((z == 0) & np.signbit(z)), tiny=np.sum(np.abs(z) == 1e-300))
        p = _vec_problem(m)
        p.configure(reg, scsopt.PHuberSmootherL1L2(1.0))
        with np.errstate(all="ignore"):
            ref = (O.prox_l1 if reg == "l1" else O.prox_l2)(z, 1.0 / Hr, PROX_LAM, PROX_ALPHA)
    assert not np.any(np.isnan(ref))
    got = p.prox(z, Hr, PROX_LAM, PROX_ALPHA)
    assert np.array_equal(bits(got), bits(ref)), np.nonzero(bits(got) != bits(ref))[0][:8]


@pytest.mark.parametrize("m", [1, 3000])
def test_prox_gl_bit_exact_at_sizes(m):
    """prox_block's gl branch (soft threshold, then one thread per group) at m = 1 and 3000: ragged
    out-of-order weighted groups, a group of size 1, and a group the soft threshold zeroes
    entirely (‖·‖ = 0: β/(h·0) = Inf, max(1 - Inf, 0) = 0, the entries stay ±0)."""
    rng = np.random.default_rng(70 + m)
    ind, G = _ragged_groups(m, rng)
    _need_ragged(ind, m)
    z, Hr, t = _prox_inputs(m, "l1")
    t = PROX_LAM / (1.0 / Hr)                   # gl's soft threshold carries no α
    sizes = ind[1] - ind[0] + 1
    g0 = int(np.argmax(sizes))                  # the largest group: every entry below its threshold
    seg = slice(int(ind[0, g0]) - 1, int(ind[1, g0]))
    z[seg] = 0.5 * t[seg] * np.where(np.arange(seg.stop - seg.start) % 2 == 0, 1.0, -1.0)
    if m == 1:
        z[0] = t[0]                             # at the threshold: zeroed as well
    soft = np.abs(z) - t
    zeroed = [bool(np.all(soft[int(s) - 1:int(e)] <= 0)) for s, e in zip(ind[0], ind[1])]
    _need(zeroed_groups=sum(zeroed))
    if m > 1:
        _need(live_groups=len(zeroed) - sum(zeroed), zeroed_group_size=sizes[g0] - 1)
    lam = [PROX_LAM, 0.2]
    p = _vec_problem(m, lam=lam, P=scsopt.get_P(m, G, ind))
    p.configure("gl", scsopt.PHuberSmootherL1L2(1.0))
    model = _vec_model(m, lam=lam, P=O.GroupP(m, ind, G))
    with np.errstate(all="ignore"):
        ref = O.prox_gl(model, z, 1.0 / Hr, PROX_ALPHA)
    assert not np.any(np.isnan(ref)) and np.all(ref[seg] == 0.0)
    got = p.prox(z, Hr, PROX_LAM, PROX_ALPHA)
    assert np.array_equal(bits(got), bits(ref)), np.nonzero(bits(got) != bits(ref))[0][:8]


_REG_M = (1, 1000, 16383, 16384, M_TWO_TRIPS)


@pytest.mark.parametrize("m", _REG_M)
@pytest.mark.parametrize("reg", ["l1", "l2"])
def test_get_reg_l1_l2_sizes(reg, m):
    """get_reg for l1 / l2: reg_value_kernel (m < 16384) and reg_part_kernel + reg_final_kernel
    (m >= 16384), either side of the dispatch, and m = 65536 + 300: the second trip of
    i += TAIL_G*TAIL_T.  Sums of non-negative terms: rel 1e-13.  The last 300 entries carry a
    visible part of the sum, so a loop that stopped after one trip fails."""
    rng = np.random.default_rng(m)
    x = rng.standard_normal(m)
    if m > TRIP:
        x[TRIP:] *= 40.0
        tail = np.sum(np.abs(x[TRIP:])) / np.sum(np.abs(x))
        assert tail > 1e-2, tail
    lam = 0.3
    p = _vec_problem(m, lam=lam)
    p.configure(reg, scsopt.PHuberSmootherL1L2(1.0))
    ref = O.get_reg(_vec_model(m, lam=lam), x, reg)
    got = p.get_reg(x)
    print(reg, m, "rel err", abs(got - ref) / ref)
    assert got == pytest.approx(ref, rel=1e-13)


@pytest.mark.parametrize("m", _REG_M)
def test_get_reg_indbox_single_violation(m):
    """get_reg for indbox with per-coordinate bounds (raw ±Inf included): 0.0 with every coordinate
    inside or exactly on a bound, +Inf with exactly one coordinate outside -- below its lb or
    above its ub -- at index 0, 16383 and m - 1 (the last element of the second trip decides)."""
    lb0, ub0, _ = _box_inputs(min(m, 600))
    reps = -(-m // lb0.size)
    lb, ub = np.tile(lb0, reps)[:m], np.tile(ub0, reps)[:m]
    targets = sorted(k for k in {0, 16383, m - 1} if k < m)
    lb[targets], ub[targets] = -0.5, 0.75       # finite on both sides, so each can be violated
    a, b = _sanitized(lb, ub)
    rng = np.random.default_rng(m + 5)
    x = a + (b - a) * rng.uniform(0.05, 0.95, m)
    k = np.arange(m)
    x = np.where(k % 7 == 1, a, np.where(k % 7 == 2, b, x))   # exactly on a bound: not a violation
    x = np.where((lb == -INF) & (k % 7 == 1), -1e300, np.where((ub == INF) & (k % 7 == 2), 1e300, x))
    assert np.all(x >= lb) and np.all(x <= ub)
    if m > 7:
        _need(on_lb=np.sum(x == lb), on_ub=np.sum(x == ub), lb_inf=np.sum(lb == -INF), ub_inf=np.sum(ub == INF))
    p = _vec_problem(m, C_set=[lb, ub])
    p.configure("indbox", scsopt.PHuberSmootherIndBox(lb, ub, BOX_MU))
    model = _vec_model(m, C_set=[lb, ub])
    assert O.get_reg(model, x, "indbox") == 0.0
    assert p.get_reg(x) == 0.0
    tried = 0
    for idx in targets:
        for side in ("below", "above"):
            bound = lb[idx] if side == "below" else ub[idx]
            xv = x.copy()
            xv[idx] = np.nextafter(bound, -INF if side == "below" else INF)
            assert int(np.sum((xv < lb) | (xv > ub))) == 1
            assert O.get_reg(model, xv, "indbox") == INF
            got = p.get_reg(xv)
            assert got == INF, (idx, side, got)
            tried += 1
    assert tried == 2 * len(targets)


# ---------------------------------------------------------------------------
# E. SCORE tail, two-loop and memory update past 65536 (tail_eta / tail_apply / tail_pri,
#    lbfgs_update_part, tl_*, reg_part, norms_part; the fused lqn_tail / lqn_post)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_data(m):
    N = 64
    rng = np.random.default_rng(12)
    A = rng.standard_normal((N, m)) / np.sqrt(m)
    y = rng.standard_normal(N)
    x0 = rng.standard_normal(m) * 0.1
    for v in (A, y, x0):
        v.setflags(write=False)
    return N, A, y, x0


def _tail_pair(m, reg):
    N, A, y, x0 = _tail_data(m)
    C_set = [-0.05, 0.05] if reg == "indbox" else None
    p = scsopt.Problem(A, y, x0, losses.least_squares(1.0 / N), 1e-4, C_set=C_set)
    om = O.Problem(A, y, x0.copy(), O.Loss("least_squares", 1.0 / N), 1e-4, C_set=C_set)
    if reg == "indbox":
        hm, ohm = scsopt.PHuberSmootherIndBox(-0.05, 0.05, 0.5), O.PHuberSmootherIndBox(-0.05, 0.05, 0.5)
    else:
        hm, ohm = scsopt.PHuberSmootherL1L2(0.5), O.PHuberSmootherL1L2(0.5)
    return p, om, hm, ohm


@pytest.mark.parametrize("reg,use_prox,m", [("l1", True, M_TWO_TRIPS), ("indbox", True, M_TWO_TRIPS),
                                            ("l2", False, M_TWO_TRIPS), ("l1", True, 16383), ("l1", True, 16384)])
def test_lqn_lockstep_past_one_stride_trip(reg, use_prox, m):
    """Four lock-step steps of ProxLQNSCORE (memory 3: the two-loop and the ring are active from
    step 2) at m = 65536 + 300, where tail_eta / tail_apply, lbfgs_update_part and the tl_* kernels
    make a second trip of their 65536-element stride; l1 also at m = 16383 / 16384, either side of
    the one-workgroup / multi-workgroup dispatch.  The last 300 coordinates are compared on their
    own as well: a kernel that stopped after one trip would leave them stale, and the oracle's step
    moves them (asserted)."""
    p, om, hm, ohm = _tail_pair(m, reg)
    tail = slice(TRIP, None) if m > TRIP else slice(m - 300, None)

    def check(it, x, xn_d, dx_d, xn_o):
        moved = np.abs(xn_o[tail] - x[tail]) > 1e-5 * np.abs(x[tail])
        _need(tail_coordinates_that_move=np.sum(moved))
        np.testing.assert_allclose(xn_d[tail], xn_o[tail], rtol=1e-7, atol=1e-10)
        assert np.all(np.isfinite(dx_d))
        if not use_prox:   # x_new = x + dx, the same one addition on both buffers
            assert np.array_equal(bits(x + dx_d), bits(xn_d))
        _need(tail_dx_nonzero=np.sum(dx_d[tail] != 0.0))

    _lockstep(scsopt.ProxLQNSCORE(m=3, use_prox=use_prox), O.ProxLQNSCORE(m=3, use_prox=use_prox), p, om, reg, hm,
              ohm, 4, check)


@pytest.mark.parametrize("reg", ["l1", "indbox"])
def test_lqn_device_loop_past_one_stride_trip(reg, monkeypatch):
    """scs_iterate's ProxLQNSCORE loop at m = 65536 + 300: the fused lqn_tail / lqn_post epoch (and
    norms_part, reg_part before the first epoch) against the oracle's trajectory, and bit for bit
    against the unfused device loop (SCS_LQN_FUSED=0), as test_lqn_fused_epoch_bit_identical
    asserts at m = 20000."""
    m = M_TWO_TRIPS
    p, om, hm, ohm = _tail_pair(m, reg)
    monkeypatch.delenv("SCS_LQN_FUSED", raising=False)
    sol = scsopt.iterate(scsopt.ProxLQNSCORE(m=3), p, reg, hm, max_epoch=6, verbose=0)
    osol = O.iterate(O.ProxLQNSCORE(m=3), om, reg, ohm, max_epoch=6)
    assert sol.epochs == osol.epochs and len(sol.obj) == len(osol.obj)
    assert_close_masked(sol.obj, osol.obj, rtol=1e-8)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(sol.x[TRIP:], osol.x[TRIP:], rtol=1e-6, atol=1e-9)
    _need(tail_moved=np.sum(osol.x[TRIP:] != om.x0[TRIP:]))
    monkeypatch.setenv("SCS_LQN_FUSED", "0")
    b = scsopt.iterate(scsopt.ProxLQNSCORE(m=3), p, reg, hm, max_epoch=6, verbose=0)
    assert sol.epochs == b.epochs and len(sol.obj) == len(b.obj)
    assert_same_nonfinite(sol.obj, b.obj)
    assert np.array_equal(bits(sol.obj), bits(b.obj)) and np.array_equal(bits(sol.fval), bits(b.fval))
    assert sol.pri_res_norm == b.pri_res_norm
    assert np.array_equal(bits(sol.x), bits(b.x))
