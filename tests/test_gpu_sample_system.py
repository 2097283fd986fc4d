"""GPU: the sample-space system of a single-output ProxGGNSCORE step (N + 1 <= m), through the door onto
the step's own function (scs_sample_system_eval / Problem.sample_system):

    M[i][j] = δ_ij + q_i s_i s_j P_ij      M[i][N] = q_i s_i u_i      M[N][·] = e_N      b = [r; 1]

a. exact placement on integer data, every shape and route, nothing written beyond order N + 1;
b. the system against the NumPy restatement within derived bounds, on benign and on hard inputs;
c. the direction on systems whose LU interchanges rows, both solver arms, in lock step with the oracle;
d. the branch test N + 1 <= m on dense data and on minibatches;
e. non-finite systems, and no leftover of one in the next step;
f. state: door and step do not disturb each other; every refusal leaves the context usable.

The restatement, the cases and the bounds live in tests/sample_system_data.py; their preconditions (and
that the bounds are not vacuous) are asserted without a GPU in tests/test_sample_system_host.py.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import scsopt
from scsopt import _lib, losses
from scsopt.iterate import init_method, step

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402
import sample_system_data as D  # noqa: E402
from test_gpu_kernel_edges import _need, assert_same_nonfinite  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -7.25
# every route at these; the other shapes on the dense fp64 route and on the nonzeros
ALL_ROUTE_SHAPES = [(1, 2), (127, 128), (128, 129)]
TWO_ROUTE_SHAPES = [s for s in D.SHAPES if s not in ALL_ROUTE_SHAPES]
DIRECTION_SHAPES = [(1, 2), (2, 3)] + [s for s in D.SHAPES if s[0] >= 127]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _losses(kind, c):
    if kind == "logistic":
        return losses.logistic_ce(c), losses.sigmoid_ce(c)
    return losses.least_squares(c), losses.linear_ls(c)


def _oracle_problem(kind, A, y, x0, c, lam):
    loss = O.Loss("logistic_ce", c, ggn="sigmoid_ce") if kind == "logistic" else O.Loss("least_squares", c, ggn="linear_ls")
    return O.Problem(A, y, x0, loss, lam)


def _problem(kind, A, y, x0, c, lam, route="dense", **kw):
    f, out = _losses(kind, c)
    if route == "dense_f32":
        p = scsopt.Problem(A.astype(np.float32), y, x0, f, lam, out_fn=out, dense_f32=True, **kw)
        assert p.data_info()[0] == 4
    elif route == "sparse_sample":
        p = scsopt.Problem(sp.csr_matrix(A), y, x0, f, lam, out_fn=out, sparse_sample=True, **kw)
    elif route == "sparse_mirror":
        p = scsopt.Problem(sp.csr_matrix(A), y, x0, f, lam, out_fn=out, **kw)
    else:
        p = scsopt.Problem(A, y, x0, f, lam, out_fn=out, **kw)
    return p


def _case_problem(cs, route="dense"):
    p = _problem(cs.kind, cs.A, cs.y, cs.x0, cs.c, cs.lam, route)
    p.configure("l1", scsopt.PHuberSmootherL1L2(cs.mu))
    return p


def _door_raw(p, x, n1):
    """The door into a host matrix with a larger leading dimension and spare columns: (M, b), after
    checking that the sentinel beyond order n1 is untouched."""
    ldm, ncol = n1 + 3, n1 + 2
    buf = np.full(ldm * ncol, SENT)
    b = np.full(n1 + 2, SENT)
    p.ctx.check(_lib.lib.scs_sample_system_eval(p.ctx.h, _lib.dptr(np.ascontiguousarray(x)), _lib.dptr(buf), ldm,
                                                _lib.dptr(b)))
    G = buf.reshape(ncol, ldm).T                                     # column-major: G[i, j]
    assert np.all(G[n1:, :] == SENT) and np.all(G[:, n1:] == SENT) and np.all(b[n1:] == SENT)
    return G[:n1, :n1].copy(), b[:n1].copy()


def _check_structure(M, b, kind):
    """The last row is exactly e_N, b[N] exactly 1.0; the least-squares block is bitwise symmetric."""
    n1 = b.size
    e_n = np.zeros(n1)
    e_n[-1] = 1.0
    assert np.array_equal(bits(M[-1]), bits(e_n)) and b[-1] == 1.0
    if kind == "least_squares":
        assert np.array_equal(bits(M[:-1, :-1]), bits(M[:-1, :-1].T))


# ---------------------------------------------------------------------------------------------
# a. exact placement
# ---------------------------------------------------------------------------------------------
_A_CASES = [(s, r) for s in D.SHAPES for r in ("dense", "dense_f32")] + \
           [(s, r) for s in D.SHAPES if s not in ((1, 130), (127, 129), (128, 300), (129, 130))
            for r in ("sparse_sample", "sparse_mirror")]


@pytest.mark.parametrize("shape,route", _A_CASES, ids=[f"{s[0]}x{s[1]}-{r}" for s, r in _A_CASES])
def test_placement_exact(shape, route):
    """Least squares at x = 0, scale 2⁻², integer A in ±8 and y in ±5, PHuberSmootherL1L2(mu) with mu a power
    of two (Hr = 1 / mu exactly, gr = 0; Σ|terms| < 2^53 asserted in exact_case): the door returns, bit for
    bit, M = I + 2⁻² mu A Aᵀ with a last column of +0.0 and b = [-y / 4; 1], and leaves the sentinel around
    order N + 1 untouched.  The integers are exact in fp32, so the fp32-stored routes give the same bits."""
    N, m = shape
    mu = 2.0 if (N + m) % 2 else 0.5
    A, y, Mx, bx = D.exact_case(N, m, mu)
    x = np.zeros(m)
    p = _problem("least_squares", A, y, x, 0.25, 0.3, route)
    hm = scsopt.PHuberSmootherL1L2(mu)
    p.configure("l1", hm)
    gr, Hr = p._smoother_eval(hm, x)
    assert np.all(Hr == 1.0 / mu) and np.array_equal(bits(gr), bits(np.zeros(m)))
    M, b = _door_raw(p, x, N + 1)
    M2, b2 = p.sample_system(x)
    p.ctx.close()
    assert np.array_equal(bits(M), bits(M2)) and np.array_equal(bits(b), bits(b2))
    assert not np.any(np.signbit(M[:N, N])) and np.all(M[:N, N] == 0.0)
    assert np.array_equal(bits(b), bits(bx))
    assert np.array_equal(bits(M), bits(Mx)), np.argwhere(bits(M) != bits(Mx))[:4]


# ---------------------------------------------------------------------------------------------
# b. the system against the restatement at x != 0
# ---------------------------------------------------------------------------------------------
_B_CASES = [(k, s, h, r) for k in D.KINDS for s in ALL_ROUTE_SHAPES for h in (False, True) for r in D.ROUTES] + \
           [(k, s, True, r) for k in D.KINDS for s in TWO_ROUTE_SHAPES for r in ("dense", "sparse_sample")] + \
           [(k, (300, 1000), False, "dense") for k in D.KINDS]


@pytest.mark.parametrize("kind,shape,hard,route", _B_CASES,
                         ids=[f"{k}-{s[0]}x{s[1]}-{'hard' if h else 'easy'}-{r}" for k, s, h, r in _B_CASES])
def test_system_vs_restatement(kind, shape, hard, route):
    """sample_system(x0) against sample_system_data.system on the values the route stores (an fp32-stored
    A is rounded first), entry by entry within system_bounds -- derived there: the product bound
    1e-13 Σ|terms| for z, P and u; δz carried through s, q, r by their derivatives (the cancellation of
    1 - ŷ included); a counted number of ε for the elementwise operations and for the device's exp against
    libm.  gr and Hr are the device's own (the smoother kernels have their tests), so h and h ∘ λ gr carry no
    error.  The nonzeros route and the mirrored one differ in P's summation order only: both within the
    bound of the one restatement.  Structure: last row e_N and b[N] = 1 exactly, least squares bitwise
    symmetric, nothing written beyond order N + 1."""
    N, m = shape
    cs = D.case(kind, N, m, hard)
    if hard:
        f = D.hard_preconditions(cs)
        _need(last_column=f["last"] >= 1.0, pivots=(kind != "logistic" or N < 2 or f["swaps"] >= 1))
    p = _case_problem(cs, route)
    gr, Hr = p._smoother_eval(scsopt.PHuberSmootherL1L2(cs.mu), cs.x0)
    M, b = _door_raw(p, cs.x0, N + 1)
    p.ctx.close()
    Mr, br, dM, db, _, _, _ = cs.system_at(cs.x0, route, Hr=Hr, gr=gr)
    assert np.all(np.isfinite(M)) and np.all(np.isfinite(b))
    _check_structure(M, b, kind)
    errM, errb = np.abs(M - Mr), np.abs(b - br)
    wM = float(np.max(errM[:N] / dM[:N])) if N else 0.0
    wb = float(np.max(errb[:N] / db[:N]))
    print(f"[b] {kind} ({N}, {m}) {'hard' if hard else 'easy'} {route}: max M err / bound {wM:.3e}, "
          f"max b err / bound {wb:.3e}, cond {np.linalg.cond(Mr):.3g}")
    assert np.all(errM <= dM)
    assert np.all(errb <= db)


# ---------------------------------------------------------------------------------------------
# c. the direction, on systems that pivot
# ---------------------------------------------------------------------------------------------
def _oracle_step_dx(ometh, om, ohm, x, it):
    """O.step's x_new and pri, and the dx of that step from the oracle's own functions (O.step returns
    x_new = x + dx only; x_new - x would carry the rounding of that sum)."""
    xn, pri = O.step(ometh, om, "l1", ohm, x, x, None, it)
    lam = om.lam
    gr, Hr = ohm.grad(None, x), ohm.hess(None, x)
    s, r, q = om.f.ggn_parts(om.A, om.y, x)
    d = O.ggn_score_step(om.A, s, r, q, lam * gr, Hr, lam)
    _, dx, _ = O._score_finish(ometh, om, "l1", ohm, x, d, lam, lam * gr, Hr, O._step_size_newton_like(ometh, om, it))
    assert np.array_equal(bits(x + dx), bits(xn)) and pri == float(np.linalg.norm(dx))
    return xn, dx, pri


def _direction_lockstep(cs, p, solver, nsteps=3):
    """Both sides step from the oracle's x; returns the worst error over 1e-13·cond(M)·max|dx_oracle|."""
    if solver != "default":
        p.set_solver(solver)
    hm, ohm = scsopt.PHuberSmootherL1L2(cs.mu), O.PHuberSmootherL1L2(cs.mu)
    meth, ometh = scsopt.ProxGGNSCORE(use_prox=False), O.ProxGGNSCORE(use_prox=False)
    om = _oracle_problem(cs.kind, cs.A, cs.y, cs.x0, cs.c, cs.lam)
    p.configure("l1", hm)
    init_method(meth, p)
    x = cs.x0.copy()
    worst = 0.0
    for it in range(1, nsteps + 1):
        cond = float(np.linalg.cond(cs.system_at(x)[0]))
        xn_d, dx_d, pri_d = step(meth, p, "l1", hm, x, x, it, return_dx=True)
        xn_o, dx_o, pri_o = _oracle_step_dx(ometh, om, ohm, x, it)
        assert np.all(np.isfinite(dx_o))
        tol = 1e-13 * cond
        e_dx = float(np.max(np.abs(dx_d - dx_o))) / float(np.max(np.abs(dx_o)))
        e_pri = abs(pri_d - pri_o) / abs(pri_o)
        print(f"[c] {cs.kind} ({cs.N}, {cs.m}) {solver} step {it}: cond {cond:.3g}, max |Δdx| / max |dx| = {e_dx:.3e} "
              f"({e_dx / tol:.3e} of 1e-13 cond), pri rel = {e_pri:.3e} ({e_pri / tol:.3e})")
        assert e_dx <= tol
        assert e_pri <= tol
        worst = max(worst, e_dx / tol, e_pri / tol)
        x = xn_o
    return worst


@pytest.mark.parametrize("solver", ["default", "reference"])
@pytest.mark.parametrize("shape", DIRECTION_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in DIRECTION_SHAPES])
@pytest.mark.parametrize("kind", D.KINDS)
def test_direction_on_pivoting_systems(kind, shape, solver):
    """Three lock-step ProxGGNSCORE steps (use_prox=False, ss_type 1, return_dx) on the hard inputs, from the
    oracle's x: max |Δdx| <= 1e-13·cond(M)·max |dx_oracle| and pri to the same relative bound -- the
    tolerance test_reference_solver_ill_conditioned holds this project's solvers to -- with the default LU
    (whose getrf interchanges rows here, asserted for the logistic loss) and the reference mode's
    Householder QR (the oracle's literal QR, FAST_LINALG off)."""
    assert O.FAST_LINALG is False
    cs = D.case(kind, shape[0], shape[1], True)
    f = D.hard_preconditions(cs)
    _need(pivots=(kind != "logistic" or shape[0] < 2 or f["swaps"] >= 1))
    p = _problem(kind, cs.A, cs.y, cs.x0, cs.c, cs.lam)
    try:
        _direction_lockstep(cs, p, solver)
    finally:
        p.ctx.close()


# ---------------------------------------------------------------------------------------------
# d. the branch boundary on dense data
# ---------------------------------------------------------------------------------------------
def _step_vs_oracle(cs, p, x):
    """One default step against the oracle's at the project's lock-step tolerances."""
    hm, ohm = scsopt.PHuberSmootherL1L2(cs.mu), O.PHuberSmootherL1L2(cs.mu)
    meth = scsopt.ProxGGNSCORE()
    p.configure("l1", hm)
    init_method(meth, p)
    xn, pri = step(meth, p, "l1", hm, x, x, 1)
    om = _oracle_problem(cs.kind, cs.A, cs.y, cs.x0, cs.c, cs.lam)
    xo, prio = O.step(O.ProxGGNSCORE(), om, "l1", ohm, x, x, None, 1)
    np.testing.assert_allclose(xn, xo, rtol=1e-7, atol=1e-10)
    assert pri == pytest.approx(prio, rel=1e-7)
    return xn, pri


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("m", [128, 130])
def test_branch_boundary_dense(m, kind):
    """(m - 1, m): N + 1 = m, the last shape of the sample-space branch -- the door returns a system (within
    the bounds of b) and the step matches the oracle.  (m, m): the door refuses with SCS_ERR_ARG, the step
    matches the oracle's feature branch."""
    cs = D.case(kind, m - 1, m, False)
    p = _case_problem(cs)
    gr, Hr = p._smoother_eval(scsopt.PHuberSmootherL1L2(cs.mu), cs.x0)
    M, b = _door_raw(p, cs.x0, m)
    Mr, br, dM, db, _, _, _ = cs.system_at(cs.x0, Hr=Hr, gr=gr)
    assert np.all(np.abs(M - Mr) <= dM) and np.all(np.abs(b - br) <= db)
    _check_structure(M, b, kind)
    _step_vs_oracle(cs, p, cs.x0)
    p.ctx.close()
    cs = D.case(kind, m, m, False)
    p = _case_problem(cs)
    with pytest.raises(scsopt.ScsError, match=rf"N \+ 1 = {m + 1} > m = {m}.*feature branch.*scs_solve_eval") as ei:
        p.sample_system(cs.x0)
    assert ei.value.code == _lib.SCS_ERR_ARG
    _step_vs_oracle(cs, p, cs.x0)
    p.ctx.close()


@pytest.mark.parametrize("m", [128, 130])
def test_door_follows_select_batch(m):
    """One dense context of 2 m - 1 rows with the batches (m - 1 rows, m rows): the door serves the rows
    select_batch chose -- a system for batch 0, bit for bit the system of a context holding those rows; a
    refusal naming n_b + 1 = m + 1 for batch 1; the full data's own answer (its N + 1 = 2 m) before and
    after.  On a context whose full data has the branch's shape, select_batch(-1) brings its system back
    bit for bit."""
    kind = "logistic"
    cs = D.case(kind, 2 * m - 1, m, False)
    perm = np.random.default_rng(m).permutation(cs.N)
    batches = [perm[:m - 1], perm[m - 1:]]
    assert [b.size for b in batches] == [m - 1, m]
    p = _case_problem(cs)
    init_method(scsopt.ProxGGNSCORE(), p)
    p.set_batches(batches)
    try:
        with pytest.raises(scsopt.ScsError, match=rf"N \+ 1 = {2 * m} > m = {m}"):
            p.sample_system(cs.x0)
        p.select_batch(0)
        M0, b0 = p.sample_system(cs.x0)
        assert M0.shape == (m, m)
        p.select_batch(1)
        with pytest.raises(scsopt.ScsError, match=rf"N \+ 1 = {m + 1} > m = {m}") as ei:
            p.sample_system(cs.x0)
        assert ei.value.code == _lib.SCS_ERR_ARG
        p.select_batch(-1)
        with pytest.raises(scsopt.ScsError, match=rf"N \+ 1 = {2 * m} > m = {m}"):
            p.sample_system(cs.x0)
        p.select_batch(0)
        M0b, b0b = p.sample_system(cs.x0)
        assert np.array_equal(bits(M0), bits(M0b)) and np.array_equal(bits(b0), bits(b0b))
        p.select_batch(-1)
    finally:
        p.set_batches(None)
        p.ctx.close()
    rows = batches[0]
    q = _problem(kind, cs.A[rows], cs.y[rows], cs.x0, cs.c, cs.lam)
    q.configure("l1", scsopt.PHuberSmootherL1L2(cs.mu))
    Mq, bq = q.sample_system(cs.x0)
    assert np.array_equal(bits(M0), bits(Mq)) and np.array_equal(bits(b0), bits(bq))
    # the full data in the branch's shape: its rows again after select_batch(-1)
    init_method(scsopt.ProxGGNSCORE(), q)
    q.set_batches([np.arange(m - 1)[::-1][:m - 3]])
    try:
        q.select_batch(0)
        Ms, _ = q.sample_system(cs.x0)
        assert Ms.shape == (m - 2, m - 2)
        q.select_batch(-1)
        Mf, bf = q.sample_system(cs.x0)
        assert np.array_equal(bits(Mf), bits(Mq)) and np.array_equal(bits(bf), bits(bq))
    finally:
        q.set_batches(None)
        q.ctx.close()


# ---------------------------------------------------------------------------------------------
# e. non-finite systems
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["default", "reference"])
@pytest.mark.parametrize("kind", D.KINDS)
def test_nonfinite_system_and_no_leftover(kind, solver):
    """x with one coordinate 1e200: Hr = 0 there, h = Inf.  The oracle's step is all NaN with a NaN pri and
    raises nothing (asserted, under both FAST_LINALG settings); so is the device's, with no error and nothing
    counted in scs_fallback_counts; the door's NaN / +Inf / -Inf masks are the restatement's.  Then a
    finite x on the same context gives, bit for bit, the step of a fresh context: nothing of the NaN step is
    left in the system, the right-hand side or the QR's copy."""
    N, m = 127, 129
    cs = D.case(kind, N, m, False)
    xbad = cs.x0.copy()
    xbad[5] = 1e200
    hm, ohm = scsopt.PHuberSmootherL1L2(cs.mu), O.PHuberSmootherL1L2(cs.mu)
    om = _oracle_problem(kind, cs.A, cs.y, cs.x0, cs.c, cs.lam)
    for fast in (False, True):
        O.FAST_LINALG = fast
        try:
            with np.errstate(all="ignore"):
                xo, prio = O.step(O.ProxGGNSCORE(), om, "l1", ohm, xbad, xbad, None, 1)
        finally:
            O.FAST_LINALG = False
        assert np.all(np.isnan(xo)) and np.isnan(prio)
    with np.errstate(all="ignore"):
        Mr, br, _, _, _, _, Hr = cs.system_at(xbad)
    _need(zero_Hr=np.sum(Hr == 0.0), nonfinite_M=np.sum(~np.isfinite(Mr)), finite_M=np.sum(np.isfinite(Mr)))

    def steps(p, xs):
        if solver != "default":
            p.set_solver(solver)
        p.configure("l1", hm)
        meth = scsopt.ProxGGNSCORE()
        init_method(meth, p)
        return [step(meth, p, "l1", hm, x, x, it + 1) for it, x in enumerate(xs)]

    p = _problem(kind, cs.A, cs.y, cs.x0, cs.c, cs.lam)
    fresh = _problem(kind, cs.A, cs.y, cs.x0, cs.c, cs.lam)
    try:
        (xn, pri), = steps(p, [xbad])
        assert np.all(np.isnan(xn)) and np.isnan(pri)
        assert not any(p.ctx.fallback_counts().values())
        M, b = _door_raw(p, xbad, N + 1)
        assert_same_nonfinite(M.ravel(), Mr.ravel())
        assert_same_nonfinite(b, br)
        (xn, pri), = steps(p, [xbad])                                   # after the door, the same
        assert np.all(np.isnan(xn)) and np.isnan(pri)
        got = steps(p, [cs.x0, 0.5 * cs.x0])
        ref = steps(fresh, [cs.x0, 0.5 * cs.x0])
        for (xg, pg), (xr, pr) in zip(got, ref):
            assert np.all(np.isfinite(xr)) and np.isfinite(pr)
            assert np.array_equal(bits(xg), bits(xr)) and np.array_equal(bits(pg), bits(pr))
        Mg, bg = p.sample_system(cs.x0)
        Mf, bf = fresh.sample_system(cs.x0)
        assert np.array_equal(bits(Mg), bits(Mf)) and np.array_equal(bits(bg), bits(bf))
    finally:
        p.ctx.close()
        fresh.ctx.close()


# ---------------------------------------------------------------------------------------------
# f. state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", D.ROUTES)
def test_door_and_step_do_not_disturb_each_other(route):
    """A sample-space step, the door, the same step again: the same bits; the door twice: the same bits; and
    the door's system is the one of a context that never stepped."""
    cs = D.case("logistic", 128, 129, True)
    hm = scsopt.PHuberSmootherL1L2(cs.mu)
    p = _case_problem(cs, route)
    meth = scsopt.ProxGGNSCORE()
    init_method(meth, p)
    try:
        x1, pri1 = step(meth, p, "l1", hm, cs.x0, cs.x0, 1)
        Ma, ba = p.sample_system(0.5 * cs.x0)                          # another point than the step's
        Mb, bb = p.sample_system(0.5 * cs.x0)
        x2, pri2 = step(meth, p, "l1", hm, cs.x0, cs.x0, 1)
        assert np.array_equal(bits(x1), bits(x2)) and np.array_equal(bits(pri1), bits(pri2))
        assert np.array_equal(bits(Ma), bits(Mb)) and np.array_equal(bits(ba), bits(bb))
        fresh = _case_problem(cs, route)
        Mf, bf = fresh.sample_system(0.5 * cs.x0)
        fresh.ctx.close()
        assert np.array_equal(bits(Ma), bits(Mf)) and np.array_equal(bits(ba), bits(bf))
        # either output may be NULL
        n1 = cs.N + 1
        bonly = np.empty(n1)
        p.ctx.check(_lib.lib.scs_sample_system_eval(p.ctx.h, _lib.dptr(0.5 * cs.x0), None, 0, _lib.dptr(bonly)))
        assert np.array_equal(bits(bonly), bits(ba))
        Monly = np.zeros(n1 * n1)
        p.ctx.check(_lib.lib.scs_sample_system_eval(p.ctx.h, _lib.dptr(0.5 * cs.x0), _lib.dptr(Monly), n1, None))
        assert np.array_equal(bits(Monly.reshape(n1, n1).T), bits(Ma))
    finally:
        p.ctx.close()


def _refused(p, x, code, pattern, M=True, ldm=None, n1=21):
    buf = np.zeros(n1 * n1)
    b = np.zeros(n1)
    rc = _lib.lib.scs_sample_system_eval(p.ctx.h, None if x is None else _lib.dptr(x), _lib.dptr(buf) if M else None,
                                         n1 if ldm is None else ldm, _lib.dptr(b))
    assert rc == code, (rc, code)
    with pytest.raises(scsopt.ScsError, match=pattern):
        p.ctx.check(rc)


def test_refusals_leave_the_context_usable():
    """Every refusal names its reason and carries the code of the header; after each the context still
    gives the system and the step it gave before."""
    cs = D.case("logistic", 20, 30, False)
    hm = scsopt.PHuberSmootherL1L2(cs.mu)
    x0 = cs.x0
    ST, ARG = _lib.SCS_ERR_STATE, _lib.SCS_ERR_ARG
    # no regularizer / smoother yet
    p = _problem(cs.kind, cs.A, cs.y, x0, cs.c, cs.lam)
    _refused(p, x0, ST, r"regularizer and the smoother")
    p.configure("l1", hm)
    meth = scsopt.ProxGGNSCORE()
    init_method(meth, p)
    M0, b0 = p.sample_system(x0)
    xs, ps = step(meth, p, "l1", hm, x0, x0, 1)

    def still_fine():
        M1, b1 = p.sample_system(x0)
        xn, pn = step(meth, p, "l1", hm, x0, x0, 1)
        assert np.array_equal(bits(M1), bits(M0)) and np.array_equal(bits(b1), bits(b0))
        assert np.array_equal(bits(xn), bits(xs)) and np.array_equal(bits(pn), bits(ps))

    _refused(p, None, ARG, r"null x")
    still_fine()
    _refused(p, x0, ARG, r"ldm 20 < N \+ 1 = 21", ldm=20)
    still_fine()
    p.ctx.close()
    # no GGN kind
    f, _ = _losses(cs.kind, cs.c)
    p = scsopt.Problem(cs.A, cs.y, x0, f, cs.lam)
    p.configure("l1", hm)
    _refused(p, x0, ARG, r"out_fn / GGN loss kind")
    assert np.isfinite(p.fx(x0))
    p.ctx.close()
    # a context without data or loss
    ctx = _lib.Context(0)
    rc = _lib.lib.scs_sample_system_eval(ctx.h, _lib.dptr(x0), None, 0, None)
    assert rc == ST
    ctx.close()
    # a generic problem (no data), a callback loss on data (its J is the caller's)
    p = scsopt.Problem(x0, losses.rosenbrock(), cs.lam)
    p.configure("l1", hm)
    _refused(p, x0, ST, r"no data")
    p.ctx.close()
    fo = _oracle_problem(cs.kind, cs.A, cs.y, x0, cs.c, cs.lam)
    p = scsopt.Problem(cs.A, cs.y, x0, losses.callback(lambda A, y, x: fo.f.f(A, y, x), lambda A, y, x: fo.f.grad(A, y, x)),
                       cs.lam)
    p.configure("l1", hm)
    _refused(p, x0, ARG, r"callback loss")
    assert p.fx(x0) == pytest.approx(fo.fx(x0), rel=1e-12)
    p.ctx.close()
    # a multi-output context: the multi door is named
    Y = np.stack([cs.y, 1.0 - cs.y], axis=1)
    p = scsopt.Problem(cs.A, Y, np.concatenate([x0, x0]), losses.softmax_ce(2, cs.c), cs.lam,
                       out_fn=losses.linear_softmax_ce(2, cs.c),
                       multi_sample=True)
    p.configure("l1", hm)
    n1 = cs.N + 1
    rc = _lib.lib.scs_sample_system_eval(p.ctx.h, _lib.dptr(np.concatenate([x0, x0])), _lib.dptr(np.zeros(n1 * n1)), n1,
                                         _lib.dptr(np.zeros(n1)))
    assert rc == ST
    with pytest.raises(scsopt.ScsError, match=r"scs_multi_sample_system_eval"):
        p.ctx.check(rc)
    Mm, _ = p.multi_sample_system(np.concatenate([x0, x0]))
    assert np.all(np.isfinite(Mm))
    p.ctx.close()
    # a batch held as ProxLQNSCORE's sparse view (sparse_batches) keeps no rows for the system
    p = _problem(cs.kind, cs.A, cs.y, x0, cs.c, cs.lam, "sparse_mirror", sparse_batches=True)
    p.configure("l1", hm)
    Mfull, _ = p.sample_system(x0)
    np.testing.assert_allclose(Mfull, M0, rtol=1e-12, atol=1e-15)     # (z by the SpMV: another summation order)
    lqn = scsopt.ProxLQNSCORE(m=3)
    init_method(lqn, p)
    p.set_batches([np.arange(10), np.arange(10, 20)])
    p.select_batch(0)
    _refused(p, x0, ST, r"sparse view of ProxLQNSCORE", n1=11)
    xl, _ = step(lqn, p, "l1", hm, x0, x0, 1)
    assert np.all(np.isfinite(xl))
    p.select_batch(-1)
    Mfull2, _ = p.sample_system(x0)
    assert np.array_equal(bits(Mfull2), bits(Mfull))
    p.set_batches(None)
    p.ctx.close()
    # more than one rank: a group of two sub-contexts
    p = _problem(cs.kind, cs.A, cs.y, x0, cs.c, cs.lam, devices=[0, 0], device_exchange="host")
    p.configure("l1", hm)
    rc = _lib.lib.scs_sample_system_eval(p.ctx.h, _lib.dptr(x0), None, 0, None)
    assert rc == ARG
    with pytest.raises(scsopt.ScsError, match=r"single-device context"):
        p.ctx.check(rc)
    assert p.fx(x0) == pytest.approx(fo.fx(x0), rel=1e-12)
    p.ctx.close()
