"""The Cholesky (chol.hip) and Householder QR (qr.hip) factors themselves, against LAPACK.

Both solvers are reached through their test doors (scs_chol_eval / scs_qr_eval: any matrix, the
production sequence on door-owned buffers), on the cases of solver_factor_data.py whose preconditions
tests/test_solver_factors_host.py asserts.  Every tolerance is one of the project's own bars, a derived
bound, or a stated multiple of LAPACK's value on the same input:

  Cholesky  ρ(U) = max |UᵀU - M|_jk / sqrt(M_jj M_kk) <= γ_{3n+1} + γ_n (Higham Thm 10.4 + the host's
            product) and <= 8 max(ρ(LAPACK), 2⁻⁵³); η = ‖Mx - b‖∞ / (‖M‖∞‖x‖∞) <= 8 max(η(LAPACK), 2⁻⁵³);
            x within 1e-13·cond of LAPACK's; info = dpotrf's.  (8: margin over the 1.8 x a NumPy emulation
            of a 128-blocked factor with explicitly inverted diagonal blocks shows -- MFMA's four partial
            chains per tile, pivots from rsq + Newton.)
  QR        sign(diag R) = LAPACK's and r = ‖RᵀR - AᵀA‖_F <= 8 max(r(LAPACK), 2⁻⁵²‖A‖_F²) (together they pin
            R: the Cholesky factor of AᵀA is unique up to row signs); x by the bars of
            test_householder_qr_solve; exact cases with ==; power-of-two scaling bit for bit.
"""
import numpy as np
import pytest

import scsopt
import solver_factor_data as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = scsopt._lib.Context(0)
    yield c
    c.close()


def _strict_lower_is_zero(T):
    return not np.any(np.tril(T, -1))


# ---- Cholesky -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,dec", D.CHOL_GRID)
def test_chol_factor_vs_lapack(n, dec, ctx, record_property):
    c = D.spd_case(n, dec)
    x, U, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    Ul, linfo = D.lapack_chol(c.M)
    assert info == linfo == 0
    assert U.shape == (n, n) and np.all(np.isfinite(U))
    assert np.all(np.diag(U) > 0)
    assert _strict_lower_is_zero(U)
    rho_dev, rho_ref = D.rho(U, c.M), D.rho(Ul, c.M)
    record_property("rho_dev", rho_dev)
    record_property("rho_ref", rho_ref)
    print(f"chol factor n={n} dec={dec}: rho_dev={rho_dev:.3e} rho_ref={rho_ref:.3e}")
    assert rho_dev <= D.chol_rho_bound(n), (rho_dev, D.chol_rho_bound(n))
    assert rho_dev <= 8 * max(rho_ref, D.U64), (rho_dev, rho_ref)


@pytest.mark.parametrize("n,dec", D.CHOL_GRID)
def test_chol_solve_vs_lapack(n, dec, ctx, record_property):
    c = D.spd_case(n, dec)
    x, _, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    Ul, linfo = D.lapack_chol(c.M)
    assert info == linfo == 0
    xr = D.lapack_chol_solve(Ul, c.b)
    eta_dev, eta_ref = D.eta(c.M, x, c.b), D.eta(c.M, xr, c.b)
    record_property("eta_dev", eta_dev)
    record_property("eta_ref", eta_ref)
    record_property("cond", c.cond)
    print(f"chol solve n={n} dec={dec}: eta_dev={eta_dev:.3e} eta_ref={eta_ref:.3e} cond={c.cond:.3e}")
    assert eta_dev <= 8 * max(eta_ref, D.U64), (eta_dev, eta_ref)
    assert np.max(np.abs(x - xr)) <= 1e-13 * c.cond * np.max(np.abs(xr))


@pytest.mark.parametrize("p", D.INFO_PIVOTS + (-1,))
def test_chol_info_matches_dpotrf(p, ctx):
    """A negative pivot at p (-1: an exactly zero one at D.INFO_SEMIDEF_P): info as dpotrf's, the call
    returns, no x; the SPD solve that follows on the same context is right (info does not stick)."""
    c = D.info_case(p)
    x, U, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    _, linfo = D.lapack_chol(c.M)
    assert info == linfo == c.info
    assert x is None
    xd = np.full(c.n, 7.0)   # the door itself leaves x alone
    di = scsopt._lib.C.c_int()
    Mc, bc = np.ascontiguousarray(c.M.T), np.ascontiguousarray(c.b)
    ctx.check(scsopt._lib.lib.scs_chol_eval(ctx.h, c.n, scsopt._lib.dptr(Mc), scsopt._lib.dptr(bc),
                                            scsopt._lib.dptr(xd), None, scsopt._lib.C.byref(di)))
    assert di.value == c.info and np.all(xd == 7.0)
    good = D.spd_case(D.INFO_N, 2)
    x, U, info = scsopt.chol_solve(good.M, good.b, ctx=ctx)
    assert info == 0
    xr = D.lapack_chol_solve(D.lapack_chol(good.M)[0], good.b)
    assert D.eta(good.M, x, good.b) <= 8 * max(D.eta(good.M, xr, good.b), D.U64)
    assert D.rho(U, good.M) <= D.chol_rho_bound(D.INFO_N)


def _chol_checked(n, dec, ctx):
    c = D.spd_case(n, dec)
    x, U, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    Ul, _ = D.lapack_chol(c.M)
    assert info == 0
    assert D.rho(U, c.M) <= 8 * max(D.rho(Ul, c.M), D.U64)
    xr = D.lapack_chol_solve(Ul, c.b)
    assert D.eta(c.M, x, c.b) <= 8 * max(D.eta(c.M, xr, c.b), D.U64)
    return x, U


def test_chol_sizes_descend_on_one_context():
    """The door's buffers are rebuilt when the padded order changes: 10 blocks, 5, 2, 1."""
    c = scsopt._lib.Context(0)
    for n in (1153, 640, 129, 5):
        _chol_checked(n, 6 if n >= 16 else 2, c)
    c.close()


def test_chol_repeat_is_bitwise(ctx):
    x0, U0 = _chol_checked(1153, 6, ctx)
    x1, U1 = _chol_checked(1153, 6, ctx)
    assert np.array_equal(U0.view(np.int64), U1.view(np.int64))
    assert np.array_equal(x0.view(np.int64), x1.view(np.int64))


def test_chol_reads_upper_triangle_only(ctx):
    """The door's contract (and chol_factor's): nothing below the diagonal is read."""
    c = D.spd_case(257, 6)
    x0, U0, info0 = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    Mu = np.triu(c.M) + np.tril(np.full_like(c.M, np.nan), -1)
    x1, U1, info1 = scsopt.chol_solve(Mu, c.b, ctx=ctx)
    assert info0 == info1 == 0
    assert np.array_equal(U0.view(np.int64), U1.view(np.int64))
    assert np.array_equal(x0.view(np.int64), x1.view(np.int64))


def test_chol_arms_same_factor(ctx, monkeypatch):
    """n = 2304 (18 blocks: the lookahead's bulk stream runs, OB = 4): the arms whose trajectory tests
    claim bit identity give the same U and x bits; the per-block solves (another association) the η bar."""
    c = D.spd_case(*D.CHOL_ARMS)
    x0, U0, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    assert info == 0
    Ul, _ = D.lapack_chol(c.M)
    eta_bar = 8 * max(D.eta(c.M, D.lapack_chol_solve(Ul, c.b), c.b), D.U64)
    assert D.rho(U0, c.M) <= 8 * max(D.rho(Ul, c.M), D.U64)
    assert D.eta(c.M, x0, c.b) <= eta_bar
    for var in ("SCS_CHOL_LA", "SCS_CHOL_SBL", "SCS_CHOL_DIAG"):
        monkeypatch.setenv(var, "0")
        x1, U1, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
        monkeypatch.delenv(var)
        assert info == 0
        assert np.array_equal(U0.view(np.int64), U1.view(np.int64)), var
        assert np.array_equal(x0.view(np.int64), x1.view(np.int64)), var
    monkeypatch.setenv("SCS_SOLVE_PERSIST", "0")
    x2, U2, info = scsopt.chol_solve(c.M, c.b, ctx=ctx)
    assert info == 0
    assert np.array_equal(U0.view(np.int64), U2.view(np.int64))
    assert D.eta(c.M, x2, c.b) <= eta_bar


# ---- QR -----------------------------------------------------------------------------------------

def _coop(monkeypatch, coop):
    if coop:
        monkeypatch.setenv("SCS_QR_COOP", coop)
    else:
        monkeypatch.delenv("SCS_QR_COOP", raising=False)


@pytest.mark.parametrize("coop", ["", "1"])
@pytest.mark.parametrize("family,n", D.QR_GRID)
def test_qr_factor_vs_lapack(family, n, coop, ctx, monkeypatch, record_property):
    _coop(monkeypatch, coop)
    c = D.qr_case(family, n)
    x, R = scsopt.qr_solve(c.A, c.b, ctx=ctx)
    _, _, Rl = D.lapack_qr(c.A)
    assert R.shape == (n, n) and np.all(np.isfinite(R)) and _strict_lower_is_zero(R)
    bad = np.nonzero(np.sign(np.diag(R)) != np.sign(np.diag(Rl)))[0]
    assert bad.size == 0, (bad[:10], np.diag(R)[bad[:10]], np.diag(Rl)[bad[:10]])
    r_dev, r_ref = D.qr_r_measure(R, c.A), D.qr_r_measure(Rl, c.A)
    record_property("r_dev", r_dev)
    record_property("r_ref", r_ref)
    fro2 = float(np.linalg.norm(c.A) ** 2)
    print(f"qr factor {family} n={n} coop={coop!r}: r_dev={r_dev:.3e} r_ref={r_ref:.3e} |A|_F^2={fro2:.3e}")
    assert r_dev <= 8 * max(r_ref, 2.0 ** -52 * fro2), (r_dev, r_ref, fro2)


@pytest.mark.parametrize("coop", ["", "1"])
@pytest.mark.parametrize("family,n", D.QR_GRID)
def test_qr_solve_vs_lapack(family, n, coop, ctx, monkeypatch):
    _coop(monkeypatch, coop)
    c = D.qr_case(family, n)
    x, _ = scsopt.qr_solve(c.A, c.b, ctx=ctx)
    xr = D.lapack_qr_solve(c.A, c.b)
    cond = float(np.linalg.cond(c.A, 2))
    np.testing.assert_allclose(x, xr, rtol=0, atol=1e-13 * cond * float(np.max(np.abs(xr))))
    assert np.linalg.norm(c.A @ x - c.b) <= 1e-12 * np.linalg.norm(c.A, 2) * np.linalg.norm(x)


@pytest.mark.parametrize("coop", ["", "1"])
@pytest.mark.parametrize("n", D.EXACT_ORDERS)
def test_qr_exact_cases(n, coop, ctx, monkeypatch):
    """Upper triangular A with a mixed-sign diagonal: every column is zero below its diagonal, so every tau
    is 0 (the `xx > 0` branch not taken, with a nonzero alpha of either sign) and R == A.
    Signed power-of-two-scaled permutations: alpha = 0 with x != 0 in every column but the first; R == the
    analytic R (every beta < 0, R_00 = s_0 > 0) and x == the exact solution.  (== and not bits: a -0.0 is
    no defect.)"""
    _coop(monkeypatch, coop)
    u = D.upper_case(n)
    _, R = scsopt.qr_solve(u.A, u.b, ctx=ctx)
    assert np.all(R == u.R), np.argwhere(R != u.R)[:10]
    c = D.perm_case(n)
    x, R = scsopt.qr_solve(c.A, c.b, ctx=ctx)
    assert np.all(R == c.R), (np.argwhere(R != c.R)[:10], np.diag(R)[:8], np.diag(c.R)[:8])
    assert np.all(x == c.x), np.nonzero(x != c.x)[0][:10]


def test_qr_lu_power_of_two_scaling(ctx):
    """Scaling A and b by 2^±200 (every square stays in the normal range) changes no rounding: the same
    x bits, R times 2^k exactly, the same LU pivots.  An absolute threshold anywhere would show."""
    c = D.qr_case("gauss", 300)
    x0, R0 = scsopt.qr_solve(c.A, c.b, ctx=ctx)
    xl0, piv0, info0 = scsopt.lu_solve(c.A, c.b, ctx=ctx)
    assert info0 == 0
    for k in (200, -200):
        s = np.ldexp(1.0, k)
        x1, R1 = scsopt.qr_solve(c.A * s, c.b * s, ctx=ctx)
        assert np.array_equal(x1.view(np.int64), x0.view(np.int64)), k
        assert np.all(R1 == R0 * s), k
        xl1, piv1, info1 = scsopt.lu_solve(c.A * s, c.b * s, ctx=ctx)
        assert info1 == 0 and np.array_equal(piv1, piv0), k
        assert np.array_equal(xl1.view(np.int64), xl0.view(np.int64)), k


def test_qr_arms_same_factor(ctx, monkeypatch):
    """The sample-space family at n = 1000 (8 panels): the arms whose existing tests claim the same bits
    give the same R and x bits."""
    c = D.qr_case("sample", 1000)

    def run():
        x, R = scsopt.qr_solve(c.A, c.b, ctx=ctx)
        return x.view(np.int64), R.view(np.int64)

    monkeypatch.setenv("SCS_QR_LA", "0")
    x0, R0 = run()
    monkeypatch.setenv("SCS_QR_LA", "1")
    x1, R1 = run()
    monkeypatch.delenv("SCS_QR_LA")
    assert np.array_equal(R0, R1) and np.array_equal(x0, x1)
    monkeypatch.setenv("SCS_QR_RC", "1024")
    monkeypatch.setenv("SCS_QR_CPW", "1")
    x0, R0 = run()
    monkeypatch.setenv("SCS_QR_CPW", "4")
    x1, R1 = run()
    assert np.array_equal(R0, R1) and np.array_equal(x0, x1)


def test_qr_sizes_descend_on_one_context():
    c = scsopt._lib.Context(0)
    for n in (1000, 300, 129, 5):
        q = D.qr_case("sample", n)
        x, R = scsopt.qr_solve(q.A, q.b, ctx=c)
        _, _, Rl = D.lapack_qr(q.A)
        assert np.array_equal(np.sign(np.diag(R)), np.sign(np.diag(Rl)))
        assert D.qr_r_measure(R, q.A) <= 8 * max(D.qr_r_measure(Rl, q.A), 2.0 ** -52 * np.linalg.norm(q.A) ** 2)
        assert np.linalg.norm(q.A @ x - q.b) <= 1e-12 * np.linalg.norm(q.A, 2) * np.linalg.norm(x)
    c.close()
