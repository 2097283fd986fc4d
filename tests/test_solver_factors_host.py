"""Preconditions of tests/test_gpu_solver_factors.py, asserted on the host with LAPACK alone
(scipy.linalg.lapack dpotrf / dpotrs / dgeqrf): the cases of solver_factor_data.py are what the GPU
tests take them for, and LAPACK's own factors meet the bounds the device's are then held to."""
import numpy as np
import pytest

import solver_factor_data as D


@pytest.mark.parametrize("n,dec", D.CHOL_GRID + (D.CHOL_ARMS,))
def test_spd_family(n, dec):
    """dpotrf succeeds; cond₂ within a factor 2 of 10^dec (a 1 x 1 matrix has cond 1); LAPACK's own
    componentwise backward ratio ρ below the derived bound γ_{3n+1} + γ_n."""
    c = D.spd_case(n, dec)
    assert np.array_equal(c.M, c.M.T)
    U, info = D.lapack_chol(c.M)
    assert info == 0 and np.all(np.diag(U) > 0)
    want = 10.0 ** dec if n > 1 else 1.0
    cond = float(np.linalg.cond(c.M, 2))
    assert want / 2 <= cond <= want * 2, cond
    assert want / 2 <= c.cond <= want * 2, c.cond   # (the eigenvalue form the GPU tests use)
    r = D.rho(U, c.M)
    assert r <= D.chol_rho_bound(n), (r, D.chol_rho_bound(n))
    x = D.lapack_chol_solve(U, c.b)
    assert D.eta(c.M, x, c.b) <= D.chol_rho_bound(n)


def test_gamma():
    assert D.gamma(1) == pytest.approx(2.0 ** -53)
    assert 5.4e-12 < D.gamma(3 * 16384 + 1) < 5.6e-12   # the figure test_gpu_full_size.py quotes


@pytest.mark.parametrize("p", D.INFO_PIVOTS + (-1,))
def test_pivot_placement(p):
    c = D.info_case(p)
    _, info = D.lapack_chol(c.M)
    assert info == c.info
    assert c.info == (p + 1 if p >= 0 else D.INFO_SEMIDEF_P + 1)
    assert np.array_equal(c.M, c.M.T)


def test_pivot_placement_moves():
    """The construction at the edges a block kernel has: first / last step of a 128-block, a 16-sub-block
    edge, and the last row, on a second order as well."""
    base = D.spd_case(257, 2)
    U, _ = D.lapack_chol(base.M)
    for p in (0, 15, 16, 127, 128, 200, 256):
        M = base.M.copy()
        M[p, p] -= 1.5 * U[p, p] ** 2
        assert D.lapack_chol(M)[1] == p + 1


@pytest.mark.parametrize("family,n", D.QR_GRID)
def test_qr_family(family, n):
    """cond₂ <= 1e4, and no diagonal entry of LAPACK's R near zero: min |R_cc| >= 1e-3 ‖A‖_F / √n, so a
    sign comparison is never made on rounding noise."""
    c = D.qr_case(family, n)
    assert np.linalg.cond(c.A, 2) <= 1e4
    _, _, R = D.lapack_qr(c.A)
    assert np.min(np.abs(np.diag(R))) >= 1e-3 * np.linalg.norm(c.A) / np.sqrt(n)
    # LAPACK's R by the measure the device's is held to: far below the 8 x 2⁻⁵² ‖A‖_F² floor's scale
    assert D.qr_r_measure(R, c.A) <= 8 * 2.0 ** -52 * np.linalg.norm(c.A) ** 2
    x = D.lapack_qr_solve(c.A, c.b)
    assert np.linalg.norm(c.A @ x - c.b) <= 1e-12 * np.linalg.norm(c.A, 2) * np.linalg.norm(x)
    if family == "negdiag" and n >= 127:
        assert 0.4 <= np.mean(np.diag(c.A) < 0) <= 0.6
        assert 0.4 <= np.mean(np.diag(R) > 0) <= 0.6   # beta > 0 where alpha < 0


@pytest.mark.parametrize("n", D.EXACT_ORDERS)
def test_upper_triangular_exact(n):
    c = D.upper_case(n)
    d = np.diag(c.A)
    assert np.all(d != 0) and np.any(d < 0) and np.any(d > 0)
    _, tau, R = D.lapack_qr(c.A)
    assert np.all(tau == 0.0)
    assert np.all(R == c.R)


@pytest.mark.parametrize("n", D.EXACT_ORDERS)
def test_signed_permutation_exact(n):
    c = D.perm_case(n)
    assert np.all(np.count_nonzero(c.A, axis=0) == 1) and np.all(np.count_nonzero(c.A, axis=1) == 1)
    _, tau, R = D.lapack_qr(c.A)
    assert np.all(R == c.R)
    assert np.all(tau == c.tau)
    assert np.all(np.isin(tau, (0.0, 1.0))) and np.any(tau == 0.0) and np.any(tau == 1.0)
    assert np.all(R == np.diag(np.diag(R)))
    assert np.array_equal(np.abs(np.diag(R)), np.abs(c.s))
    assert np.any(np.diag(R) > 0) and np.any(np.diag(R) < 0)
    assert np.all(c.A @ c.x == c.b)
    assert np.all(D.lapack_qr_solve(c.A, c.b) == c.x)


def test_power_of_two_scaling_is_exact_on_the_host():
    """2^±200 A stays inside the normal range with its squares and their sum, so arithmetic without an
    absolute threshold cannot tell the scaled system from the unscaled one."""
    c = D.qr_case("gauss", 300)
    for k in (200, -200):
        s = np.ldexp(1.0, k)
        As = c.A * s
        assert np.all(As / s == c.A)
        sq = float(np.sum(As * As))
        assert np.isfinite(sq) and sq > np.finfo(np.float64).tiny / 2.0 ** -52
        assert np.min(np.abs(As[As != 0])) ** 2 > np.finfo(np.float64).tiny
