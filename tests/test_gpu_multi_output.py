"""GPU: multi-output losses on the device data path (scs_set_outputs; losses.softmax_ce /
losses.multi_least_squares): K outputs on one dense A that stays on the device.  csrc/multi.hip's
products A X and Aᵀ V (A read once for all K columns), the softmax / least-squares epilogue, the
block weights and the placement of K (K + 1) / 2 weighted Grams into the order-d·K system, and the
three methods on top of them, against exact integer arithmetic, the NumPy restatement of
tests/multi_output_data.py, the oracle on the same closures and the host callback route."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import scsopt
from scsopt import _lib, losses

import multi_output_data as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
HM = lambda: scsopt.PHuberSmootherL1L2(0.5)      # noqa: E731
OHM = lambda: O.PHuberSmootherL1L2(0.5)          # noqa: E731
METHODS = {"ggn": (scsopt.ProxGGNSCORE, O.ProxGGNSCORE), "nscore": (scsopt.ProxNSCORE, O.ProxNSCORE),
           "lqn": (lambda **kw: scsopt.ProxLQNSCORE(m=5, **kw), lambda **kw: O.ProxLQNSCORE(m=5, **kw))}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_problem(kind, A, Y, x0, lam, c, **kw):
    f, out_fn = M.device_losses(losses, kind, Y.shape[1], c)
    return scsopt.Problem(A, Y, x0, f, lam, out_fn=out_fn, **kw)


# ---------------------------------------------------------------------------------------------
# 1. exact products
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("d", [1, 127, 129, 260])
@pytest.mark.parametrize("N", [1, 17, 4097, 16400])
def test_products_exact_integers(N, d, f32):
    """Integer data in the ranges of tests/exact_data.py (A in ±8191, X and V in ±1000; Σ|terms| < 2^53
    asserted): every product and partial sum is an integer double in any summation order, so
    scs_multi_products_eval must return A X and Aᵀ V of the int64 reference bit for bit.  N: one row,
    one partial stage block, one row past a 4096-row chunk, a fifth chunk with a ragged tail; d: one
    column, one short of / one past a 128-column panel, a third panel.  K = 1, 2, 3, 16 on one
    context.  The entries of A are exact in fp32 (13 bits), so both storage types give the same bits."""
    rng = np.random.default_rng(1000003 * d + N)
    Ai = rng.integers(-8191, 8192, size=(N, d), dtype=np.int64)
    A = Ai.astype(np.float32 if f32 else np.float64)
    p = scsopt.Problem(A, np.zeros(N), np.zeros(d), losses.least_squares(), 1.0, dense_f32=f32)
    assert p.data_info()[0] == (4 if f32 else 8)
    for K in (1, 2, 3, 16):
        Xi = rng.integers(-1000, 1001, size=(d, K), dtype=np.int64)
        Vi = rng.integers(-1000, 1001, size=(N, K), dtype=np.int64)
        assert int((np.abs(Ai) @ np.abs(Xi)).max()) < 2 ** 53 and int((np.abs(Ai).T @ np.abs(Vi)).max()) < 2 ** 53
        ax, atv = p.multi_products(Xi.astype(np.float64), Vi.astype(np.float64))
        assert np.array_equal(bits(ax), bits((Ai @ Xi).astype(np.float64))), (K, "A X")
        assert np.array_equal(bits(atv), bits((Ai.T @ Vi).astype(np.float64))), (K, "A' V")
    p.ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. exact placement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(1, 2), (1, 3), (127, 2), (127, 3), (129, 2), (129, 3), (260, 2), (260, 3), (33, 16)])
def test_placement_exact_multi_ls(d, K):
    """Multi-target least squares, scale 1, integer A (±8191, N = 300: Σ|terms| <= 300·8191² < 2^53):
    scs_multi_system_eval returns AᵀA of the int64 reference in every diagonal block bit for bit and
    +0.0 in every off-diagonal block, and writes nothing beyond order d·K (the host matrix has a
    larger leading dimension and spare columns, filled with a sentinel)."""
    N = 300
    rng = np.random.default_rng(7 * d + K)
    Ai = rng.integers(-8191, 8192, size=(N, d), dtype=np.int64)
    Y = rng.integers(-5, 6, size=(N, K)).astype(np.float64)
    x = rng.integers(-1, 2, size=d * K).astype(np.float64)    # |A X - Y| <= 260·8191 + 5: Σ res² < 2^53
    p = device_problem("multi_least_squares", Ai.astype(np.float64), Y, x, 1e-3, 1.0)
    m = d * K
    ldg, ncol = m + 3, m + 2
    G = np.full(ldg * ncol, -7.25)
    g = np.empty(m)
    f = C.c_double()
    p.ctx.check(_lib.lib.scs_multi_system_eval(p.ctx.h, _lib.dptr(x), _lib.dptr(G), ldg, _lib.dptr(g), C.byref(f)))
    G = G.reshape(ncol, ldg).T            # column-major: G[i, j]
    assert np.all(G[m:, :] == -7.25) and np.all(G[:, m:] == -7.25)
    ref = (Ai.T @ Ai).astype(np.float64)
    for k in range(K):
        for l in range(K):
            blk = G[k * d:(k + 1) * d, l * d:(l + 1) * d]
            want = ref if k == l else np.zeros((d, d))
            assert np.array_equal(bits(blk), bits(want)), (k, l)
    # the residual side on the same integers: R = A X - Y and Aᵀ R are exact too
    Xi = x.reshape(d, K, order="F").astype(np.int64)
    Ri = Ai @ Xi - Y.astype(np.int64)
    assert np.array_equal(bits(g), bits((Ai.T @ Ri).ravel(order="F").astype(np.float64)))
    assert f.value == 0.5 * float(np.sum(Ri * Ri))
    p.ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. softmax epilogue and system against NumPy
# ---------------------------------------------------------------------------------------------
def _softmax_bounds(A, Y, X, c):
    """Bounds for f, R, vec(AᵀR) and the system, derived (not fitted).
    z: the device sums A X in another order than NumPy: |δz_ik| <= 1e-13·(|A||X|)_ik, the project's
    product bound (test_gpu_parity.py); τ_i = 2 max_k |δz_ik| + (K + 8) ε covers exp of a shifted logit
    (argument error |δz| twice: the logit and the row maximum; 1 ulp of exp; K additions and one division
    for P).  So |δP_ik| <= P_ik τ_i, |δlog P_ik| <= τ_i + 4 ε |log P_ik|, and
      R = c (s P - Y):           |δR_ik| <= c (s_i P_ik + |Y_ik|) (τ_i + 4 ε)
      f = -c Σ Y log P:          |δf|    <= c Σ |Y_ik| (τ_i + (4 + 2 log2(N K)) ε |log P_ik|)
      g = vec(AᵀR):              |δg_jl| <= 1e-13 (|A|ᵀ|R|)_jl + (|A|ᵀ|δR|)_jl
      w_kl = c s (δ_kl P_k - P_k P_l): |δw| <= w̄_kl (2 τ_i + 6 ε), w̄_kl = c s (δ_kl P_k + P_k P_l)
      G_kl = Aᵀ diag(w_kl) A:    |δG|    <= (1e-13 + 2 τ + 6 ε) |A|ᵀ diag(w̄_kl) |A|, τ = max τ_i
    (1e-13·Σ|terms| is the project's Gram bound)."""
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


def _check_softmax_system(A, Y, x0, c, need_R=False):
    N, K = Y.shape
    d = A.shape[1]
    p = device_problem("softmax_ce", A, Y, x0, 1e-3, c)
    G, g, f = p.multi_system(x0)
    p.ctx.close()
    cl = M.closures("softmax_ce", d, K, c)
    X = x0.reshape(d, K, order="F")
    R, dR, df, dg, tau, P, s = _softmax_bounds(A, Y, X, c)
    f_ref, g_ref, H_ref = cl["f"](A, Y, x0), cl["grad_fx"](A, Y, x0), cl["hess_fx"](A, Y, x0)
    assert np.isfinite(f) and np.all(np.isfinite(g)) and np.all(np.isfinite(G))
    print(f"N={N} d={d} K={K}: |f err| {abs(f - f_ref):.3e} (bound {df:.3e}), max g err / bound "
          f"{float(np.max(np.abs(g - g_ref) / (dg.ravel(order='F') + 1e-300))):.3e}")
    assert abs(f - f_ref) <= df
    assert np.all(np.abs(g - g_ref) <= dg.ravel(order="F"))
    absA = np.abs(A)
    worst = 0.0
    for k in range(K):
        for l in range(K):
            wbar = c * s * ((P[:, k] if k == l else 0.0) + P[:, k] * P[:, l])
            T = absA.T @ (wbar[:, None] * absA)
            err = np.abs(G[k * d:(k + 1) * d, l * d:(l + 1) * d] - H_ref[k * d:(k + 1) * d, l * d:(l + 1) * d])
            bound = (1e-13 + 2 * tau + 6 * EPS) * T
            worst = max(worst, float(np.max(err / (bound + 1e-300))))
            assert np.all(err <= bound), (k, l)
    print(f"   max G err / bound {worst:.3e}")
    assert np.array_equal(G, G.T)       # placed as blocks (k, l) and (l, k) of one symmetric Gram
    if need_R:                          # A = I: vec(AᵀR) is R itself
        assert np.all(np.abs(g.reshape(N, K, order="F") - R) <= dR)
    return f, g, G


@pytest.mark.parametrize("K", [2, 3, 7, 16])
@pytest.mark.parametrize("d", [17, 129])
@pytest.mark.parametrize("N", [1, 17, 300])
def test_softmax_system_vs_numpy(N, d, K):
    """f, vec(AᵀR) and the assembled system from scs_multi_system_eval against the helper's NumPy at
    x0 != 0 (a swapped k / l index changes the off-diagonal blocks there), bounds of _softmax_bounds."""
    A, Y, x0 = M.problem(N, d, K)
    _check_softmax_system(A, Y, x0, 1.0 / N)


def test_softmax_saturated_logits_stay_finite():
    """Logits of ±700 (exp(700) overflows a naive softmax; exp(-1400) underflows): with the row maximum
    subtracted P, f and R are finite.  A = I (N = d = 24), so Z = X exactly and vec(AᵀR) = R."""
    N = d = 24
    K = 3
    rng = np.random.default_rng(3)
    X = rng.choice([-700.0, 700.0, 0.5, -0.25], size=(d, K))
    X[0] = [700.0, -700.0, 700.0]      # a tie at the maximum and a far loser
    X[1] = [-700.0, -700.0, -700.0]    # all equal and very negative
    Y = np.eye(K)[rng.integers(0, K, size=N)]
    Y[0] = [0.0, 1.0, 0.0]             # the label on the class with P = exp(-1400) = 0: log P = -1400, finite
    f, g, G = _check_softmax_system(np.eye(N), Y, X.ravel(order="F"), 1.0 / N, need_R=True)
    assert f > 1400.0 / N


def test_softmax_soft_labels():
    """Rows of Y that do not sum to 1 (s_i in [0.5, 1.5]): R = c (s_i P - Y) and Q_i = c s_i (...)."""
    A, Y, x0 = M.problem(300, 17, 7, soft=True)
    assert np.all(np.abs(Y.sum(axis=1) - 1.0) > 1e-3)
    _check_softmax_system(A, Y, x0, 1.0 / 300)
    N = 17
    A, Y, x0 = M.problem(N, N, 3, soft=True)
    _check_softmax_system(np.eye(N), Y, x0, 1.0 / N, need_R=True)


# ---------------------------------------------------------------------------------------------
# 4. trajectories against the oracle
# ---------------------------------------------------------------------------------------------
SHAPES = [(300, 130, 3), (200, 17, 7), (520, 129, 2), (40, 33, 16)]


@functools.lru_cache(maxsize=None)
def _oracle(kind, method, shape, lam, ss_type=1, test=False):
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    kw = {}
    if test:
        At, Yt, _ = M.problem(77, d, K, soft=True)
        kw = dict(Atest=At, ytest=Yt)
    om = O.Problem(A, Y, x0, M.oracle_loss(O, kind, d, K, 1.0 / N), lam, **kw)
    return O.iterate(METHODS[method][1](ss_type=ss_type), om, "l1", OHM(), max_epoch=6)


def _compare(sol, osol):
    assert np.all(np.isfinite(osol.obj)) and np.all(np.isfinite(osol.x))     # the oracle itself ran clean
    assert sol.epochs == osol.epochs
    np.testing.assert_allclose(sol.obj, osol.obj, rtol=1e-8)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("lam", [2e-3, 2e-2])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("method", ["ggn", "nscore", "lqn"])
@pytest.mark.parametrize("kind", M.KINDS)
def test_trajectory_vs_oracle(kind, method, shape, lam, device_loop):
    """6 epochs, "l1" with PHuberSmootherL1L2(0.5), against the oracle on the helper's closures (the
    tolerances of test_ggn_callback_multioutput_softmax_vs_oracle).  Every shape has N K + 1 > d K
    (the feature branch).  (300, 130, 3): two column panels, N no multiple of 16; (200, 17, 7): odd K;
    (520, 129, 2): one column past a panel; (40, 33, 16): the largest K, 136 Grams per step."""
    N, d, K = shape
    assert N * K + 1 > d * K
    A, Y, x0 = M.problem(N, d, K)
    osol = _oracle(kind, method, shape, lam)
    p = device_problem(kind, A, Y, x0, lam, 1.0 / N)
    sol = scsopt.iterate(METHODS[method][0](), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    p.ctx.close()
    _compare(sol, osol)
    if kind == "softmax_ce" and lam == 2e-2 and method != "lqn":   # the prox support is not trivial
        zeros = int(np.sum(sol.x == 0.0))
        assert 0 < zeros < d * K, zeros


def test_nscore_and_ggn_build_the_same_system():
    """∇²f = JᵀQJ for these losses: ProxNSCORE and ProxGGNSCORE take the same steps (1e-14)."""
    N, d, K = SHAPES[0]
    A, Y, x0 = M.problem(N, d, K)
    sols = []
    for meth in (scsopt.ProxNSCORE, scsopt.ProxGGNSCORE):
        p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
        sols.append(scsopt.iterate(meth(), p, "l1", HM(), max_epoch=6, verbose=0))
        p.ctx.close()
    np.testing.assert_allclose(sols[0].x, sols[1].x, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(sols[0].obj, sols[1].obj, rtol=1e-14)


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("kind,method,ss_type,shape", [
    ("softmax_ce", "lqn", 2, (200, 17, 7)),            # the Barzilai-Borwein step: ∇q at x_prev
    ("softmax_ce", "nscore", 3, (520, 129, 2)),        # the line search on N x K trial products
    ("multi_least_squares", "lqn", 3, (300, 130, 3)),
])
def test_trajectory_step_size_rules(kind, method, ss_type, shape, device_loop):
    """ss_type 2 and 3 (the fixed rule 1 is the trajectory matrix above).  ProxNSCORE / ProxGGNSCORE
    raise the reference's MethodError at ss_type 2 from the second step on, and ProxGGNSCORE's ss_type 3
    needs a one-argument grad_fx the oracle's data closures do not have: those stay with the
    single-output tests."""
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    osol = _oracle(kind, method, shape, 2e-3, ss_type)
    p = device_problem(kind, A, Y, x0, 2e-3, 1.0 / N)
    sol = scsopt.iterate(METHODS[method][0](ss_type=ss_type), p, "l1", HM(), max_epoch=6, verbose=0,
                         device_loop=device_loop)
    p.ctx.close()
    _compare(sol, osol)


def test_ggn_line_search_runs():
    """ProxGGNSCORE ss_type 3 on the device kind (grad_f is the device's own): equal to ProxNSCORE's."""
    N, d, K = 200, 17, 7
    A, Y, x0 = M.problem(N, d, K)
    out = []
    for meth in (scsopt.ProxGGNSCORE, scsopt.ProxNSCORE):
        p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
        out.append(scsopt.iterate(meth(ss_type=3), p, "l1", HM(), max_epoch=4, verbose=0))
        p.ctx.close()
    np.testing.assert_allclose(out[0].x, out[1].x, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------------
# 5. against the host callback route
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,method", [("softmax_ce", "ggn"), ("softmax_ce", "nscore"),
                                         ("multi_least_squares", "nscore"), ("softmax_ce", "lqn")])
def test_matches_the_callback_route(kind, method):
    """The same closures through losses.callback (J = I ⊗ A materialised on the host) on (200, 17, 7)."""
    N, d, K = 200, 17, 7
    A, Y, x0 = M.problem(N, d, K)
    pc = scsopt.Problem(A, Y, x0, M.callback_loss(losses, kind, d, K, 1.0 / N), 2e-3)
    ref = scsopt.iterate(METHODS[method][0](), pc, "l1", HM(), max_epoch=6, verbose=0)
    pc.ctx.close()
    p = device_problem(kind, A, Y, x0, 2e-3, 1.0 / N)
    sol = scsopt.iterate(METHODS[method][0](), p, "l1", HM(), max_epoch=6, verbose=0)
    p.ctx.close()
    _compare(sol, ref)


# ---------------------------------------------------------------------------------------------
# 6. fp32 storage, 7. the device door
# ---------------------------------------------------------------------------------------------
def _same_bits(a, b):
    assert a.epochs == b.epochs
    for name in ("x", "obj", "fval"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert np.array_equal(bits(a.pri_res_norm[1:]), bits(b.pri_res_norm[1:]))


@pytest.mark.parametrize("method", ["ggn", "nscore", "lqn"])
def test_dense_f32_equals_widened_values(method):
    """DESIGN §2b's contract on the new kernels: an fp32-stored context gives, bit for bit, the
    histories and x of an fp64-stored context holding the same values widened."""
    N, d, K = 300, 130, 3
    A, Y, x0 = M.problem(N, d, K)
    A32 = A.astype(np.float32)
    sols = []
    for Ain, f32 in ((A32, True), (A32.astype(np.float64), False)):
        p = device_problem("softmax_ce", Ain, Y, x0, 2e-3, 1.0 / N, dense_f32=f32)
        assert p.data_info()[0] == (4 if f32 else 8)
        sols.append(scsopt.iterate(METHODS[method][0](), p, "l1", HM(), max_epoch=5, verbose=0))
        p.ctx.close()
    _same_bits(sols[0], sols[1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("layout", ["row", "col"])
def test_device_door_equals_host_door(layout, dtype):
    """A torch A on the GPU (row- and column-major, fp64 and fp32; Y on the host, and once more on the
    device, column-major) gives bit for bit the host door's system and trajectory."""
    N, d, K = 300, 130, 3
    A, Y, x0 = M.problem(N, d, K)
    Ah = A.astype(np.float32).astype(np.float64) if dtype == torch.float32 else A
    ph = device_problem("softmax_ce", Ah, Y, x0, 2e-3, 1.0 / N)
    Gh, gh, fh = ph.multi_system(x0)
    sh = scsopt.iterate(scsopt.ProxGGNSCORE(), ph, "l1", HM(), max_epoch=3, verbose=0)
    ph.ctx.close()
    At = torch.from_numpy(Ah).to(dtype)
    At = At.cuda() if layout == "row" else At.t().contiguous().cuda().t()
    assert tuple(At.shape) == (N, d) and At.stride() == ((d, 1) if layout == "row" else (1, N))
    Yd = torch.from_numpy(np.ascontiguousarray(Y.T)).cuda().t()          # N x K, strides (1, N)
    for Yin in (Y, Yd):
        pd = device_problem("softmax_ce", At, Yin, x0, 2e-3, 1.0 / N)
        Gd, gd, fd = pd.multi_system(x0)
        assert fd == fh and np.array_equal(bits(gd), bits(gh)) and np.array_equal(bits(Gd), bits(Gh))
        sd = scsopt.iterate(scsopt.ProxGGNSCORE(), pd, "l1", HM(), max_epoch=3, verbose=0)
        pd.ctx.close()
        _same_bits(sd, sh)


# ---------------------------------------------------------------------------------------------
# 8. the held-out set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("kind", M.KINDS)
def test_heldout_fvaltest_vs_oracle(kind, device_loop):
    """Atest / ytest (77 x K soft labels): fvaltest of every pushed point against the oracle, rtol 1e-8."""
    shape = (200, 17, 7)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    At, Yt, _ = M.problem(77, d, K, soft=True)
    osol = _oracle(kind, "ggn", shape, 2e-3, 1, True)
    p = device_problem(kind, A, Y, x0, 2e-3, 1.0 / N, Atest=At, ytest=Yt)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    assert p.ftest(x0) == pytest.approx(M.closures(kind, d, K, 1.0 / N)["f"](At, Yt, x0), rel=1e-12)
    p.ctx.close()
    _compare(sol, osol)
    assert len(sol.fvaltest) == len(sol.obj) == len(osol.fvaltest)
    np.testing.assert_allclose(sol.fvaltest, osol.fvaltest, rtol=1e-8)


# ---------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_name_the_option():
    import scipy.sparse as sp
    N, d, K = 60, 9, 3
    A, Y, x0 = M.problem(N, d, K)
    f, of = M.device_losses(losses, "softmax_ce", K, 1.0 / N)
    with pytest.raises(ValueError, match="sparse A"):
        scsopt.Problem(sp.csr_matrix(A), Y, x0, f, 1e-3, out_fn=of)
    with pytest.raises(ValueError, match="sparse A"):
        scsopt.Problem(torch.from_numpy(A).cuda().to_sparse_csr(), Y, x0, f, 1e-3, out_fn=of)
    with pytest.raises(ValueError, match=r"devices=\[\.\.\.\]"):
        scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of, devices=[0, 0], device_exchange="host")
    for other in (losses.least_squares(1.0 / N), losses.quadratic(), losses.rosenbrock(),
                  losses.samplewise(lambda z, y: z), losses.callback(lambda A, y, x: 0.0)):
        with pytest.raises(ValueError, match="nout"):
            scsopt.Problem(A, Y, x0, other, 1e-3, out_fn=of)
    with pytest.raises(ValueError, match="nout"):
        losses.softmax_ce(17)
    with pytest.raises(ValueError, match="not A.shape"):
        scsopt.Problem(A, Y, x0[:-1], f, 1e-3, out_fn=of)
    with pytest.raises(ValueError, match="N x nout"):
        scsopt.Problem(A, Y[:, :2], x0, f, 1e-3, out_fn=of)
    # the library's own refusals (SCS_ERR_ARG), through a bare context
    ctx = _lib.Context(0)
    for bad in (1, 17, -2):
        with pytest.raises(scsopt.ScsError, match=r"outside 2\.\.16"):
            ctx.check(_lib.lib.scs_set_outputs(ctx.h, bad))
    ctx.check(_lib.lib.scs_set_outputs(ctx.h, K))
    nout, nvar = C.c_int(), C.c_int64()
    ctx.check(_lib.lib.scs_get_outputs(ctx.h, C.byref(nout), C.byref(nvar)))
    assert nout.value == K
    for kind in ("samplewise", "callback", "quadratic", "rosenbrock", "least_squares"):
        with pytest.raises(scsopt.ScsError, match=rf"scs_set_outputs.*{kind}"):
            ctx.check(_lib.lib.scs_set_loss(ctx.h, _lib.LOSS[kind], 0, 1.0))
    cb = _lib.ALLREDUCE_FN(lambda buf, n, st, user: 0)
    with pytest.raises(scsopt.ScsError, match="nranks > 1"):
        ctx.check(_lib.lib.scs_set_comm(ctx.h, 0, 2, cb, None))
    csr = sp.csr_matrix(A)
    csc = sp.csc_matrix(A)
    i64, i32 = _lib.c_i64p, _lib.c_i32p
    arrs = [np.ascontiguousarray(csr.indptr, dtype=np.int64), np.ascontiguousarray(csr.indices, dtype=np.int32),
            np.ascontiguousarray(csr.data), np.ascontiguousarray(csc.indptr, dtype=np.int64),
            np.ascontiguousarray(csc.indices, dtype=np.int32), np.ascontiguousarray(csc.data)]
    yv = np.zeros(N)
    with pytest.raises(scsopt.ScsError, match="sparse A"):
        ctx.check(_lib.lib.scs_set_sparse(ctx.h, N, d, csr.nnz, arrs[0].ctypes.data_as(i64), arrs[1].ctypes.data_as(i32),
                                          _lib.dptr(arrs[2]), arrs[3].ctypes.data_as(i64), arrs[4].ctypes.data_as(i32),
                                          _lib.dptr(arrs[5]), 0, _lib.dptr(yv), N, 0))
    ctx.close()
    # minibatches
    p = scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of)
    for kw in (dict(batch_size=20), dict(slice_samples=True)):
        with pytest.raises(scsopt.ScsError, match="batch_size / slice_samples"):
            scsopt.iterate(scsopt.ProxLQNSCORE(m=3), p, "l1", HM(), max_epoch=2, verbose=0, **kw)
    # the single-vector kernel doors
    with pytest.raises(scsopt.ScsError, match="scs_gemv_t_eval"):
        p.gemv_t(np.zeros(N))
    p.ctx.close()


@pytest.mark.parametrize("device_loop", [False, True])
def test_ggn_sample_space_shape_is_refused(device_loop):
    """(N, d, K) = (20, 30, 3): N K + 1 = 61 <= d K = 90, where the reference's ProxGGNSCORE takes its
    sample-space branch (another step).  Refused with a pointer to losses.callback, not silently run
    in the feature branch; ProxLQNSCORE on the same problem runs (against the oracle)."""
    N, d, K = 20, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
    with pytest.raises(scsopt.ScsError, match=r"sample-space branch.*losses\.callback"):
        scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=3, verbose=0, device_loop=device_loop)
    sol = scsopt.iterate(scsopt.ProxLQNSCORE(m=5), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    p.ctx.close()
    _compare(sol, _oracle("softmax_ce", "lqn", (N, d, K), 2e-3))


# ---------------------------------------------------------------------------------------------
# 10. no drift without nout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("method", ["ggn", "nscore", "lqn"])
def test_no_drift_without_outputs(method, device_loop):
    """A context with nout never set reproduces bit for bit the x / obj stored in
    tests/golden/multi_output_no_drift.npz.  Provenance: computed on an MI355X by the commit before
    this feature (e992b36), with exactly the calls below (N = 150, d = 37, 5 epochs, "l1",
    PHuberSmootherL1L2(0.5), λ = 2e-3; the data A, y01, x0 are stored in the file)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "multi_output_no_drift.npz"))
    A, y01, x0 = g["A"], g["y01"], g["x0"]
    N = A.shape[0]
    if method == "ggn":
        meth, p = scsopt.ProxGGNSCORE(), scsopt.Problem(A, y01, x0, losses.logistic_ce(1.0 / N), 2e-3,
                                                        out_fn=losses.sigmoid_ce(1.0 / N))
    elif method == "nscore":
        meth, p = scsopt.ProxNSCORE(), scsopt.Problem(A, 2 * y01 - 1, x0, losses.logistic_margin(1.0 / N), 2e-3)
    else:
        meth, p = scsopt.ProxLQNSCORE(m=5), scsopt.Problem(A, y01, x0, losses.least_squares(1.0 / N), 2e-3)
    s = scsopt.iterate(meth, p, "l1", HM(), max_epoch=5, verbose=0, device_loop=device_loop)
    p.ctx.close()
    assert np.array_equal(bits(s.x), bits(g[f"{method}_x_{int(device_loop)}"]))
    assert np.array_equal(bits(s.obj), bits(g[f"{method}_obj_{int(device_loop)}"]))
