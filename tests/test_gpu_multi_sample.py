"""GPU: ProxGGNSCORE's sample-space branch of a multi-output loss on the device (multi_sample=True /
scs_set_multi_sample).  With N K + 1 <= d K the reference solves the order-(N K + 1) system

    M[(i,k),(j,l)] = δ_ij δ_kl + Q_i[k,l] P_l[i,j]     P_l = A diag(h_l) Aᵀ,  h = 1 ./ Hr
    M[(i,k), n]    = Σ_l Q_i[k,l] u_l[i]               u_l = A (h_l ∘ g_l),   g = λ gr
    M[n, ·]        = e_n,   b = [vec(R); 1]            rows / columns (i, k) = i + N k, n = N K

(block (k, l) carries P_l, the Gram of the COLUMN block).  The assembled system against this formula in
NumPy and against the oracle's own matrix, the exact placement of the blocks, trajectories against the
oracle and the host callback route, both sides of the branch test, the storage types and data doors,
and the refusals."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import scsopt
from scsopt import _lib, losses

import multi_output_data as M
from test_gpu_multi_output import _compare, _same_bits, _softmax_bounds, bits, device_problem

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
HM = lambda: scsopt.PHuberSmootherL1L2(0.5)      # noqa: E731
OHM = lambda: O.PHuberSmootherL1L2(0.5)          # noqa: E731

# (N, d, K), all with N K + 1 <= d K: order 3 | the shape the refusal test of the feature branch uses |
# d one past a panel | n1 = 256, a whole multiple of the pad | N one short of 128, n1 = 382 | two P
# tiles per side, n1 = 259, three LU panels | the largest K, n1 = 257
SHAPES = [(1, 2, 2), (20, 30, 3), (43, 129, 2), (85, 86, 3), (127, 130, 3), (129, 260, 2), (16, 33, 16)]
SENT = -7.25


def _problem(kind, shape, lam, c, soft=False, **kw):
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K, soft=soft)
    return device_problem(kind, A, Y, x0, lam, c, multi_sample=True, **kw), A, Y, x0


# ---------------------------------------------------------------------------------------------
# 1. the system against NumPy
# ---------------------------------------------------------------------------------------------
def _reference_system(kind, A, Y, x0, c, h, g):
    """The block formula above in NumPy, with its entrywise error bounds (derived, not fitted).

    h = 1 ./ Hr and g = λ gr are formed from the device's own gr / Hr by the same two roundings the
    device applies (1 / Hr; h·(λ·gr)), so they carry no error.  For every entry e = δ + w p:
      p = P_l[i,j]:  |δp| <= 1e-13 (|A| diag(h_l) |A|ᵀ)_ij =: dp, the project's product bound (it also
                     covers NumPy's own summation error, d ε <= 260 ε < 1e-13);
      w = Q_i[k,l]:  |δw| <= w̄ (2 τ + 6 ε) =: dw with w̄ = c s_i (δ_kl P_ik + P_ik P_il) and τ of
                     _softmax_bounds (the feature branch's bound on the same arithmetic); the multi-target
                     least squares has w = c δ_kl exactly, dw = 0;
      the device rounds the product and the add once each (no contraction): 2 ε (δ + (|w| + dw)(|p| + dp)).
    So |δe| <= dw (|p| + dp) + |w| dp + 2 ε (δ + (|w| + dw)(|p| + dp)).
    Last column e = Σ_l w_kl u_l, |δu_l| <= 1e-13 (|A| |h_l ∘ g_l|)_i =: du: the same two terms per l plus
    (K + 1) ε Σ_l (|w| + dw)(|u_l| + du) for the K products and K - 1 additions (fused or not).
    b = vec(R): softmax dR of _softmax_bounds; least squares R = c (Z - Y): c (dz + 2 ε (|Z| + |Y|)),
    dz = 1e-13 |A||X|.  The last row and b[n] are exact."""
    N, K = Y.shape
    d = A.shape[1]
    n = N * K
    X = x0.reshape(d, K, order="F")
    Z = A @ X
    absA = np.abs(A)
    Q = M.q_blocks(kind, Y, Z, c)                                   # N x K x K
    if kind == "softmax_ce":
        R, dR, _, _, tau, P, s = _softmax_bounds(A, Y, X, c)
        wbar = c * s[:, None, None] * (P[:, :, None] * np.eye(K)[None] + P[:, :, None] * P[:, None, :])
        dW = wbar * (2 * tau + 6 * EPS)
    else:
        R = c * (Z - Y)
        dR = c * (1e-13 * (absA @ np.abs(X)) + 2 * EPS * (np.abs(Z) + np.abs(Y)))
        dW = np.zeros_like(Q)
    Mr = np.zeros((n + 1, n + 1))
    dM = np.zeros((n + 1, n + 1))
    hl = h.reshape(d, K, order="F")
    hg = (h * g).reshape(d, K, order="F")
    U = A @ hg                                                      # N x K
    dU = 1e-13 * (absA @ np.abs(hg))
    for l in range(K):
        Pl = (A * hl[:, l][None, :]) @ A.T
        dp = 1e-13 * ((absA * hl[:, l][None, :]) @ absA.T)
        q = np.abs(Pl) + dp
        for k in range(K):
            w, dw = Q[:, k, l][:, None], dW[:, k, l][:, None]
            blk = w * Pl
            delta = np.eye(N) if k == l else 0.0
            Mr[k * N:(k + 1) * N, l * N:(l + 1) * N] = delta + blk
            dM[k * N:(k + 1) * N, l * N:(l + 1) * N] = (dw * q + np.abs(w) * dp
                                                        + 2 * EPS * (delta + (np.abs(w) + dw) * q))
    for k in range(K):
        aw = np.abs(Q[:, k, :]) + dW[:, k, :]
        qu = np.abs(U) + dU
        Mr[k * N:(k + 1) * N, n] = np.sum(Q[:, k, :] * U, axis=1)
        dM[k * N:(k + 1) * N, n] = np.sum(dW[:, k, :] * qu + np.abs(Q[:, k, :]) * dU, axis=1) \
            + (K + 1) * EPS * np.sum(aw * qu, axis=1)
    Mr[n, n] = 1.0
    br = np.concatenate([R.ravel(order="F"), [1.0]])
    db = np.concatenate([dR.ravel(order="F"), [0.0]])
    return Mr, dM, br, db


def _oracle_matrix(kind, A, Y, x0, c, lam, gr, Hr):
    """The matrix ggn_score_step_general forms in its sample branch (its own three lines), and its
    direction from the function itself."""
    N, K = Y.shape
    d = A.shape[1]
    cl = M.closures(kind, d, K, c)
    Z = cl["out_fn"](A, x0)
    J = cl["jac_yx"](A, Y, Z, x0)
    Qm = cl["hess_fy"](A, Y, Z)
    r = cl["grad_fy"](A, Y, Z)
    lgr = lam * gr
    nq = J.shape[0]
    assert nq + 1 <= J.shape[1]                                      # the oracle takes its sample branch
    Jt = np.hstack([J.T, lgr[:, None]])
    Qp = np.zeros((nq + 1, nq + 1))
    Qp[:nq, :nq] = Qm
    Mo = np.eye(nq + 1) + Qp @ ((Jt.T * (1.0 / Hr)[None, :]) @ Jt)
    dirn = O.ggn_score_step_general(J, Qm, r, lgr, Hr, lam)
    return Mo, dirn


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", M.KINDS)
def test_system_vs_numpy(kind, shape, soft):
    """multi_sample_system(x0) at scale c = 1 (at c = 1/N the system is I + tiny and a wrong block hides)
    against the block formula within the bounds of _reference_system; the formula against the oracle's
    matrix and direction; nothing written beyond order n1; the last row exactly e_n."""
    N, d, K = shape
    lam, c = 2e-3, 1.0
    p, A, Y, x0 = _problem(kind, shape, lam, c, soft=soft)
    if soft:
        assert N == 1 or np.all(np.abs(Y.sum(axis=1) - 1.0) > 1e-3)
    p.configure("l1", HM())
    gr, Hr = p._smoother_eval(HM(), x0)
    n1 = N * K + 1
    ldm, ncol = n1 + 3, n1 + 2
    buf = np.full(ldm * ncol, SENT)
    b = np.full(n1 + 2, SENT)
    p.ctx.check(_lib.lib.scs_multi_sample_system_eval(p.ctx.h, _lib.dptr(x0), _lib.dptr(buf), ldm, _lib.dptr(b)))
    Mm2, b2 = p.multi_sample_system(x0)
    p.ctx.close()
    G = buf.reshape(ncol, ldm).T                                     # column-major: G[i, j]
    assert np.all(G[n1:, :] == SENT) and np.all(G[:, n1:] == SENT) and np.all(b[n1:] == SENT)
    Md, bd = G[:n1, :n1], b[:n1]
    assert np.array_equal(bits(Md), bits(Mm2)) and np.array_equal(bits(bd), bits(b2))   # the same call twice
    e_n = np.zeros(n1)
    e_n[-1] = 1.0
    assert np.array_equal(bits(Md[-1]), bits(e_n)) and bd[-1] == 1.0
    h = 1.0 / Hr
    g = lam * gr
    Mr, dM, br, db = _reference_system(kind, A, Y, x0, c, h, g)
    errM, errb = np.abs(Md - Mr), np.abs(bd - br)
    print(f"{kind} {shape} soft={soft}: max M err / bound {float(np.max(errM / (dM + 1e-300))):.3e}, "
          f"max b err / bound {float(np.max(errb / (db + 1e-300))):.3e}, cond {np.linalg.cond(Mr):.3g}")
    assert np.all(np.isfinite(Md)) and np.all(np.isfinite(bd))
    assert np.all(errM <= dM)
    assert np.all(errb <= db)
    # the formula is the oracle's matrix (to rounding of two different summation orders) ...
    Mo, dirn = _oracle_matrix(kind, A, Y, x0, c, lam, gr, Hr)
    scale = np.abs(Mr).max()
    np.testing.assert_allclose(Mr, Mo, rtol=0, atol=1e-12 * scale)
    # ... and gives the oracle's direction: d_l = -h_l ∘ (Aᵀ B_l + g_l B[n])
    B = np.linalg.solve(Mr, br)
    V = B[:-1].reshape(N, K, order="F")
    dref = -(h * ((A.T @ V).ravel(order="F") + g * B[-1]))
    np.testing.assert_allclose(dref, dirn, rtol=1e-9, atol=1e-12 * np.abs(dirn).max())


def test_column_block_gram_is_visible():
    """The check above sees P_k in place of P_l: on (20, 30, 3), softmax, c = 1, the wrong formula leaves
    the bound by orders of magnitude in an off-diagonal block (a guard of the test itself)."""
    N, d, K = 20, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    rng = np.random.default_rng(0)
    h = 1.0 / (1.0 + rng.random(d * K))
    g = 2e-3 * rng.standard_normal(d * K)
    Mr, dM, _, _ = _reference_system("softmax_ce", A, Y, x0, 1.0, h, g)
    Q = M.q_blocks("softmax_ce", Y, A @ x0.reshape(d, K, order="F"), 1.0)
    hl = h.reshape(d, K, order="F")
    k, l = 0, 1
    wrong = Q[:, k, l][:, None] * ((A * hl[:, k][None, :]) @ A.T)
    blk = slice(k * N, (k + 1) * N), slice(l * N, (l + 1) * N)
    assert np.max(np.abs(wrong - Mr[blk]) / dM[blk]) > 1e6


# ---------------------------------------------------------------------------------------------
# 2. exact placement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(43, 129, 2), (129, 260, 2), (16, 33, 16)])
def test_placement_exact_multi_ls(shape):
    """Multi-target least squares, c = 1: Q_i = I, so every off-diagonal block (k != l) is exactly +0.0
    and block (k, k) is, bit for bit, δ_ij + P_k[i,j] with P_k from scs_sample_gram_eval(h_k) on a
    single-output context holding the same A -- the same Gram launch, and 1·p is exact."""
    N, d, K = shape
    lam = 2e-3
    p, A, Y, x0 = _problem("multi_least_squares", shape, lam, 1.0)
    p.configure("l1", HM())
    _, Hr = p._smoother_eval(HM(), x0)
    Mm, _ = p.multi_sample_system(x0)
    p.ctx.close()
    h = (1.0 / Hr).reshape(d, K, order="F")
    p1 = scsopt.Problem(A, np.zeros(N), np.zeros(d), losses.least_squares(), 1.0)
    for k in range(K):
        Pk = p1.sample_gram(np.ascontiguousarray(h[:, k]))
        assert np.array_equal(Pk, Pk.T)
        for l in range(K):
            blk = Mm[k * N:(k + 1) * N, l * N:(l + 1) * N]
            want = np.eye(N) + Pk if k == l else np.zeros((N, N))
            assert np.array_equal(bits(blk), bits(want)), (k, l)
    p1.ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. trajectories against the oracle
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(kind, shape, lam, cn, ss_type=1, test=False):
    """cn: the scale is 1 (False) or 1/N (True)."""
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    c = 1.0 / N if cn else 1.0
    kw = {}
    if test:
        At, Yt, _ = M.problem(77, d, K, soft=True)
        kw = dict(Atest=At, ytest=Yt)
    loss = M.oracle_loss(O, kind, d, K, c)
    if ss_type == 3:
        # ProxGGNSCORE's line search calls model.grad_fx(x) with x alone (prox-GGN-SCORE.jl:58-59): the
        # closure takes both forms here, the data it closes over being the problem's own
        g3 = loss._g
        loss._g = lambda *a: g3(*a) if len(a) == 3 else g3(A, Y, a[0])
    om = O.Problem(A, Y, x0, loss, lam, **kw)
    return O.iterate(O.ProxGGNSCORE(ss_type=ss_type), om, "l1", OHM(), max_epoch=6)


def _run(kind, shape, lam, cn, device_loop=False, ss_type=1, solver=None, test=False, **kw):
    N, d, K = shape
    c = 1.0 / N if cn else 1.0
    if test:
        At, Yt, _ = M.problem(77, d, K, soft=True)
        kw.update(Atest=At, ytest=Yt)
    p, A, Y, x0 = _problem(kind, shape, lam, c, **kw)
    if solver:
        p.set_solver(solver)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(ss_type=ss_type), p, "l1", HM(), max_epoch=6, verbose=0,
                         device_loop=device_loop)
    p.ctx.close()
    return sol


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("lam", [2e-3, 2e-2])
@pytest.mark.parametrize("cn", [False, True], ids=["c1", "c1overN"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", M.KINDS)
def test_trajectory_vs_oracle(kind, shape, cn, lam, device_loop):
    """6 epochs of ProxGGNSCORE, "l1" with PHuberSmootherL1L2(0.5), against the oracle on the helper's
    closures (which takes its sample branch on every shape), tolerances of _compare."""
    N, d, K = shape
    assert N * K + 1 <= d * K
    _compare(_run(kind, shape, lam, cn, device_loop), _oracle(kind, shape, lam, cn))


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("kind", M.KINDS)
def test_trajectory_line_search(kind, device_loop):
    """ss_type = 3 on (20, 30, 3): the sample-space direction under the line search."""
    shape = (20, 30, 3)
    _compare(_run(kind, shape, 2e-3, True, device_loop, ss_type=3), _oracle(kind, shape, 2e-3, True, 3))


def test_trajectory_reference_solver():
    """The reference-solver mode (Householder QR of the sample-space system) on (127, 130, 3)."""
    shape = (127, 130, 3)
    _compare(_run("softmax_ce", shape, 2e-3, False, solver="reference"), _oracle("softmax_ce", shape, 2e-3, False))


@pytest.mark.parametrize("device_loop", [False, True])
def test_heldout_fvaltest_vs_oracle(device_loop):
    """Atest / ytest (77 soft-label rows): fvaltest of every pushed point, rtol 1e-8."""
    shape = (20, 30, 3)
    osol = _oracle("softmax_ce", shape, 2e-3, True, 1, True)
    sol = _run("softmax_ce", shape, 2e-3, True, device_loop, test=True)
    _compare(sol, osol)
    assert len(sol.fvaltest) == len(sol.obj) == len(osol.fvaltest)
    np.testing.assert_allclose(sol.fvaltest, osol.fvaltest, rtol=1e-8)


# ---------------------------------------------------------------------------------------------
# 4. against the callback route
# ---------------------------------------------------------------------------------------------
def test_matches_the_callback_route():
    """(20, 30, 3) softmax through losses.callback (J = I ⊗ A uploaded every step) on the same data."""
    shape = (20, 30, 3)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    pc = scsopt.Problem(A, Y, x0, M.callback_loss(losses, "softmax_ce", d, K, 1.0 / N), 2e-3)
    ref = scsopt.iterate(scsopt.ProxGGNSCORE(), pc, "l1", HM(), max_epoch=6, verbose=0)
    pc.ctx.close()
    _compare(_run("softmax_ce", shape, 2e-3, True), ref)


# ---------------------------------------------------------------------------------------------
# 5. both sides of the branch test
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loop", [False, True])
def test_feature_shape_is_unchanged_by_the_switch(device_loop):
    """(30, 30, 3): N K + 1 = 91 > d K = 90 -- the feature branch, bit for bit the run without the switch."""
    N, d, K = 30, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    sols = []
    for on in (False, True):
        p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, multi_sample=on)
        sols.append(scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=6, verbose=0,
                                   device_loop=device_loop))
        p.ctx.close()
    _same_bits(sols[0], sols[1])


@pytest.mark.parametrize("kind", M.KINDS)
def test_first_sample_shape_runs_the_branch(kind):
    """(29, 30, 3): N K + 1 = 88 <= 90 -- the new branch, against the oracle."""
    shape = (29, 30, 3)
    _compare(_run(kind, shape, 2e-3, True), _oracle(kind, shape, 2e-3, True))


# ---------------------------------------------------------------------------------------------
# 6. storage and doors
# ---------------------------------------------------------------------------------------------
def test_dense_f32_equals_widened_values():
    """An fp32-stored context gives, bit for bit, the system and the trajectory of an fp64-stored
    context holding the same values widened."""
    shape = (43, 129, 2)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    A32 = A.astype(np.float32)
    out = []
    for Ain, f32 in ((A32, True), (A32.astype(np.float64), False)):
        p = device_problem("softmax_ce", Ain, Y, x0, 2e-3, 1.0, dense_f32=f32, multi_sample=True)
        assert p.data_info()[0] == (4 if f32 else 8)
        p.configure("l1", HM())
        Mm, b = p.multi_sample_system(x0)
        sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=5, verbose=0)
        p.ctx.close()
        out.append((Mm, b, sol))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    _same_bits(out[0][2], out[1][2])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("layout", ["row", "col"])
def test_device_door_equals_host_door(layout, dtype):
    """A torch A on the GPU (row- and column-major, fp64 and fp32) gives bit for bit the host door's
    system and 3-epoch trajectory."""
    shape = (43, 129, 2)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    Ah = A.astype(np.float32).astype(np.float64) if dtype == torch.float32 else A

    def run(Ain):
        p = device_problem("softmax_ce", Ain, Y, x0, 2e-3, 1.0, multi_sample=True)
        p.configure("l1", HM())
        Mm, b = p.multi_sample_system(x0)
        sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=3, verbose=0)
        p.ctx.close()
        return Mm, b, sol

    Mh, bh, sh = run(Ah)
    At = torch.from_numpy(Ah).to(dtype)
    At = At.cuda() if layout == "row" else At.t().contiguous().cuda().t()
    assert tuple(At.shape) == (N, d) and At.stride() == ((d, 1) if layout == "row" else (1, N))
    Md, bd, sd = run(At)
    assert np.array_equal(bits(Md), bits(Mh)) and np.array_equal(bits(bd), bits(bh))
    _same_bits(sd, sh)


def test_same_call_twice_gives_equal_bits():
    shape = (85, 86, 3)
    a = _run("softmax_ce", shape, 2e-3, False)
    b = _run("softmax_ce", shape, 2e-3, False)
    _same_bits(a, b)


# ---------------------------------------------------------------------------------------------
# 7. refusals and no drift
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loop", [False, True])
def test_switch_off_keeps_the_old_refusal(device_loop):
    N, d, K = 20, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
    with pytest.raises(scsopt.ScsError, match=r"sample-space branch.*losses\.callback"):
        scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=3, verbose=0, device_loop=device_loop)
    # switched on afterwards the same context runs; off again it refuses again
    p.set_multi_sample(True)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    _compare(sol, _oracle("softmax_ce", (N, d, K), 2e-3, True))
    p.set_multi_sample(False)
    with pytest.raises(scsopt.ScsError, match=r"sample-space branch.*losses\.callback"):
        scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=3, verbose=0, device_loop=device_loop)
    p.ctx.close()


def test_sparse_A_is_refused_in_the_sample_shape():
    import scipy.sparse as sp
    N, d, K = 20, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    f, of = M.device_losses(losses, "softmax_ce", K, 1.0 / N)
    p = scsopt.Problem(sp.csr_matrix(A), Y, x0, f, 2e-3, out_fn=of, sparse_outputs=True, multi_sample=True)
    with pytest.raises(scsopt.ScsError, match=r"multi_sample.*dense A"):
        scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=3, verbose=0)
    p.configure("l1", HM())
    with pytest.raises(scsopt.ScsError, match=r"multi_sample.*dense A"):
        p.multi_sample_system(x0)
    # the other methods are unaffected
    sol = scsopt.iterate(scsopt.ProxLQNSCORE(m=5), p, "l1", HM(), max_epoch=3, verbose=0)
    assert np.all(np.isfinite(sol.x))
    p.ctx.close()


def test_door_refusals():
    """The door names its cause: the feature shape, no nout, no switch."""
    N, d, K = 30, 30, 3
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, multi_sample=True)
    p.configure("l1", HM())
    with pytest.raises(scsopt.ScsError, match=r"feature branch"):
        p.multi_sample_system(x0)
    p.ctx.close()
    N = 20
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
    p.configure("l1", HM())
    with pytest.raises(scsopt.ScsError, match=r"multi_sample=True / scs_set_multi_sample"):
        p.multi_sample_system(x0)
    p.ctx.close()
    p = scsopt.Problem(A, Y[:, 0].copy(), x0[:d].copy(), losses.logistic_ce(1.0 / N), 2e-3,
                       out_fn=losses.sigmoid_ce(1.0 / N), multi_sample=True)
    p.configure("l1", HM())
    buf = np.zeros((N + 1) * (N + 1))
    b = np.zeros(N + 1)
    with pytest.raises(scsopt.ScsError, match=r"scs_set_outputs"):
        p.ctx.check(_lib.lib.scs_multi_sample_system_eval(p.ctx.h, _lib.dptr(x0[:d].copy()), _lib.dptr(buf), N + 1,
                                                          _lib.dptr(b)))
    p.ctx.close()


@pytest.mark.parametrize("device_loop", [False, True])
def test_no_drift_without_outputs(device_loop):
    """A single-output context with the switch set: its ProxGGNSCORE sample-space trajectory (N + 1 <= m)
    is bit for bit the one without it."""
    N, d = 40, 130
    rng = np.random.default_rng(11)
    A = rng.standard_normal((N, d)) / np.sqrt(d)
    y01 = (rng.random(N) < 0.5).astype(np.float64)
    x0 = 0.2 * rng.standard_normal(d)
    sols = []
    for on in (False, True):
        p = scsopt.Problem(A, y01, x0, losses.logistic_ce(1.0 / N), 2e-3, out_fn=losses.sigmoid_ce(1.0 / N),
                           multi_sample=on)
        sols.append(scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=5, verbose=0,
                                   device_loop=device_loop))
        p.ctx.close()
    _same_bits(sols[0], sols[1])
