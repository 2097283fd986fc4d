"""GPU: multi-output losses on a sparse A (sparse_outputs=True / scs_set_sparse_outputs).  The products
A X and Aᵀ V with K right-hand sides in one pass over the nonzeros (csrc/multi_sparse.hip) and the loop
arm (SCS_MULTI_SPARSE_KERNEL=0: K launches of the single-vector product), the order-d·K system on the
three Gram routes of a sparse A, and the three methods on top of them -- against exact integer
arithmetic, NumPy on the densified A under the derived bounds, the dense device path, and the oracle.

Edges of the K-column layout (multi_sparse.hip): the sub-block width is min(2^ceil(log2 ncols),
16384 / KP) indices with KP = 2, 4, 16 for K = 2, 3, 16; KP sub-blocks make a 16384-index group; a
workgroup takes 1024 rows, a wave 64.  The exact shapes cross each: (65, 1) a wave; (300, 4200) four
1024-wide sub-blocks at K = 16 and the 4096 edge of K = 3; (300, 16500) / (16500, 300) the 8192 edge of
K = 2, the 16384 group edge and 16 row chunks of 1024 with a ragged 116-row tail, on the CSR and on the
CSC side."""
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
import multi_sparse_data as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

HM = lambda: scsopt.PHuberSmootherL1L2(0.5)      # noqa: E731
OHM = lambda: O.PHuberSmootherL1L2(0.5)          # noqa: E731
METHODS = {"ggn": (scsopt.ProxGGNSCORE, O.ProxGGNSCORE), "nscore": (scsopt.ProxNSCORE, O.ProxNSCORE),
           "lqn": (lambda **kw: scsopt.ProxLQNSCORE(m=5, **kw), lambda **kw: O.ProxLQNSCORE(m=5, **kw))}
ARM_KERNEL = {"0": "spmv_blk_kernel<", "1": "multi_spmm_blk_kernel<"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def sparse_device_problem(kind, A, Y, x0, lam, c, **kw):
    f, out_fn = M.device_losses(losses, kind, Y.shape[1], c)
    return scsopt.Problem(A, Y, x0, f, lam, out_fn=out_fn, sparse_outputs=True, **kw)


def torch_csr(A, idx_dtype=torch.int64, val_dtype=torch.float64):
    """scipy CSR -> torch.sparse_csr_tensor on the GPU."""
    A = A.tocsr()
    return torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)).to(idx_dtype).cuda(),
                                   torch.from_numpy(A.indices.astype(np.int64)).to(idx_dtype).cuda(),
                                   torch.from_numpy(A.data).to(val_dtype).cuda(), size=A.shape)


# ---------------------------------------------------------------------------------------------
# 1. exact products
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["0", "1"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("N,d", S.EXACT_SHAPES)
def test_products_exact_integers(N, d, f32, arm, monkeypatch):
    """Integer data (A in ±4000 with duplicates summed by the door, X and V in ±1000; Σ|terms| < 2^53
    asserted by the generator): scs_multi_products_eval must return the int64 A X and Aᵀ V bit for bit
    on both arms and both storage types, with +0.0 in the empty rows and columns.  kernel_names()
    proves the arm.  K = 2, 3, 16: one context each (the blocked copies are cut for K)."""
    monkeypatch.setenv("SCS_MULTI_SPARSE_KERNEL", arm)
    for K in S.EXACT_K:
        c = S.exact_sparse_case(N, d, K)
        f, of = M.device_losses(losses, "multi_least_squares", K, 1.0)
        p = scsopt.Problem(c.coo, np.zeros((N, K)), np.zeros(d * K), f, 1.0, out_fn=of, sparse_outputs=True,
                           sparse_f32=f32)
        ax, atv = p.multi_products(c.X, c.V)
        name = p.ctx.kernel_names()[1]
        p.ctx.close()
        assert name.startswith(ARM_KERNEL[arm]), name
        if arm == "1":
            assert name.startswith("multi_spmm_blk_kernel<float, 8" if f32 else "multi_spmm_blk_kernel<double, 4"), name
        assert np.array_equal(bits(ax), bits(c.AX.astype(np.float64))), (K, "A X")
        assert np.array_equal(bits(atv), bits(c.ATV.astype(np.float64))), (K, "A' V")
        for r in c.empty_rows:
            assert np.all(bits(ax[r]) == 0), (K, "empty row", r)        # +0.0, not -0.0
        for j in c.empty_cols:
            assert np.all(bits(atv[j]) == 0), (K, "empty column", j)


def test_products_eval_needs_the_mode_and_nout():
    """A sparse context without outputs keeps SCS_ERR_STATE; in the mode K must be the context's nout."""
    c = S.exact_sparse_case(700, 300, 3)
    p = scsopt.Problem(c.coo, np.zeros(700), np.zeros(300), losses.least_squares(), 1.0)
    with pytest.raises(scsopt.ScsError, match="needs a dense A"):
        p.multi_products(c.X, c.V)
    p.ctx.close()
    f, of = M.device_losses(losses, "multi_least_squares", 3, 1.0)
    p = scsopt.Problem(c.coo, np.zeros((700, 3)), np.zeros(900), f, 1.0, out_fn=of, sparse_outputs=True)
    with pytest.raises(scsopt.ScsError, match="K = nout = 3"):
        p.multi_products(np.zeros((300, 2)), None)
    p.ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. exact placement on each Gram route
# ---------------------------------------------------------------------------------------------
ROUTES = {"sparse": (dict(SCS_SPARSE_GRAM="1"), "sparse_gram_"),
          "mirror": (dict(SCS_SPARSE_GRAM="0"), "gram_sia_kernel<"),
          "ring": (dict(SCS_SPARSE_GRAM="0", SCS_SPARSE_MIRROR_MAX_GB="0", SCS_SPARSE_CHUNK_ROWS="48"),
                   "gram_sia_kernel<")}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("N,d,K", S.PLACEMENT_SHAPES)
def test_placement_exact_multi_ls(N, d, K, route, monkeypatch):
    """Multi-target least squares, scale 1, integer sparse A: scs_multi_system_eval returns the int64
    AᵀA in every diagonal block bit for bit, +0.0 elsewhere, and nothing beyond order d·K (sentinel
    around the host matrix) -- on the Gram priced by nonzeros, the dense mirror and the streaming ring
    (48 rows per chunk: 7 chunks), each on the d-column view of the data."""
    env, prefix = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = S.placement_case(N, d, K)
    p = sparse_device_problem("multi_least_squares", c.coo, c.Y, c.x, 1e-3, 1.0)
    m = d * K
    ldg, ncol = m + 3, m + 2
    G = np.full(ldg * ncol, -7.25)
    g = np.empty(m)
    f = C.c_double()
    p.ctx.check(_lib.lib.scs_multi_system_eval(p.ctx.h, _lib.dptr(c.x), _lib.dptr(G), ldg, _lib.dptr(g), C.byref(f)))
    name = p.ctx.kernel_names()[0]
    p.ctx.close()
    assert name.startswith(prefix), name
    G = G.reshape(ncol, ldg).T
    assert np.all(G[m:, :] == -7.25) and np.all(G[:, m:] == -7.25)
    ref = c.G.astype(np.float64)
    for k in range(K):
        for l in range(K):
            blk = G[k * d:(k + 1) * d, l * d:(l + 1) * d]
            want = ref if k == l else np.zeros((d, d))
            assert np.array_equal(bits(blk), bits(want)), (k, l)
    Xi = c.x.reshape(d, K, order="F").astype(np.int64)
    Ri = c.Ai @ Xi - c.Y.astype(np.int64)
    assert np.array_equal(bits(g), bits((c.Ai.T @ Ri).ravel(order="F").astype(np.float64)))
    assert f.value == 0.5 * float(np.sum(Ri * Ri))


# ---------------------------------------------------------------------------------------------
# 3. softmax system against NumPy on the densified A
# ---------------------------------------------------------------------------------------------
def _check_softmax_system(As, Y, x0, c, G, g, f):
    N, K = Y.shape
    A = As.toarray()
    d = A.shape[1]
    cl = M.closures("softmax_ce", d, K, c)
    X = x0.reshape(d, K, order="F")
    R, dR, df, dg, tau, P, s = S.softmax_bounds(A, Y, X, c)
    f_ref, g_ref, H_ref = cl["f"](A, Y, x0), cl["grad_fx"](A, Y, x0), cl["hess_fx"](A, Y, x0)
    assert np.isfinite(f) and np.all(np.isfinite(g)) and np.all(np.isfinite(G))
    print(f"N={N} d={d} K={K}: |f err| {abs(f - f_ref):.3e} (bound {df:.3e}), max g err / bound "
          f"{float(np.max(np.abs(g - g_ref) / (dg.ravel(order='F') + 1e-300))):.3e}")
    assert abs(f - f_ref) <= df
    assert np.all(np.abs(g - g_ref) <= dg.ravel(order="F"))
    worst = 0.0
    for k in range(K):
        for l in range(K):
            err = np.abs(G[k * d:(k + 1) * d, l * d:(l + 1) * d] - H_ref[k * d:(k + 1) * d, l * d:(l + 1) * d])
            bound = S.system_bound(A, P, s, c, tau, k, l)
            worst = max(worst, float(np.max(err / (bound + 1e-300))))
            assert np.all(err <= bound), (k, l)
    print(f"   max G err / bound {worst:.3e}")
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("K", [2, 3, 7, 16])
@pytest.mark.parametrize("d", [17, 129])
@pytest.mark.parametrize("N", [1, 17, 300])
def test_softmax_system_vs_numpy(N, d, K):
    """f, vec(AᵀR) and the assembled system at x0 != 0 against NumPy on the densified A, within the
    derived bounds of multi_sparse_data.softmax_bounds; G == Gᵀ exactly."""
    As, Y, x0 = S.sparse_problem(N, d, K)
    p = sparse_device_problem("softmax_ce", As, Y, x0, 1e-3, 1.0 / N)
    G, g, f = p.multi_system(x0)
    p.ctx.close()
    _check_softmax_system(As, Y, x0, 1.0 / N, G, g, f)


def test_softmax_soft_labels():
    """Rows of Y that do not sum to 1 (s_i in [0.5, 1.5])."""
    As, Y, x0 = S.sparse_problem(300, 17, 7, soft=True)
    assert np.mean(np.abs(Y.sum(axis=1) - 1.0) > 1e-3) > 0.9        # s_i != 1 on (nearly) every row
    p = sparse_device_problem("softmax_ce", As, Y, x0, 1e-3, 1.0 / 300)
    G, g, f = p.multi_system(x0)
    p.ctx.close()
    _check_softmax_system(As, Y, x0, 1.0 / 300, G, g, f)


# ---------------------------------------------------------------------------------------------
# 4. the sparse path against the dense path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(300, 130, 3), (40, 33, 16)])
def test_sparse_door_vs_dense_door(shape):
    """The same values through the dense door and the sparse door: each path is within its own bound
    of the exact result, so f, vec(AᵀR) and the system differ by at most twice the derived bound (the
    two paths share it: it depends on the values alone).  No bitwise claim."""
    N, d, K = shape
    c = 1.0 / N
    As, Y, x0 = S.sparse_problem(N, d, K)
    A = As.toarray()
    f_, of = M.device_losses(losses, "softmax_ce", K, c)
    pd = scsopt.Problem(A, Y, x0, f_, 1e-3, out_fn=of)
    Gd, gd, fd = pd.multi_system(x0)
    pd.ctx.close()
    ps = sparse_device_problem("softmax_ce", As, Y, x0, 1e-3, c)
    Gs, gs, fs = ps.multi_system(x0)
    ps.ctx.close()
    R, dR, df, dg, tau, P, s = S.softmax_bounds(A, Y, x0.reshape(d, K, order="F"), c)
    assert abs(fd - fs) <= 2 * df
    assert np.all(np.abs(gd - gs) <= 2 * dg.ravel(order="F"))
    for k in range(K):
        for l in range(K):
            sl = (slice(k * d, (k + 1) * d), slice(l * d, (l + 1) * d))
            assert np.all(np.abs(Gd[sl] - Gs[sl]) <= 2 * S.system_bound(A, P, s, c, tau, k, l)), (k, l)


# ---------------------------------------------------------------------------------------------
# 5. trajectories against the oracle on the densified A
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(kind, method, shape, lam, ss_type=1, test=False):
    N, d, K = shape
    As, Y, x0 = S.sparse_problem(N, d, K)
    kw = {}
    if test:
        At, Yt, _ = S.sparse_problem(77, d, K, soft=True)
        kw = dict(Atest=At.toarray(), ytest=Yt)
    om = O.Problem(As.toarray(), Y, x0, M.oracle_loss(O, kind, d, K, 1.0 / N), lam, **kw)
    return O.iterate(METHODS[method][1](ss_type=ss_type), om, "l1", OHM(), max_epoch=6)


def _compare(sol, osol):
    assert np.all(np.isfinite(osol.obj)) and np.all(np.isfinite(osol.x))     # the oracle itself ran clean
    assert sol.epochs == osol.epochs
    np.testing.assert_allclose(sol.obj, osol.obj, rtol=1e-8)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("lam", [2e-3, 2e-2])
@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("method", ["ggn", "nscore", "lqn"])
@pytest.mark.parametrize("kind", M.KINDS)
def test_trajectory_vs_oracle(kind, method, shape, lam, device_loop):
    """6 epochs, "l1" with PHuberSmootherL1L2(0.5), against the oracle on the densified A (the
    project's _compare tolerances).  At λ = 2e-2 the Gram methods end with a non-trivial support."""
    N, d, K = shape
    assert N * K + 1 > d * K
    As, Y, x0 = S.sparse_problem(N, d, K)
    osol = _oracle(kind, method, shape, lam)
    p = sparse_device_problem(kind, As, Y, x0, lam, 1.0 / N)
    sol = scsopt.iterate(METHODS[method][0](), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    p.ctx.close()
    _compare(sol, osol)
    if lam == 2e-2 and method != "lqn":
        zeros = int(np.sum(sol.x == 0.0))
        assert 0 < zeros < d * K, zeros


@pytest.mark.parametrize("kind,method,ss_type,shape", [
    ("softmax_ce", "lqn", 2, (200, 17, 7)),            # the Barzilai-Borwein step
    ("softmax_ce", "ggn", 3, (520, 129, 2)),           # the line search on N x K trial products
])
def test_trajectory_step_size_rules(kind, method, ss_type, shape):
    """ss_type 2 on ProxLQNSCORE against the oracle; ss_type 3 on ProxGGNSCORE against ProxNSCORE's
    oracle trajectory (the two methods build the same system; the oracle's ProxGGNSCORE line search
    needs a one-argument grad_fx its data closures do not have)."""
    N, d, K = shape
    As, Y, x0 = S.sparse_problem(N, d, K)
    osol = _oracle(kind, "nscore" if method == "ggn" else method, shape, 2e-3, ss_type)
    p = sparse_device_problem(kind, As, Y, x0, 2e-3, 1.0 / N)
    sol = scsopt.iterate(METHODS[method][0](ss_type=ss_type), p, "l1", HM(), max_epoch=6, verbose=0)
    p.ctx.close()
    _compare(sol, osol)


@pytest.mark.parametrize("device_loop", [False, True])
def test_heldout_fvaltest_sparse_atest(device_loop):
    """A sparse Atest (77 x d, soft labels) through the test door: fvaltest of every pushed point
    against the oracle, rtol 1e-8."""
    shape = (200, 17, 7)
    N, d, K = shape
    As, Y, x0 = S.sparse_problem(N, d, K)
    At, Yt, _ = S.sparse_problem(77, d, K, soft=True)
    osol = _oracle("softmax_ce", "ggn", shape, 2e-3, 1, True)
    p = sparse_device_problem("softmax_ce", As, Y, x0, 2e-3, 1.0 / N, Atest=At, ytest=Yt)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    assert p.ftest(x0) == pytest.approx(M.closures("softmax_ce", d, K, 1.0 / N)["f"](At.toarray(), Yt, x0), rel=1e-12)
    p.ctx.close()
    _compare(sol, osol)
    assert len(sol.fvaltest) == len(sol.obj) == len(osol.fvaltest)
    np.testing.assert_allclose(sol.fvaltest, osol.fvaltest, rtol=1e-8)
    # a sparse Atest beside a dense A (the mode admits the sparse test door alone)
    pd = sparse_device_problem("softmax_ce", As.toarray(), Y, x0, 2e-3, 1.0 / N, Atest=At, ytest=Yt)
    assert pd.ftest(x0) == pytest.approx(M.closures("softmax_ce", d, K, 1.0 / N)["f"](At.toarray(), Yt, x0), rel=1e-12)
    pd.ctx.close()


# ---------------------------------------------------------------------------------------------
# 6. doors and storage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [torch.int32, torch.int64])
def test_device_csr_door_equals_host_door(idx):
    """torch.sparse_csr_tensor on the GPU (int32 and int64 indices; Y on the host and on the device):
    bit for bit the host scipy door's products, system and getters."""
    N, d, K = 300, 130, 3
    As, Y, x0 = S.sparse_problem(N, d, K)
    rng = np.random.default_rng(2)
    X, V = rng.standard_normal((d, K)), rng.standard_normal((N, K))
    ph = sparse_device_problem("softmax_ce", As, Y, x0, 2e-3, 1.0 / N)
    axh, atvh = ph.multi_products(X, V)
    Gh, gh, fh = ph.multi_system(x0)
    ph.ctx.close()
    Yd = torch.from_numpy(np.ascontiguousarray(Y.T)).cuda().t()          # N x K, strides (1, N)
    for Yin in (Y, Yd):
        pd = sparse_device_problem("softmax_ce", torch_csr(As, idx), Yin, x0, 2e-3, 1.0 / N)
        axd, atvd = pd.multi_products(X, V)
        Gd, gd, fd = pd.multi_system(x0)
        Ag, Yg = pd.get_sparse()
        dims = C.c_int64()
        pd.ctx.check(_lib.lib.scs_get_dims(pd.ctx.h, None, C.byref(dims), None, None))
        Acsc = pd.get_sparse_csc()
        pd.ctx.close()
        assert np.array_equal(bits(axd), bits(axh)) and np.array_equal(bits(atvd), bits(atvh))
        assert fd == fh and np.array_equal(bits(gd), bits(gh)) and np.array_equal(bits(Gd), bits(Gh))
        assert dims.value == d and Ag.shape == (N, d) and Acsc.shape == (N, d)
        assert np.array_equal(Yg, Y) and (Ag != As).nnz == 0 and (Acsc.tocsr() != As).nnz == 0


def test_sparse_f32_equals_widened_values(monkeypatch):
    """sparse_f32=True gives bit for bit the products, system and trajectory of the same values widened
    to fp64 -- on the one-pass kernel, whose sum order (ascending index, one accumulator) does not
    depend on the slot width of the storage type.  The loop arm runs the single-vector kernels, whose
    4- and 8-entry slots sum in different orders (as on a single-output sparse context): no claim there."""
    monkeypatch.setenv("SCS_MULTI_SPARSE_KERNEL", "1")
    N, d, K = 300, 130, 3
    As, Y, x0 = S.sparse_problem(N, d, K)
    A32 = As.astype(np.float32)
    rng = np.random.default_rng(2)
    X, V = rng.standard_normal((d, K)), rng.standard_normal((N, K))
    out = []
    for Ain, f32 in ((A32.astype(np.float64), True), (A32.astype(np.float64), False)):
        p = sparse_device_problem("softmax_ce", Ain, Y, x0, 2e-3, 1.0 / N, sparse_f32=f32)
        ax, atv = p.multi_products(X, V)
        G, g, f = p.multi_system(x0)
        sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=4, verbose=0)
        p.ctx.close()
        out.append((ax, atv, G, g, np.array([f]), sol.x, sol.obj))
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------
# 7. determinism, and both arms against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["0", "1"])
def test_two_runs_give_equal_bits(arm, monkeypatch):
    """Two contexts in one process: equal bits in x and obj of a 6-epoch trajectory, and the arm's
    trajectory matches the oracle."""
    monkeypatch.setenv("SCS_MULTI_SPARSE_KERNEL", arm)
    shape = (300, 130, 3)
    N, d, K = shape
    As, Y, x0 = S.sparse_problem(N, d, K)
    sols = []
    for _ in range(2):
        p = sparse_device_problem("softmax_ce", As, Y, x0, 2e-3, 1.0 / N)
        sols.append(scsopt.iterate(scsopt.ProxLQNSCORE(m=5), p, "l1", HM(), max_epoch=6, verbose=0))
        assert p.ctx.kernel_names()[1].startswith(ARM_KERNEL[arm])
        p.ctx.close()
    assert np.array_equal(bits(sols[0].x), bits(sols[1].x)) and np.array_equal(bits(sols[0].obj), bits(sols[1].obj))
    _compare(sols[0], _oracle("softmax_ce", "lqn", shape, 2e-3))


# ---------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_name_the_switch_and_the_option():
    N, d, K = 60, 9, 3
    As, Y, x0 = S.sparse_problem(N, d, K)
    f, of = M.device_losses(losses, "softmax_ce", K, 1.0 / N)
    # without the mode: refused, and the message names the switch
    for Ain in (As, torch_csr(As)):
        with pytest.raises(ValueError, match=r"sparse A.*sparse_outputs=True / scs_set_sparse_outputs"):
            scsopt.Problem(Ain, Y, x0, f, 1e-3, out_fn=of)
    pdn = scsopt.Problem(As.toarray(), Y, x0, f, 1e-3, out_fn=of)
    with pytest.raises(ValueError, match=r"sparse Atest.*sparse_outputs=True / scs_set_sparse_outputs"):
        pdn.set_test(As, Y)
    pdn.ctx.close()
    csr, csc = As.tocsr(), As.tocsc()
    i64, i32 = _lib.c_i64p, _lib.c_i32p
    arrs = [np.ascontiguousarray(csr.indptr, dtype=np.int64), np.ascontiguousarray(csr.indices, dtype=np.int32),
            np.ascontiguousarray(csr.data), np.ascontiguousarray(csc.indptr, dtype=np.int64),
            np.ascontiguousarray(csc.indices, dtype=np.int32), np.ascontiguousarray(csc.data)]
    yv = np.zeros(N * K)

    def set_sparse(ctx):
        return _lib.lib.scs_set_sparse(ctx.h, N, d, csr.nnz, arrs[0].ctypes.data_as(i64), arrs[1].ctypes.data_as(i32),
                                       _lib.dptr(arrs[2]), arrs[3].ctypes.data_as(i64), arrs[4].ctypes.data_as(i32),
                                       _lib.dptr(arrs[5]), 0, _lib.dptr(yv), N, 0)

    ctx = _lib.Context(0)
    ctx.check(_lib.lib.scs_set_outputs(ctx.h, K))
    with pytest.raises(scsopt.ScsError, match=r"sparse A.*scs_set_sparse_outputs"):
        ctx.check(set_sparse(ctx))
    ctx.check(_lib.lib.scs_set_sparse_outputs(ctx.h, 1))     # accepted before the door, after scs_set_outputs
    ctx.check(set_sparse(ctx))
    dims = C.c_int64()
    ctx.check(_lib.lib.scs_get_dims(ctx.h, None, C.byref(dims), None, None))
    assert dims.value == d
    with pytest.raises(scsopt.ScsError, match=r"scs_set_compute_f32.*scs_set_outputs"):
        ctx.check(_lib.lib.scs_set_compute_f32(ctx.h, 1))
    spec = _lib.Synth(N_global=64, row0=0, N=64, m=8, seed=1, kind=4, density=0.25)
    with pytest.raises(scsopt.ScsError, match=r"scs_gen_sparse.*scs_set_outputs"):
        ctx.check(_lib.lib.scs_gen_sparse(ctx.h, C.byref(spec), 0))
    cb = _lib.ALLREDUCE_FN(lambda buf, n, st, user: 0)
    with pytest.raises(scsopt.ScsError, match="nranks > 1"):
        ctx.check(_lib.lib.scs_set_comm(ctx.h, 0, 2, cb, None))
    ctx.check(_lib.lib.scs_set_sparse_outputs(ctx.h, 0))     # off again: the door refuses again
    with pytest.raises(scsopt.ScsError, match=r"sparse A.*scs_set_sparse_outputs"):
        ctx.check(set_sparse(ctx))
    ctx.close()
    # in the mode: batches, the single-vector doors
    p = sparse_device_problem("softmax_ce", As, Y, x0, 1e-3, 1.0 / N)
    for kw in (dict(batch_size=20), dict(slice_samples=True)):
        with pytest.raises(scsopt.ScsError, match=r"batch_size / slice_samples.*scs_set_outputs"):
            scsopt.iterate(scsopt.ProxLQNSCORE(m=3), p, "l1", HM(), max_epoch=2, verbose=0, **kw)
    with pytest.raises(scsopt.ScsError, match="scs_gemv_t_eval"):
        p.gemv_t(np.zeros(N))
    p.ctx.close()


@pytest.mark.parametrize("device_loop", [False, True])
def test_ggn_sample_space_shape_is_refused(device_loop):
    """(20, 30, 3): N K + 1 = 61 <= d K = 90.  ProxGGNSCORE is refused as on a dense A (with
    scs_set_sparse_sample stored: it has no effect); ProxLQNSCORE on the same problem matches the oracle."""
    N, d, K = 20, 30, 3
    As, Y, x0 = S.sparse_problem(N, d, K)
    p = sparse_device_problem("softmax_ce", As, Y, x0, 2e-3, 1.0 / N, sparse_sample=True)
    with pytest.raises(scsopt.ScsError, match=r"scs_set_outputs.*sample-space branch.*losses\.callback"):
        scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", HM(), max_epoch=3, verbose=0, device_loop=device_loop)
    sol = scsopt.iterate(scsopt.ProxLQNSCORE(m=5), p, "l1", HM(), max_epoch=6, verbose=0, device_loop=device_loop)
    p.ctx.close()
    _compare(sol, _oracle("softmax_ce", "lqn", (N, d, K), 2e-3))


# ---------------------------------------------------------------------------------------------
# 9. no drift without nout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ggn", "nscore", "lqn"])
def test_mode_is_inert_without_outputs(method):
    """A sparse context with nout unset: the same 6-epoch trajectory with scs_set_sparse_outputs(1)
    stored and without it, equal bits (the mode has no effect without nout)."""
    N, d = 300, 130
    As, Y, x0 = S.sparse_problem(N, d, 2)
    y01, x0 = Y[:, 0].copy(), x0[:d].copy()
    sols = []
    for on in (False, True):
        if method == "ggn":
            meth, p = scsopt.ProxGGNSCORE(), scsopt.Problem(As, y01, x0, losses.logistic_ce(1.0 / N), 2e-3,
                                                            out_fn=losses.sigmoid_ce(1.0 / N), sparse_outputs=on)
        elif method == "nscore":
            meth, p = scsopt.ProxNSCORE(), scsopt.Problem(As, 2 * y01 - 1, x0, losses.logistic_margin(1.0 / N), 2e-3,
                                                          sparse_outputs=on)
        else:
            meth, p = scsopt.ProxLQNSCORE(m=5), scsopt.Problem(As, y01, x0, losses.least_squares(1.0 / N), 2e-3,
                                                               sparse_outputs=on)
        sols.append(scsopt.iterate(meth, p, "l1", HM(), max_epoch=6, verbose=0))
        p.ctx.close()
    assert np.array_equal(bits(sols[0].x), bits(sols[1].x)) and np.array_equal(bits(sols[0].obj), bits(sols[1].obj))
