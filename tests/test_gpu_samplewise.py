"""GPU: sample-wise losses outside the menu on the device data path (losses.samplewise,
scs_set_loss_samplewise): f(A, y, x) = Σᵢ ℓ(yᵢ, aᵢᵀx) with the caller's ℓ, ∂ℓ/∂z, ∂²ℓ/∂z² (and
ŷ = φ(z), dŷ/dz, ∂f/∂ŷ, ∂²f/∂ŷ² for ProxGGNSCORE) evaluated on z = A x and y, N numbers per
derivative; A, the products, the Gram, the solves, the line search and the exchange stay on the
device.

* bitwise against the menu: least squares with c = 2⁻⁸ on integer data written as a sample-wise
  loss.  Scaling by a power of two commutes with rounding and the reduction order is the menu's, so
  x and every history array are equal, in host and device mode, for every method, both ProxGGNSCORE
  branches, ss_type 1 and 3, fp32 storage, sparse A, a device A, minibatches, held-out rows, both
  loops and two row-sharded ranks.
* the new kernel's edges: N < 16, the 16-row padding, the 256-sample block edge, several partials.
* to rounding against the menu (logistic margin, sigmoid / cross-entropy) and against the oracle
  (Poisson regression), at the shapes and tolerances the host-callback tests hold.
* refusals and errors, after each of which the context still runs a menu loss.
"""
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import scsopt
from scsopt import losses

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

C8 = 2.0 ** -8
LAM = 2e-3
HIST = ("obj", "fval", "pri_res_norm", "rel", "objrel", "fvaltest")


def ls_samplewise(device):
    """0.5·c·Σ(z − y)² as a sample-wise loss; operators only, so NumPy arrays and torch tensors both
    pass through (a scalar return is broadcast)."""
    def value(z, y):
        r = z - y
        return (0.5 * C8) * (r * r)
    return losses.samplewise(value, lambda z, y: C8 * (z - y), lambda z, y: C8,
                             link=lambda z: z, link_d1=lambda z: 1.0,
                             grad_fy=lambda y, yh: C8 * (yh - y), hess_fy=lambda y, yh: C8, device=device)


def ls_menu():
    return losses.least_squares(C8), losses.linear_ls(C8)


@functools.lru_cache(maxsize=None)
def int_data(N, m, seed=7):
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 4, size=(N, m)).astype(np.float64)
    y = rng.integers(-5, 6, size=N).astype(np.float64)
    x0 = rng.integers(-2, 3, size=m).astype(np.float64)
    for a in (A, y, x0):
        a.setflags(write=False)
    return A, y, x0


def make_method(name, ss_type=1):
    if name == "nscore":
        return scsopt.ProxNSCORE(ss_type=ss_type)
    if name == "ggn":
        return scsopt.ProxGGNSCORE(ss_type=ss_type)
    return scsopt.ProxLQNSCORE(ss_type=ss_type, m=5)


def run(p, method, ss_type=1, epochs=6, **kw):
    return scsopt.iterate(make_method(method, ss_type), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=epochs,
                          verbose=0, **kw)


def hist_of(sol):
    out = {k: np.array([np.nan if v is None else v for v in getattr(sol, k)], dtype=np.float64) for k in HIST}
    out["x"] = np.array(sol.x)
    out["epochs"] = sol.epochs
    return out


def assert_same(a, b, what=""):
    assert a["epochs"] == b["epochs"], what
    for k in HIST + ("x",):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, a[k], b[k])


def menu_problem(A, y, x0, **kw):
    f, out = ls_menu()
    return scsopt.Problem(A, y, x0, f, LAM, out_fn=out, **kw)


@functools.lru_cache(maxsize=None)
def menu_reference(N, m, method, ss_type):
    A, y, x0 = int_data(N, m)
    return hist_of(run(menu_problem(A, y, x0, L=ls_L(ss_type)), method, ss_type))


def ls_L(ss_type):
    """With L set, ProxLQNSCORE's ss_type 3 is the line search too (without it: the BB step)."""
    return 4.0 if ss_type == 3 else None


ARMS = [("nscore", 300, 40), ("ggn", 300, 40), ("ggn", 30, 64), ("lqn", 300, 40)]


@pytest.mark.parametrize("ss_type", [1, 3])
@pytest.mark.parametrize("method,N,m", ARMS)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_least_squares_bitwise_vs_menu(device, method, N, m, ss_type):
    A, y, x0 = int_data(N, m)
    ref = menu_reference(N, m, method, ss_type)
    got = hist_of(run(scsopt.Problem(A, y, x0, ls_samplewise(device), LAM, L=ls_L(ss_type)), method, ss_type))
    assert_same(got, ref, (device, method, N, m, ss_type))
    assert np.all(np.isfinite(got["x"])) and got["epochs"] == 6   # the comparison covers six real steps


def test_bitwise_dense_f32():
    A, y, x0 = int_data(300, 40)
    ref = hist_of(run(menu_problem(A, y, x0, dense_f32=True), "ggn"))
    got = hist_of(run(scsopt.Problem(A, y, x0, ls_samplewise(True), LAM, dense_f32=True), "ggn"))
    assert_same(got, ref)


def test_bitwise_sparse():
    import scipy.sparse as sp
    A, y, x0 = int_data(300, 40)
    S = sp.csr_matrix(A)
    for method in ("nscore", "lqn"):
        ref = hist_of(run(menu_problem(S, y, x0), method))
        got = hist_of(run(scsopt.Problem(S, y, x0, ls_samplewise(False), LAM), method))
        assert_same(got, ref, method)


def test_bitwise_device_tensor():
    A, y, x0 = int_data(300, 40)
    At = torch.as_tensor(np.array(A), device="cuda")
    yt = torch.as_tensor(np.array(y), device="cuda")
    ref = hist_of(run(menu_problem(At, yt, x0), "ggn"))
    got = hist_of(run(scsopt.Problem(At, yt, x0, ls_samplewise(False), LAM), "ggn"))
    assert_same(got, ref)
    assert_same(got, menu_reference(300, 40, "ggn", 1))


def test_bitwise_two_unequal_batches():
    A, y, x0 = int_data(300, 40)
    kw = dict(batch_size=200, shuffle_batch=False, epochs=4)     # batches of 200 and 100 rows
    for method, device in (("nscore", True), ("ggn", False)):
        ref = hist_of(run(menu_problem(A, y, x0), method, **kw))
        got = hist_of(run(scsopt.Problem(A, y, x0, ls_samplewise(device), LAM), method, **kw))
        assert_same(got, ref, method)


def test_bitwise_held_out_set():
    A, y, x0 = int_data(300, 40)
    At, yt, _ = int_data(77, 40, seed=9)
    for device in (False, True):
        ref = hist_of(run(menu_problem(A, y, x0, Atest=At, ytest=yt), "lqn"))
        p = scsopt.Problem(A, y, x0, ls_samplewise(device), LAM, Atest=At, ytest=yt)
        got = hist_of(run(p, "lqn"))
        assert len(got["fvaltest"]) == len(got["obj"]) > 0
        assert_same(got, ref, device)
        assert p.ftest(x0) == menu_problem(A, y, x0, Atest=At, ytest=yt).ftest(x0)


@pytest.mark.parametrize("method", ["nscore", "lqn"])
def test_bitwise_host_loop_vs_device_loop(method):
    A, y, x0 = int_data(300, 40)
    ref = menu_reference(300, 40, method, 1)
    for device_loop in (False, True):
        got = hist_of(run(scsopt.Problem(A, y, x0, ls_samplewise(True), LAM), method, device_loop=device_loop))
        for k in ("obj", "fval", "x"):   # rel / objrel of the two loops differ in summation order only
            assert np.array_equal(got[k], ref[k]), (device_loop, k)


# ---- two row-sharded ranks on one GPU: sharded sample-wise against sharded menu ----------------
SHARD_ARMS = [("nscore", 301, 40, False), ("ggn", 301, 40, True), ("ggn", 30, 64, False), ("lqn", 301, 40, True)]


def _shard_worker(rank, world, store_path, out):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "selfconcordantsmoothoptimization.jl_amd"))
    import torch.distributed as dist
    from scsopt import shard
    dist.init_process_group("gloo", store=dist.FileStore(store_path, world), rank=rank, world_size=world)
    res = {}
    for method, N, m, device in SHARD_ARMS:
        A, y, x0 = int_data(N, m)
        r0, r1 = shard.row_range(N, world, rank)
        seen = []

        def value(z, y_, seen=seen):
            seen.append(len(z))
            r = z - y_
            return (0.5 * C8) * (r * r)
        sw = dataclasses.replace(ls_samplewise(device), value=value)
        sols = []
        for f, out_fn in (ls_menu(), (sw, None)):
            comm = shard.Comm(device=torch.device("cuda", 0))
            p = scsopt.Problem(A[r0:r1], y[r0:r1], x0, f, LAM, out_fn=out_fn, comm=comm, N_global=N, row0=r0)
            sols.append(hist_of(run(p, method)))
        res[(method, N, m)] = (sols[0], sols[1], sorted(set(seen)), r1 - r0)
    out[rank] = res
    dist.destroy_process_group()


def test_bitwise_two_ranks(tmp_path):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, str(tmp_path / "store"), out), nprocs=world, join=True)
    for method, N, m, _ in SHARD_ARMS:
        for r in range(world):
            menu, sw, seen, nloc = out[r][(method, N, m)]
            assert_same(sw, menu, (method, N, m, r))
            # each rank's functions see its own rows (the sharded sample-space branch: the gathered rows too)
            assert nloc in seen and set(seen) <= {nloc, N}, (method, seen, nloc)
        assert_same(out[0][(method, N, m)][1], out[1][(method, N, m)][1], method)


# ---- the new kernel's edges ------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 255, 256, 257, 513])
def test_kernel_edges_exact(N, device):
    """val_i = d1_i = i + 1 whatever z is: f = N(N+1)/2 and ∇f = Aᵀd1 exactly (integer A), at N < 16, the
    16-row padding, the 256-sample block edge and more than one value partial."""
    m = 8
    A, y, x0 = int_data(N, m, seed=100 + N)

    def ramp(z, y_):
        return torch.arange(1, len(z) + 1, dtype=torch.float64, device=z.device) if device else \
            np.arange(1.0, len(z) + 1)
    p = scsopt.Problem(A, y, x0, losses.samplewise(ramp, ramp, device=device), LAM)
    assert p.fx(x0) == N * (N + 1) / 2
    assert np.array_equal(p.gradx(x0), A.T @ np.arange(1.0, N + 1))


# ---- to rounding against the menu ------------------------------------------------------------
def _round_data():
    rng = np.random.default_rng(3)
    N, m = 400, 60
    A = rng.standard_normal((N, m)) / np.sqrt(m)
    return N, m, A, rng


@pytest.mark.parametrize("method", ["nscore", "lqn"])
def test_logistic_margin_matches_menu(method):
    N, m, A, rng = _round_data()
    y = np.sign(rng.standard_normal(N))
    x0 = rng.standard_normal(m) * 0.3

    def value(z, y):
        return np.log1p(np.exp(-y * z)) / N

    def d1(z, y):
        e = np.exp(-y * z)
        return (-y * e / (1.0 + e)) / N

    def d2(z, y):
        e = np.exp(-y * z)
        return (y * y) * e / ((1.0 + e) ** 2) / N
    a = run(scsopt.Problem(A, y, x0, losses.logistic_margin(1.0 / N), LAM), method, epochs=8)
    b = run(scsopt.Problem(A, y, x0, losses.samplewise(value, d1, d2), LAM), method, epochs=8)
    assert a.epochs == b.epochs
    np.testing.assert_allclose(b.obj, a.obj, rtol=1e-10)
    np.testing.assert_allclose(b.x, a.x, rtol=1e-8, atol=1e-12)


def _sigmoid_ce_samplewise(N, device=False):
    xp = torch if device else np
    sig = lambda z: 1.0 / (1.0 + xp.exp(-z))  # noqa: E731

    def value(z, y):
        yh = sig(z)
        return -(y * xp.log(yh) + (1 - y) * xp.log(1 - yh)) / N

    def link_d1(z):
        yh = sig(z)
        return yh * (1 - yh)
    return losses.samplewise(value, lambda z, y: (sig(z) - y) / N, link=sig, link_d1=link_d1,
                             grad_fy=lambda y, yh: (-(y / yh) + (1 - y) / (1 - yh)) / N,
                             hess_fy=lambda y, yh: (y / yh ** 2 + (1 - y) / (1 - yh) ** 2) / N, device=device)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sigmoid_ce_ggn_matches_menu(device):
    N, m, A, rng = _round_data()
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-A @ rng.standard_normal(m)))).astype(np.float64)
    x0 = rng.standard_normal(m) * 0.2
    pk = scsopt.Problem(A, y, x0, losses.logistic_ce(1.0 / N), LAM, out_fn=losses.sigmoid_ce(1.0 / N))
    a = run(pk, "ggn", epochs=8)
    b = run(scsopt.Problem(A, y, x0, _sigmoid_ce_samplewise(N, device), LAM), "ggn", epochs=8)
    assert a.epochs == b.epochs
    np.testing.assert_allclose(b.obj, a.obj, rtol=1e-10)
    np.testing.assert_allclose(b.x, a.x, rtol=1e-8, atol=1e-12)


# ---- against the oracle: Poisson regression --------------------------------------------------
@pytest.mark.parametrize("method,N,m,zero_x0", [a + (False,) for a in ARMS] + [("nscore", 300, 40, True)])
def test_poisson_regression_vs_oracle(method, N, m, zero_x0):
    """x0 = 0 is the default `sol`, so f_rel_error sits at f_tol in epoch 1: the reference stops the
    inner loop, refreshes f_rel_error and goes on (iterate.jl:235-259, 11 epochs counted for 10).  The
    host loop restates that; the device-resident loop of every data loss ends the solve there instead,
    so the x0 = 0 arm runs the host loop and the others start away from `sol`."""
    rng = np.random.default_rng(5)
    A = rng.standard_normal((N, m)) / np.sqrt(m)
    y = rng.poisson(np.exp(A @ (rng.standard_normal(m) * 0.5))).astype(np.float64)
    x0 = np.zeros(m) if zero_x0 else rng.standard_normal(m) * 0.1
    sw = losses.samplewise(lambda z, y: (np.exp(z) - y * z) / N, lambda z, y: (np.exp(z) - y) / N,
                           lambda z, y: np.exp(z) / N, link=np.exp, link_d1=np.exp,
                           grad_fy=lambda y, yh: (1 - y / yh) / N, hess_fy=lambda y, yh: y / (yh * yh * N))

    def f(A, y, x):
        z = A @ x
        return float(np.sum(np.exp(z) - y * z)) / N

    def g(A, y, x):
        return A.T @ (np.exp(A @ x) - y) / N

    def h(A, y, x):
        return A.T @ (np.exp(A @ x)[:, None] * A) / N
    ocb = O.CallbackLoss(f, g, h, out_fn=lambda A, x: np.exp(A @ x), jac_yx=lambda A, y, yh, x: yh[:, None] * A,
                         grad_fy=lambda A, y, yh: (1 - y / yh) / N, hess_fy=lambda A, y, yh: y / (yh * yh * N))
    lam = 1e-3
    OM = {"nscore": O.ProxNSCORE, "ggn": O.ProxGGNSCORE, "lqn": lambda: O.ProxLQNSCORE(m=5)}[method]
    sol = scsopt.iterate(make_method(method), scsopt.Problem(A, y, x0, sw, lam), "l1",
                         scsopt.PHuberSmootherL1L2(0.5), max_epoch=10, verbose=0,
                         device_loop=False if zero_x0 else None)
    osol = O.iterate(OM(), O.Problem(A, y, x0, ocb, lam), "l1", O.PHuberSmootherL1L2(0.5), max_epoch=10)
    assert sol.epochs == osol.epochs
    np.testing.assert_allclose(sol.obj, osol.obj, rtol=1e-8)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-6, atol=1e-9)


# ---- refusals and errors ---------------------------------------------------------------------
def _still_runs_menu(ctx, x0, ref):
    """The context of a refused / failed sample-wise loss, given the menu loss: the reference's bits."""
    f, out = ls_menu()
    q = scsopt.Problem(x0, f, LAM, out_fn=out, _ctx=ctx)
    assert_same(hist_of(run(q, "nscore", epochs=3)), ref)


def test_refusals_and_errors():
    N, m = 300, 40
    A, y, x0 = int_data(N, m)
    ref = hist_of(run(menu_problem(A, y, x0), "nscore", epochs=3))
    sw = ls_samplewise(False)

    # a host-exchange group of two "devices" on this GPU
    pg = menu_problem(A, y, x0, devices=[0, 0], device_exchange="host")
    fx = pg.fx(x0)
    with pytest.raises(scsopt.ScsError, match="single-device") as ei:
        scsopt.Problem(x0, sw, LAM, _ctx=pg.ctx)
    assert ei.value.code == scsopt._lib.SCS_ERR_ARG
    assert scsopt._lib.lib.scs_set_loss(pg.ctx.h, 7, 0, 1.0) == scsopt._lib.SCS_ERR_ARG
    assert pg.fx(x0) == fx
    np.testing.assert_allclose(hist_of(run(pg, "nscore", epochs=3))["obj"], ref["obj"], rtol=1e-10)

    # scale != 1
    p0 = menu_problem(A, y, x0)
    with pytest.raises(scsopt.ScsError, match="scale") as ei:
        scsopt.Problem(x0, dataclasses.replace(sw, scale=0.5), LAM, _ctx=p0.ctx)
    assert ei.value.code == scsopt._lib.SCS_ERR_ARG
    assert_same(hist_of(run(p0, "nscore", epochs=3)), ref)

    # ProxGGNSCORE without the GGN pieces: the menu's own refusal
    p = scsopt.Problem(A, y, x0, losses.samplewise(sw.value, sw.d1, sw.d2), LAM)
    with pytest.raises(scsopt.ScsError, match="ProxGGNSCORE"):
        run(p, "ggn", epochs=2)
    _still_runs_menu(p.ctx, x0, ref)

    # ProxNSCORE without d2
    p = scsopt.Problem(A, y, x0, losses.samplewise(sw.value, sw.d1), LAM)
    with pytest.raises(ValueError, match="d2.*no automatic differentiation"):
        run(p, "nscore", epochs=2)
    _still_runs_menu(p.ctx, x0, ref)

    # the caller's own exception comes back unchanged
    class Boom(Exception):
        pass
    boom = Boom("user d1 failed")

    def bad(z, y):
        raise boom
    for device in (False, True):
        p = scsopt.Problem(A, y, x0, losses.samplewise(sw.value, bad, device=device), LAM)
        assert p.fx(x0) == ref["fval"][0]
        with pytest.raises(Boom) as ei:
            run(p, "lqn", epochs=2)
        assert ei.value is boom
        _still_runs_menu(p.ctx, x0, ref)

    # a wrong length
    p = scsopt.Problem(A, y, x0, losses.samplewise(sw.value, lambda z, y: (z - y)[:-1]), LAM)
    with pytest.raises(ValueError, match="d1 returned shape"):
        p.gradx(x0)
    _still_runs_menu(p.ctx, x0, ref)
