"""GPU: ProxGGNSCORE's sample-space system of a sparse A built from its nonzeros (scs_set_sparse_sample,
Problem(..., sparse_sample=True)).

1. P = A diag(h) Aᵀ through the test door (Problem.sample_gram): the plain and the packed walk, two
   block widths, fp64- and fp32-stored values -- the same bits; on integer data exactly NumPy's P and
   the dense path's (switch off).
2. The branch boundary n_b + 1 <= m.
3. A sparse view's steps equal, bit for bit, the steps of a context holding A[rows_b], y[rows_b].
4. Trajectories against the oracle on the densified matrix.
5. Memory.
6. The switch off changes nothing.

The shapes and their edges are stated, and checked on the CPU, in tests/sparse_sample_data.py /
tests/test_sparse_sample_host.py.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scsopt
from scsopt import losses
from scsopt.iterate import device_optim_loop, init_method, optim_loop, step

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402
import sparse_sample_data as D  # noqa: E402

pytestmark = pytest.mark.gpu

HIST = ("obj", "fval", "pri_res_norm", "rel", "objrel", "fvaltest")
LAM = 1e-3
K_STEPS = 3
DEV = torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def hmu():
    return scsopt.PHuberSmootherL1L2(1.0)


def ce(N):
    return losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)


def hist_of(sol):
    out = {k: np.array([np.nan if v is None else v for v in getattr(sol, k)], dtype=np.float64) for k in HIST}
    out["x"] = np.array(sol.x)
    out["epochs"] = sol.epochs
    return out


def assert_same(a, b, what=""):
    assert a["epochs"] == b["epochs"], what
    for k in HIST + ("x",):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, a[k], b[k])


def device_csr(case):
    """the raw arrays (unsorted row, duplicated column) as a torch CSR tensor on the GPU: the device door
    sorts each row by column and keeps the duplicates"""
    ip, ix, dv = case.raw
    return torch.sparse_csr_tensor(torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV),
                                   torch.from_numpy(dv).to(DEV), size=(case.n, case.m))


def door_problem(case, sparse_f32=False, sparse_sample=True):
    n = case.n
    y = (np.arange(n) % 2).astype(np.float64)
    f, out = ce(n)
    return scsopt.Problem(device_csr(case), y, np.zeros(case.m), f, LAM, out_fn=out, sparse_f32=sparse_f32,
                          sparse_sample=sparse_sample)


# ---- 1. P through the door ---------------------------------------------------------------------------
def _arms(p, h, monkeypatch, shifts):
    out = {}
    for shift in shifts:
        monkeypatch.setenv("SCS_SPARSE_GRAM_SHIFT", str(shift))
        for arm in (0, 1):
            monkeypatch.setenv("SCS_SPARSE_SAMPLE_KERNEL", str(arm))
            out[(shift, arm)] = p.sample_gram(h)
    return out


@pytest.mark.parametrize("sparse_f32", [False, True], ids=["fp64", "fp32_stored"])
@pytest.mark.parametrize("n", D.P_SIZES)
def test_p_integer_exact(n, sparse_f32, monkeypatch):
    """Integer data, power-of-two weights: plain and packed arm, SCS_SPARSE_GRAM_SHIFT = 7 (three sample
    blocks at n = 300) and 12 give NumPy's integer P exactly, and so does the dense path."""
    c = D.gram_case(n)
    ref = D.dense_gram(c)
    p = door_problem(c, sparse_f32)
    try:
        for key, P in _arms(p, c.h, monkeypatch, (7, 12)).items():
            assert np.array_equal(P, ref), (n, key, np.max(np.abs(P - ref)))
        p.set_sparse_sample(False)
        Pd = p.sample_gram(c.h)
        assert np.array_equal(Pd, ref), (n, "dense path", np.max(np.abs(Pd - ref)))
    finally:
        p.ctx.close()


@pytest.mark.parametrize("n", D.P_SIZES)
def test_p_same_bits_across_arms_and_shifts(n, monkeypatch):
    """Real values: the packed walk and the block width change no bit of P (the summation order of each
    P(k, i) is the stored order of row i); the dense path agrees to rounding."""
    c = D.gram_case(n, integer=False)
    p = door_problem(c)
    try:
        got = _arms(p, c.h, monkeypatch, (7, 12))
        first = got[(7, 0)]
        for key, P in got.items():
            assert np.array_equal(bits(P), bits(first)), (n, key)
        assert np.array_equal(first, first.T)
        np.testing.assert_allclose(first, D.dense_gram(c), rtol=1e-12, atol=1e-11)
        # ... and it is the order restated in tests/sparse_sample_data.py
        assert np.array_equal(bits(first), bits(D.sample_gram_walk(c.stored, c.n, c.m, c.h, 7)))
    finally:
        p.ctx.close()


@pytest.mark.parametrize("sparse_f32", [False, True], ids=["fp64", "fp32_stored"])
def test_p_two_blocks_at_the_default_shift(sparse_f32, monkeypatch):
    """n = 4096 + 40, m = 4200, 8 entries per row: two blocks of 4096 samples, n + 1 <= m."""
    monkeypatch.delenv("SCS_SPARSE_GRAM_SHIFT", raising=False)
    c = D.big_case()
    ref = D.dense_gram(c)
    p = door_problem(c, sparse_f32)
    try:
        for arm in (0, 1):
            monkeypatch.setenv("SCS_SPARSE_SAMPLE_KERNEL", str(arm))
            P = p.sample_gram(c.h)
            assert np.array_equal(P, ref), (arm, np.max(np.abs(P - ref)))
    finally:
        p.ctx.close()


# ---- 2. the branch boundary --------------------------------------------------------------------------
def _ggn_steps(p, x0, batch=None, ss_type=1):
    meth = scsopt.ProxGGNSCORE(ss_type=ss_type)
    p.configure("l1", hmu())
    init_method(meth, p)
    x_prev, x, out = x0, x0, []
    for it in range(1, K_STEPS + 1):
        xn, pri = step(meth, p, "l1", hmu(), x, x_prev, it, batch=batch)
        out.append((xn, pri))
        x_prev, x = x, xn
    return out


def test_branch_boundary():
    """m = 96: a batch of m - 1 rows takes the sparse view (a build is counted), one of m rows keeps the
    dense view and the feature-space Gram -- bit for bit the steps without the switch."""
    N, m = 400, 96
    rng = np.random.default_rng(7)
    A = (sp.random(N, m, density=0.08, random_state=5, format="csr") * 3.0).tocsr()
    y = (rng.random(N) < 0.5).astype(np.float64)
    x0 = rng.standard_normal(m) * 0.3
    perm = rng.permutation(N)
    batches = [perm[:m - 1], perm[m:2 * m]]
    f, out = ce(N)
    on = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True, sparse_sample=True)
    off = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True)
    try:
        on.set_batches(batches)
        off.set_batches(batches)
        small = _ggn_steps(on, x0, batch=0)
        assert on.batch_info()[0] == 1 and on.batch_info()[2] == 1
        assert all(np.all(np.isfinite(x)) for x, _ in small)
        ref = scsopt.Problem(A[batches[0]], y[batches[0]], x0, f, LAM, out_fn=out, sparse_sample=True)
        for (xg, pg), (xr, pr) in zip(small, _ggn_steps(ref, x0)):
            assert np.array_equal(bits(xg), bits(xr)) and np.array_equal(bits(pg), bits(pr))
        ref.ctx.close()
        big = _ggn_steps(on, x0, batch=1)
        assert on.batch_info()[0] == 1 and on.batch_info()[2] == 1      # no second build: the dense view
        for (xg, pg), (xr, pr) in zip(big, _ggn_steps(off, x0, batch=1)):
            assert np.array_equal(bits(xg), bits(xr)) and np.array_equal(bits(pg), bits(pr))
        assert off.batch_info() == (0, 0, 0)
    finally:
        for p in (on, off):
            p.set_batches(None)
            p.ctx.close()


# ---- 3. the bits of a view -----------------------------------------------------------------------------
def _check_views(name, sparse_f32=False):
    A, y, x0, batches = D.view_case(name)
    N = A.shape[0]
    f, out = ce(N)
    big = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True, sparse_sample=True, sparse_f32=sparse_f32)
    big.set_batches(batches)
    try:
        for bi, rows in enumerate(batches):
            got = _ggn_steps(big, x0, batch=bi)
            ref_p = scsopt.Problem(A[rows], y[rows], x0, f, LAM, out_fn=out, sparse_sample=True,
                                   sparse_f32=sparse_f32)   # the same loss constant
            ref = _ggn_steps(ref_p, x0)
            ref_p.ctx.close()
            for it, ((xg, pg), (xr, pr)) in enumerate(zip(got, ref)):
                assert np.all(np.isfinite(xr)), (name, bi, it)
                assert np.array_equal(bits(xg), bits(xr)), (name, bi, len(rows), it, np.max(np.abs(xg - xr)))
                assert np.array_equal(bits(pg), bits(pr)), (name, bi, len(rows), it, pg, pr)
        nviews, vbytes, builds = big.batch_info()
        assert builds == len(batches) and nviews >= 1 and vbytes > 0
    finally:
        big.set_batches(None)
        big.ctx.close()


@pytest.mark.parametrize("name", ["partial", "big"])
def test_view_steps_equal_the_sliced_problem(name):
    """partial: N = 1500, m = 512, batches of 400 (the last 300), one with a row twice, one of empty rows
    only (P = 0).  big: one batch of 4096 + 40 rows at m = 4200."""
    _check_views(name)


def test_view_steps_fp32_stored():
    _check_views("partial", sparse_f32=True)


# ---- 4. trajectory -----------------------------------------------------------------------------------
def _traj_data():
    N, m = 1200, 512
    rng = np.random.default_rng(17)
    A = (sp.random(N, m, density=0.03, random_state=3, format="csr") * 3.0).tocsr()
    y = (rng.random(N) < 0.5).astype(np.float64)
    x0 = rng.standard_normal(m) * 0.3
    perm = np.random.default_rng(4).permutation(N)
    return A, y, x0, perm, N


@pytest.mark.parametrize("ss_type", [1, 3])
def test_trajectory_vs_oracle(ss_type):
    """4 shuffled batches of 300 rows (300 + 1 <= 512), 3 epochs, both loops."""
    A, y, x0, perm, N = _traj_data()
    f, out = ce(N)
    batches = O.loader_batches(N, 300, perm=perm)
    assert len(batches) == 4
    om = O.Problem(A.toarray(), y, x0, O.Loss("logistic_ce", 1.0 / N, ggn="sigmoid_ce"), LAM)
    o = O.iterate(O.ProxGGNSCORE(ss_type=ss_type), om, "l1", O.PHuberSmootherL1L2(1.0), max_epoch=3, batches=batches)
    runs = []
    for loop in (device_optim_loop, optim_loop):
        p = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True, sparse_sample=True)
        p.set_batches(batches)
        try:
            kw = {} if loop is device_optim_loop else {"nbatch": len(batches)}
            s = loop(scsopt.ProxGGNSCORE(ss_type=ss_type), p, "l1", hmu(), max_epoch=3, verbose=0, **kw)
            assert p.batch_info()[0] == 4 and p.batch_info()[2] == 4   # sparse views, each built once
        finally:
            p.set_batches(None)
            p.ctx.close()
        assert s.epochs == o.epochs and len(s.obj) == len(o.obj)
        np.testing.assert_allclose(s.obj, o.obj, rtol=1e-8)
        np.testing.assert_allclose(s.x, o.x, rtol=1e-6, atol=1e-9)
        runs.append(s)
    assert np.array_equal(bits(runs[0].x), bits(runs[1].x))


def test_full_data_vs_oracle():
    """tests/test_gpu_sparse.py's ggn_sample_space case (N = 96, m = 256) with the switch on."""
    N, m = 96, 256
    rng = np.random.default_rng(41)
    C = sp.random(N, m, density=0.05, random_state=7, format="coo")
    rows = np.concatenate([C.row, C.row[:50]])
    cols = np.concatenate([C.col, C.col[:50]])
    vals = np.concatenate([C.data, rng.standard_normal(50)]) * 2.0
    perm = rng.permutation(rows.size)
    A = sp.coo_matrix((vals[perm], (rows[perm], cols[perm])), shape=(N, m))
    y = (rng.random(N) < 0.5).astype(float)
    x0 = rng.standard_normal(m) * 0.3
    f, out = ce(N)
    p = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_sample=True)
    om = O.Problem(A.toarray(), y, x0, O.Loss("logistic_ce", 1.0 / N, ggn="sigmoid_ce"), LAM)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", hmu(), max_epoch=8, verbose=0)
    osol = O.iterate(O.ProxGGNSCORE(), om, "l1", O.PHuberSmootherL1L2(1.0), max_epoch=8)
    p.ctx.close()
    assert sol.epochs == osol.epochs and len(sol.obj) == len(osol.obj)
    np.testing.assert_allclose(sol.obj, osol.obj, rtol=1e-8, atol=0)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-6, atol=1e-9)


def _samplewise_pair():
    """The trajectory problem under the menu kind and under the logistic loss restated as a sample-wise
    loss (host callables), both on sparse views with the switch on -> (menu, samplewise) histories."""
    A, y, x0, perm, N = _traj_data()
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))  # noqa: E731

    def value(z, yy):
        yh = sig(z)
        return -(yy * np.log(yh) + (1 - yy) * np.log(1 - yh)) / N

    def link_d1(z):
        yh = sig(z)
        return yh * (1 - yh)
    sw = losses.samplewise(value, lambda z, yy: (sig(z) - yy) / N, link=sig, link_d1=link_d1,
                           grad_fy=lambda yy, yh: (-(yy / yh) + (1 - yy) / (1 - yh)) / N,
                           hess_fy=lambda yy, yh: (yy / yh ** 2 + (1 - yy) / (1 - yh) ** 2) / N)
    f, out = ce(N)
    run = lambda p: hist_of(scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", hmu(), batch_size=300, batch_perm=perm,  # noqa: E731
                                           max_epoch=3, verbose=0))
    ref = run(scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True, sparse_sample=True))
    got = run(scsopt.Problem(A, y, x0, sw, LAM, sparse_batches=True, sparse_sample=True))
    return ref, got


def test_samplewise_logistic_close_to_menu():
    """The bar of tests/test_gpu_samplewise.py::test_sigmoid_ce_ggn_matches_menu, on sparse views."""
    ref, got = _samplewise_pair()
    assert got["epochs"] == ref["epochs"] == 3 and np.all(np.isfinite(got["x"]))
    np.testing.assert_allclose(got["obj"], ref["obj"], rtol=1e-10)
    np.testing.assert_allclose(got["x"], ref["x"], rtol=1e-8, atol=1e-12)


C10 = 2.0 ** -10


def _logistic_on_device(c):
    """The menu's logistic CE + sigmoid_ce (epilogue_kernel, csrc/data.hip) restated operation by
    operation as a device-mode sample-wise loss: e = exp(-z), ŷ = 1/(1 + e), s = e/((1 + e)(1 + e)),
    r = -c(y/ŷ - (1 - y)/(1 - ŷ)), q = c(y/ŷ² + (1 - y)/(1 - ŷ)²), ∂ℓ/∂z = s·r,
    ℓ = -c(y log ŷ + (1 - y) log(1 - ŷ)).  Every operation is an IEEE one or the device's exp / log in
    both, so the bits are the same where no rounding depends on the grouping: y ∈ {0, 1} makes one of
    the two summands of ℓ, r and q an exact zero (a fused multiply-add in the kernel rounds as the two
    operations here do), and c a power of two makes Σ(-c·t) = -c·Σt exact over the same reduction."""
    def e_of(z):
        return torch.exp(-z)

    def link(z):
        e = e_of(z)
        return torch.ones_like(e) / (1.0 + e)

    def link_d1(z):
        e = e_of(z)
        return e / ((1.0 + e) * (1.0 + e))

    def grad_fy(yy, yh):
        return -c * (yy / yh - (1.0 - yy) / (1.0 - yh))

    def hess_fy(yy, yh):
        return c * (yy / (yh * yh) + (1.0 - yy) / ((1.0 - yh) * (1.0 - yh)))

    def value(z, yy):
        yh = link(z)
        return -c * (yy * torch.log(yh) + (1.0 - yy) * torch.log(1.0 - yh))
    return losses.samplewise(value, lambda z, yy: link_d1(z) * grad_fy(yy, link(z)), link=link, link_d1=link_d1,
                             grad_fy=grad_fy, hess_fy=hess_fy, device=True)


def test_samplewise_logistic_equals_menu():
    """The logistic loss restated as a sample-wise loss against the menu kind, bit for bit, on sparse
    views with the switch on: the trajectory problem (4 shuffled batches of 300 rows, 3 epochs), labels
    in {0, 1}, loss constant 2⁻¹⁰.  The callables run on the device and follow the menu's epilogue
    operation by operation (_logistic_on_device); host callables on NumPy's exp differ from the
    device's in the last bit and are held to the project's bar in test_samplewise_logistic_close_to_menu."""
    A, y, x0, perm, N = _traj_data()
    assert set(np.unique(y)) == {0.0, 1.0}
    run = lambda p: hist_of(scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", hmu(), batch_size=300, batch_perm=perm,  # noqa: E731
                                           max_epoch=3, verbose=0))
    ref = run(scsopt.Problem(A, y, x0, losses.logistic_ce(C10), LAM, out_fn=losses.sigmoid_ce(C10), sparse_batches=True,
                             sparse_sample=True))
    got = run(scsopt.Problem(A, y, x0, _logistic_on_device(C10), LAM, sparse_batches=True, sparse_sample=True))
    assert ref["epochs"] == 3 and np.all(np.isfinite(ref["x"])) and np.any(ref["x"] != x0)
    for k in ("x", "obj", "fval"):
        print(k, "max |samplewise - menu| =", np.max(np.abs(got[k] - ref[k])))
    assert_same(got, ref, "samplewise vs menu")


# ---- 5. memory ------------------------------------------------------------------------------------------
def _wide(N=200, m=16384 + 130, per_row=8):
    rng = np.random.default_rng(61)
    w = m // per_row
    cols = np.arange(per_row)[None, :] * w + rng.integers(0, w, size=(N, per_row))
    A = sp.csr_matrix((rng.standard_normal(cols.size) * 2.0, cols.ravel(), np.arange(0, cols.size + 1, per_row)),
                      shape=(N, m))
    y = (rng.random(N) < 0.5).astype(np.float64)
    return A, y, rng.standard_normal(m) * 0.1


def _grown_by_one_step(sparse_sample):
    A, y, x0 = _wide()
    N = A.shape[0]
    f, out = ce(N)
    p = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_sample=sparse_sample)
    p.configure("l1", hmu())
    meth = scsopt.ProxGGNSCORE()
    init_method(meth, p)
    base = p.data_info()[2]
    xn, pri = step(meth, p, "l1", hmu(), x0, x0, 1)
    grown = p.data_info()[2] - base
    p.ctx.close()
    return xn, pri, grown


def test_full_data_allocates_no_dense_copy():
    """N = 200, m = 16384 + 130: one mirror is Npad·mpad·8 B (26.6 MB).  With the switch on a step allocates
    less than one such copy; with it off at least two (the mirror and Aᵀ)."""
    N, m = 200, 16384 + 130
    mirror = (-(-N // 16) * 16) * (-(-m // 128) * 128) * 8
    x_on, pri_on, g_on = _grown_by_one_step(True)
    x_off, pri_off, g_off = _grown_by_one_step(False)
    assert np.all(np.isfinite(x_on)) and np.isfinite(pri_on)
    assert g_on < mirror, (g_on, mirror)
    assert g_off >= 2 * mirror, (g_off, mirror)
    np.testing.assert_allclose(x_on, x_off, rtol=1e-8, atol=1e-11)


def test_view_bytes_and_builds():
    """The views' bytes stay below the dense views'; a second epoch builds nothing; set_batches(None)
    returns the bytes to the baseline."""
    A, y, x0, perm, N = _traj_data()
    m = A.shape[1]
    f, out = ce(N)
    batches = O.loader_batches(N, 300, perm=perm)
    p = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True, sparse_sample=True)
    p.configure("l1", hmu())
    p.set_batches(batches)       # the solver's own scratch (sized by the system) exists before the baseline
    device_optim_loop(scsopt.ProxGGNSCORE(), p, "l1", hmu(), max_epoch=1, verbose=0)
    p.set_batches(None)
    assert p.batch_info() == (0, 0, 0)
    base = p.data_info()[2]
    p.set_batches(batches)
    try:
        device_optim_loop(scsopt.ProxGGNSCORE(), p, "l1", hmu(), max_epoch=1, verbose=0)
        nv1, vb1, b1 = p.batch_info()
        held = p.data_info()[2]
        device_optim_loop(scsopt.ProxGGNSCORE(), p, "l1", hmu(), max_epoch=2, verbose=0)
        nv2, vb2, b2 = p.batch_info()
    finally:
        p.set_batches(None)
    after = p.data_info()[2]
    p.ctx.close()
    assert (nv1, b1) == (4, 4) and (nv2, b2) == (4, 4) and vb2 == vb1
    dense_views = 4 * 304 * (-(-m // 128) * 128) * 8    # the four dense views' rows (Npad = 304), without their Aᵀ
    assert 0 < vb1 < dense_views, (vb1, dense_views)
    assert held >= base + vb1
    assert after == base, (after, base)


# ---- 6. the switch off --------------------------------------------------------------------------------
def test_switch_off_is_the_default():
    A, y, x0, perm, N = _traj_data()
    f, out = ce(N)
    run = lambda p: hist_of(scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", hmu(), batch_size=300, batch_perm=perm,  # noqa: E731
                                           max_epoch=2, verbose=0))
    a = run(scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True, sparse_sample=False))
    b = run(scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=True))
    assert_same(a, b, "sparse_sample=False vs no argument")
