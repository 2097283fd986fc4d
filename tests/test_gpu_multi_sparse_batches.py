"""GPU: minibatches of a multi-output loss on a sparse A (scs_set_multi_sparse_batches /
multi_sparse_batches=True).  The K-column products on a selected sparse view against exact
integers (both workgroup forms of the one-pass kernel, both storage types), a step on a sparse view against
the step of a sparse context holding that batch and a step on a densified view against the step of a dense
context holding it, the minibatch trajectories of the three methods against the oracle's loop on
A.toarray() over the same row lists (tests/multi_sparse_batches_data.py; the oracle's side is checked on the
CPU in test_multi_sparse_batches_host.py), and the switch's no-drift and refusal rules."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import scsopt
from scsopt import _lib, losses
from scsopt.iterate import init_method, step

import multi_output_data as M
import multi_sparse_batches_data as D
import multi_sparse_data as S

pytestmark = pytest.mark.gpu

HM = lambda: scsopt.PHuberSmootherL1L2(0.5)      # noqa: E731
METHODS = {"ggn": scsopt.ProxGGNSCORE, "nscore": scsopt.ProxNSCORE, "lqn": lambda **kw: scsopt.ProxLQNSCORE(m=5, **kw)}
CASE_ID = lambda c: "x".join(map(str, c[0]))     # noqa: E731
FORM_KERNEL = {"0": "multi_spmm_blk_kernel<", "1": "multi_spmm_blk256_kernel<"}
ON = dict(sparse_outputs=True, multi_batches=True, multi_sparse_batches=True)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("SCS_"):
            monkeypatch.delenv(k)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def problem(kind, A, Y, x0, lam, c, **kw):
    f, out_fn = M.device_losses(losses, kind, Y.shape[1], c)
    return scsopt.Problem(A, Y, x0, f, lam, out_fn=out_fn, **kw)


def run(method, p, device_loop, max_epoch=6, **kw):
    return scsopt.iterate(METHODS[method](), p, "l1", HM(), max_epoch=max_epoch, verbose=0, device_loop=device_loop,
                          **kw)


def shuffled(N, bs):
    return dict(batch_size=bs, shuffle_batch=True, batch_perm=D.perm_of(N))


def _compare(sol, osol):
    """test_gpu_multi_output._compare's tolerances."""
    assert np.all(np.isfinite(osol.obj)) and np.all(np.isfinite(osol.x))
    assert sol.epochs == osol.epochs and len(sol.obj) == len(osol.obj)
    np.testing.assert_allclose(sol.obj, osol.obj, rtol=1e-8)
    np.testing.assert_allclose(sol.x, osol.x, rtol=1e-6, atol=1e-9)


def _same_bits(a, b):
    assert a.epochs == b.epochs and len(a.obj) == len(b.obj)
    for name in ("x", "obj", "fval"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert np.array_equal(bits(a.pri_res_norm[1:]), bits(b.pri_res_norm[1:]))


# ---------------------------------------------------------------------------------------------
# 1. the products on a view, exactly
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("N,d", D.EXACT_VIEW_SHAPES)
def test_products_on_a_view_exact_integers(N, d, f32, form, monkeypatch):
    """Integer data (multi_sparse_data.exact_sparse_case; Σ|terms| < 2^53 asserted per batch): multi_products on
    a selected sparse view returns the int64 S[rows_b] X and S[rows_b]ᵀ V_b bit for bit with the 1024-row and
    the 256-row form of the one-pass kernel (SCS_MULTI_SPARSE_NARROW; kernel_names() proves the form), fp64 and
    fp32 values, K = 2, 3, 16 (SCS_MULTI_SPARSE_KERNEL=1: K = 2 runs the kernel too).  Batches of
    D.exact_batches: a ragged last workgroup, a repeated row, row N - 1, an empty row, two groups, two
    sub-blocks on either side, W < 16384.  Back on the full data the products are the full data's."""
    monkeypatch.setenv("SCS_MULTI_SPARSE_KERNEL", "1")
    monkeypatch.setenv("SCS_MULTI_SPARSE_NARROW", form)
    for K in D.EXACT_K:
        c, per = D.exact_view_case(N, d, K)
        f, of = M.device_losses(losses, "multi_least_squares", K, 1.0)
        p = scsopt.Problem(c.coo, np.zeros((N, K)), np.zeros(d * K), f, 1.0, out_fn=of, sparse_f32=f32,
                           sparse_batches=True, **ON)
        p.configure("l1", HM())
        init_method(scsopt.ProxLQNSCORE(m=3), p)
        p.set_batches([rows for rows, *_ in per])
        for b, (rows, V, AX, ATV, _) in enumerate(per):
            p.select_batch(b)
            ax, atv = p.multi_products(c.X, V)
            name = p.ctx.kernel_names()[1]
            assert name.startswith(FORM_KERNEL[form]), name
            assert ("float, 8" if f32 else "double, 4") in name, name
            assert ax.shape == AX.shape and np.array_equal(bits(ax), bits(AX)), (K, b, "A_b X")
            assert np.array_equal(bits(atv), bits(ATV)), (K, b, "A_b' V")
        assert p.batch_info()[0] == len(per)
        p.select_batch(-1)
        ax, atv = p.multi_products(c.X, c.V)
        assert p.ctx.kernel_names()[1].startswith("multi_spmm_blk_kernel<")       # the full data keeps 1024 rows
        p.ctx.close()
        assert np.array_equal(bits(ax), bits(c.AX.astype(np.float64))) and np.array_equal(
            bits(atv), bits(c.ATV.astype(np.float64)))


@pytest.mark.parametrize("K,narrow", [(3, False), (7, True), (16, True)])
def test_default_form_on_views(K, narrow):
    """Nothing forced: views take the 256-row form where it was measured below the 1024-row form (KP = 8 and 16,
    DESIGN §2l) and keep 1024 rows at KP = 4; the full data keeps 1024 rows."""
    N, d = 300, 130
    A, Y, x0 = S.sparse_problem(N, d, K)
    p = problem("multi_least_squares", A, Y, x0, 1e-3, 1.0 / N, sparse_batches=True, **ON)
    p.configure("l1", HM())
    init_method(scsopt.ProxLQNSCORE(m=3), p)
    p.set_batches([np.arange(40)])
    p.select_batch(0)
    p.multi_products(np.ones((d, K)), None)
    on_view = p.ctx.kernel_names()[1]
    p.select_batch(-1)
    p.multi_products(np.ones((d, K)), None)
    on_data = p.ctx.kernel_names()[1]
    p.ctx.close()
    assert on_view.startswith(FORM_KERNEL["1" if narrow else "0"]), on_view
    assert on_data.startswith(FORM_KERNEL["0"]), on_data


def test_get_batch_data_densifies_the_rows():
    """scs_get_batch_data on the new contexts: the batch's rows densified (duplicates summed: integers, exact)
    and widened, and Y_b -- whatever kind of view the method asks for; the selection and the views are left
    as found."""
    N, d, K = 700, 300, 3
    c, per = D.exact_view_case(N, d, K)
    rows = per[0][0]
    Y = np.random.default_rng(3).integers(-9, 10, size=(N, K)).astype(np.float64)
    want = np.asarray(c.S[rows].todense()).astype(np.float64)
    f, of = M.device_losses(losses, "multi_least_squares", K, 1.0)
    for f32 in (False, True):
        for sb in (False, True):
            p = scsopt.Problem(c.coo, Y, np.zeros(d * K), f, 1.0, out_fn=of, sparse_f32=f32, sparse_batches=sb, **ON)
            p.configure("l1", HM())
            init_method(scsopt.ProxLQNSCORE(m=3), p)
            p.set_batches([rows, rows[:40]])
            p.select_batch(1)
            before = p.batch_info()
            Ab, Yb = p.get_batch_data(0)
            assert p.batch_info() == before
            p.ctx.close()
            assert np.array_equal(bits(Ab), bits(want)) and np.array_equal(bits(Yb), bits(Y[rows])), (f32, sb)


# ---------------------------------------------------------------------------------------------
# 2. a step on a view is the step on that data
# ---------------------------------------------------------------------------------------------
def _row_lists(N, nrows):
    stride = N // nrows
    small = max(nrows // 3, 1)
    return [np.arange(0, stride * nrows, stride)[::-1].copy(), (np.arange(nrows) * 7 + 3) % N,
            (np.arange(small) * 5 + 1) % N]


@pytest.mark.parametrize("refill", [False, True])
@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape,nrows", [((520, 129, 2), 260), ((300, 130, 3), 137), ((40, 33, 16), 17)])
def test_step_on_a_sparse_view_is_the_step_on_that_data(shape, nrows, f32, form, refill, monkeypatch):
    """ProxLQNSCORE with sparse_batches: step(..., batch=b) equals bit for bit (x_new, pri) the step of a fresh
    sparse Problem(A[rows_b], Y[rows_b], sparse_outputs=True) with the same loss objects (scale 1/N of the full
    data) and x -- K = 2 on the loop arm, K = 3 and 16 on the product kernel, fp64 and fp32 values, both
    workgroup forms on the view (the second context always runs the 1024-row form).  Two lists of one size and
    a smaller list after them; refill: SCS_SPARSE_BATCH_CACHE_MB=0, every size has one refillable view."""
    monkeypatch.setenv("SCS_MULTI_SPARSE_NARROW", form)
    if refill:
        monkeypatch.setenv("SCS_SPARSE_BATCH_CACHE_MB", "0")
    N, d, K = shape
    A, Y, x0 = S.sparse_problem(N, d, K)
    rows = _row_lists(N, nrows)
    x = x0 + 0.05 * np.random.default_rng(8).standard_normal(d * K)
    meth = METHODS["lqn"]()
    p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, sparse_f32=f32, sparse_batches=True, **ON)
    p.configure("l1", HM())
    init_method(meth, p)
    full = step(meth, p, "l1", None, x, x, 1)
    p.set_batches(rows)
    got = [step(meth, p, "l1", None, x, x, 1, batch=b) for b in (0, 1, 2, 0)]
    name = p.ctx.kernel_names()[1]
    nviews, vbytes, builds = p.batch_info()
    again = step(meth, p, "l1", None, x, x, 1, batch=-1)
    p.set_batches(None)
    p.ctx.close()
    assert name.startswith("spmv_blk_kernel<" if K == 2 else FORM_KERNEL[form]), name
    # (within the budget -- the sparse data's bytes -- every batch keeps its view; past it, or with a budget of 0,
    # the two lists of one size share a refillable view and batch 0 is built again)
    assert (nviews, builds) in (((2, 4),) if refill else ((3, 3), (2, 4))) and vbytes > 0
    assert np.array_equal(bits(again[0]), bits(full[0])) and again[1] == full[1]
    assert np.array_equal(bits(got[3][0]), bits(got[0][0])) and got[3][1] == got[0][1]
    for b, r in enumerate(rows):
        q = problem("softmax_ce", A[r], Y[r], x0, 2e-3, 1.0 / N, sparse_f32=f32, sparse_outputs=True)
        q.configure("l1", HM())
        init_method(meth, q)
        want = step(meth, q, "l1", None, x, x, 1)
        q.ctx.close()
        assert np.all(np.isfinite(want[0])) and np.any(want[0] != x)
        assert np.array_equal(bits(got[b][0]), bits(want[0])), (b, float(np.max(np.abs(got[b][0] - want[0]))))
        assert got[b][1] == want[1], (b, got[b][1], want[1])


@pytest.mark.parametrize("method,shape,nrows,f32", [
    ("lqn", (300, 130, 3), 137, False), ("nscore", (200, 17, 7), 100, False), ("ggn", (300, 130, 3), 137, False),
    ("ggn", (40, 33, 16), 17, False), ("ggn", (300, 130, 3), 26, True), ("nscore", (520, 129, 2), 260, True),
    ("lqn", (40, 33, 16), 17, True)])
def test_step_on_a_densified_view_is_the_step_on_that_data(method, shape, nrows, f32):
    """The default views: step(..., batch=b) equals bit for bit the step of a fresh dense
    Problem(A[rows_b].toarray(), Y[rows_b]) -- the three methods, ProxGGNSCORE on the feature branch (137 rows
    of (300, 130, 3)) and on the sample-space branch (26 rows of it, 17 of (40, 33, 16); multi_sample=True).
    The generator's A has no duplicate entries.  fp32 values are widened into the fp64 view: the dense context
    holds the same rounded values."""
    N, d, K = shape
    A, Y, x0 = S.sparse_problem(N, d, K)
    assert A.has_canonical_format
    rows = _row_lists(N, nrows)
    if method == "nscore":                               # (fewer rows than columns: a rank-deficient batch Hessian)
        rows = [r for r in rows if len(r) >= d]
    x = x0 + 0.05 * np.random.default_rng(8).standard_normal(d * K)
    meth = METHODS[method]()
    p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, sparse_f32=f32, multi_sample=True, **ON)
    p.configure("l1", HM())
    init_method(meth, p)
    p.set_batches(rows)
    got = [step(meth, p, "l1", None, x, x, 1, batch=b) for b in list(range(len(rows))) + [0]]
    nviews = p.batch_info()[0]
    p.set_batches(None)
    assert p.batch_info()[0] == 0
    p.ctx.close()
    assert nviews == len({len(r) for r in rows})         # one pool view per size
    assert np.array_equal(bits(got[-1][0]), bits(got[0][0])) and got[-1][1] == got[0][1]
    Ad = A.toarray()
    if f32:
        Ad = Ad.astype(np.float32).astype(np.float64)
    for b, r in enumerate(rows):
        q = problem("softmax_ce", Ad[r], Y[r], x0, 2e-3, 1.0 / N, multi_sample=True)
        q.configure("l1", HM())
        init_method(meth, q)
        want = step(meth, q, "l1", None, x, x, 1)
        q.ctx.close()
        assert np.all(np.isfinite(want[0])) and np.any(want[0] != x)
        assert np.array_equal(bits(got[b][0]), bits(want[0])), (b, float(np.max(np.abs(got[b][0] - want[0]))))
        assert got[b][1] == want[1], (b, got[b][1], want[1])


# ---------------------------------------------------------------------------------------------
# 3. trajectories against the oracle
# ---------------------------------------------------------------------------------------------
# views: "dense" the densified default, "sparse" sparse_batches=True (sparse K-column views under ProxLQNSCORE)
TRAJ = ([(c, "lqn", v) for c in D.CASES for v in ("dense", "sparse")] + [(c, "ggn", "dense") for c in D.CASES]
        + [(c, "nscore", "dense") for c in D.NSCORE_CASES] + [(D.CASES[0], "ggn", "sparse")])


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("case,method,views", TRAJ, ids=lambda v: v if isinstance(v, str) else CASE_ID(v))
def test_minibatch_trajectory_vs_oracle(case, method, views, kind):
    """6 epochs of shuffled batches (default_rng(3).permutation(N)), "l1" with PHuberSmootherL1L2(0.5), λ = 2e-3,
    against the oracle's minibatch loop on A.toarray() over the same row lists; the device loop and the host
    loop agree bit for bit.  ProxGGNSCORE (multi_sample=True) takes the branch of D.CASES on each batch --
    (300, 130, 3) / 137: feature, feature, sample; with sparse_batches also on it keeps densified views."""
    (N, d, K), bs = case[0], case[1]
    A, Y, x0 = S.sparse_problem(N, d, K)
    osol = D.oracle_run(kind, method, case[0], bs)
    p = problem(kind, A, Y, x0, 2e-3, 1.0 / N, multi_sample=True, sparse_batches=(views == "sparse"), **ON)
    a = run(method, p, True, **shuffled(N, bs))
    b = run(method, p, False, **shuffled(N, bs))
    p.ctx.close()
    for s in (a, b):
        _compare(s, osol)
    assert a.obj == b.obj and a.pri_res_norm == b.pri_res_norm and np.array_equal(bits(a.x), bits(b.x))


def test_sample_shape_batch_without_multi_sample_is_refused():
    """(300, 130, 3) / 137 with multi_sample off: the third batch (26 rows) raises the sample-space refusal,
    naming the batch's N."""
    N, d, K = 300, 130, 3
    A, Y, x0 = S.sparse_problem(N, d, K)
    p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, **ON)
    with pytest.raises(scsopt.ScsError, match=r"N\*nout \+ 1 = 79 <= d\*nout = 390.*sample-space branch"):
        run("ggn", p, True, **shuffled(N, 137))
    p.ctx.close()


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("method,views", [("ggn", "dense"), ("lqn", "sparse")])
def test_heldout_sparse_set_with_batches(method, views, device_loop):
    """A sparse Atest / ytest (77 x K soft labels) with batches: fvaltest of every pushed point -- on the
    held-out set, not on a batch -- against the oracle, rtol 1e-8."""
    shape = (200, 17, 7)
    N, d, K = shape
    A, Y, x0 = S.sparse_problem(N, d, K)
    At, Yt, _ = S.sparse_problem(77, d, K, soft=True)
    osol = D.oracle_run("softmax_ce", method, shape, 100, test=True)
    p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, Atest=At, ytest=Yt, sparse_batches=(views == "sparse"), **ON)
    sol = run(method, p, device_loop, **shuffled(N, 100))
    p.ctx.close()
    _compare(sol, osol)
    assert len(sol.fvaltest) == len(sol.obj) == len(osol.fvaltest)
    np.testing.assert_allclose(sol.fvaltest, osol.fvaltest, rtol=1e-8)


@pytest.mark.parametrize("views", ["dense", "sparse"])
def test_unshuffled_batches_fp32_and_the_device_door(views):
    """shuffle_batch=False (128, 128, 44 rows of (300, 130, 3)) against the oracle; then fp32 values: the host
    door and the device CSR door (torch.sparse_csr_tensor) give equal bits, and a second run repeats them."""
    import torch
    shape = (300, 130, 3)
    N, d, K = shape
    A, Y, x0 = S.sparse_problem(N, d, K)
    kw = dict(sparse_batches=(views == "sparse"), **ON)
    p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, **kw)
    sol = run("lqn", p, True, batch_size=128, shuffle_batch=False)
    p.ctx.close()
    _compare(sol, D.oracle_run("softmax_ce", "lqn", shape, 128, shuffle=False))
    ph = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, sparse_f32=True, **kw)
    sh = run("lqn", ph, True, max_epoch=4, **shuffled(N, 137))
    sh2 = run("lqn", ph, True, max_epoch=4, **shuffled(N, 137))
    ph.ctx.close()
    _same_bits(sh2, sh)
    At = torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)).cuda(),
                                 torch.from_numpy(A.indices.astype(np.int64)).cuda(),
                                 torch.from_numpy(A.data).to(torch.float32).cuda(), size=A.shape)
    pd = problem("softmax_ce", At, Y, x0, 2e-3, 1.0 / N, sparse_f32=True, **kw)
    sd = run("lqn", pd, True, max_epoch=4, **shuffled(N, 137))
    pd.ctx.close()
    _same_bits(sd, sh)


# ---------------------------------------------------------------------------------------------
# 4. no drift, refusals, the views' bookkeeping
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ggn", "lqn"])
def test_no_drift_on_a_single_output_sparse_context(method):
    """A single-output sparse context with batches: the switch (stored without effect) changes no bit, with
    sparse_batches on (ProxLQNSCORE's sparse views) and off (ProxGGNSCORE's dense views)."""
    N, m = 150, 64
    rng = np.random.default_rng(31)
    A = rng.standard_normal((N, m)) / np.sqrt(m) * (rng.random((N, m)) < 0.3)
    y01 = (rng.random(N) < 0.5).astype(np.float64)
    x0 = 0.2 * rng.standard_normal(m)
    sols = []
    for on in (False, True):
        if method == "ggn":
            p = scsopt.Problem(sp.csr_matrix(A), y01, x0, losses.logistic_ce(1.0 / N), 2e-3,
                               out_fn=losses.sigmoid_ce(1.0 / N), multi_sparse_batches=on)
            meth = scsopt.ProxGGNSCORE()
        else:
            p = scsopt.Problem(sp.csr_matrix(A), y01, x0, losses.least_squares(1.0 / N), 2e-3, sparse_batches=True,
                               multi_sparse_batches=on)
            meth = scsopt.ProxLQNSCORE(m=5)
        sols.append(scsopt.iterate(meth, p, "l1", HM(), max_epoch=4, verbose=0, **shuffled(N, 40)))
        p.ctx.close()
    _same_bits(sols[0], sols[1])


@pytest.mark.parametrize("method", ["ggn", "lqn"])
def test_no_drift_on_a_dense_multi_output_context(method):
    """A dense multi-output context with batches (multi_batches=True): the switch changes no bit."""
    N, d, K = 300, 130, 3
    A, Y, x0 = M.problem(N, d, K)
    sols = []
    for on in (False, True):
        p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, multi_batches=True, multi_sample=True,
                    multi_sparse_batches=on)
        sols.append(run(method, p, True, max_epoch=4, **shuffled(N, 137)))
        p.ctx.close()
    _same_bits(sols[0], sols[1])


def test_refusals_and_the_switch():
    N, d, K = 60, 9, 3
    A, Y, x0 = S.sparse_problem(N, d, K)
    # the switch off: the two existing messages
    p = problem("softmax_ce", A, Y, x0, 1e-3, 1.0 / N, sparse_outputs=True)
    with pytest.raises(scsopt.ScsError, match=r"batch_size / slice_samples.*scs_set_outputs.*multi_batches"):
        run("lqn", p, True, max_epoch=2, batch_size=20)
    p.set_multi_batches(True)
    with pytest.raises(scsopt.ScsError, match=r"need a dense A.*scs_set_multi_batches\).*multi_sparse_batches"):
        run("lqn", p, True, max_epoch=2, batch_size=20)
    # multi_batches stays the gate
    p.set_multi_batches(False)
    p.set_multi_sparse_batches(True)
    with pytest.raises(scsopt.ScsError, match=r"unless multi_batches / scs_set_multi_batches is on"):
        run("lqn", p, True, max_epoch=2, batch_size=20)
    p.set_multi_batches(True)       # both on: accepted
    sol = run("lqn", p, True, max_epoch=2, batch_size=20, shuffle_batch=False)
    assert np.all(np.isfinite(sol.x))
    p.set_batches([np.arange(20)])
    p.set_multi_sparse_batches(False)      # off again with a list registered: the list goes
    with pytest.raises(scsopt.ScsError):
        p.select_batch(0)
    with pytest.raises(IndexError):
        p.get_batch_data(0)
    p.ctx.close()
    # a multi-device context: refused as scs_set_multi_batches is
    with pytest.raises(ValueError, match=r"devices=\[\.\.\.\]"):
        problem("softmax_ce", A.toarray(), Y, x0, 1e-3, 1.0 / N, multi_batches=True, multi_sparse_batches=True,
                devices=[0, 0], device_exchange="host")
    g = _lib.Context(0, devices=[0, 0], device_exchange="host")
    assert _lib.lib.scs_set_multi_sparse_batches(g.h, 1) != 0
    with pytest.raises(scsopt.ScsError, match=r"scs_set_multi_sparse_batches takes a single-device context"):
        g.check(_lib.lib.scs_set_multi_sparse_batches(g.h, 1))
    g.close()


@pytest.mark.parametrize("views", ["dense", "sparse"])
def test_changing_the_switch_drops_the_views_and_clearing_gives_the_bytes_back(views):
    """scs_batch_info counts the new views of both kinds; changing a mode that shapes them (sparse_batches, the
    switch itself) drops them; ctx_bytes returns to its earlier value after the list is cleared."""
    N, d, K = 300, 130, 3
    A, Y, x0 = S.sparse_problem(N, d, K)
    p = problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, sparse_batches=(views == "sparse"), **ON)
    meth = METHODS["lqn"]()
    p.configure("l1", HM())
    init_method(meth, p)
    x = x0.copy()
    step(meth, p, "l1", None, x, x, 1)
    bytes0 = p.data_info()[2]
    rows = _row_lists(N, 137)
    p.set_batches(rows)
    assert p.batch_info()[0] == 0
    for b in range(3):
        step(meth, p, "l1", None, x, x, 1, batch=b)
    nv, vb, _ = p.batch_info()
    assert nv == (3 if views == "sparse" else 2) and vb > 0 and p.data_info()[2] >= bytes0 + vb
    p.set_sparse_batches(views != "sparse")            # the other kind of view: the pooled ones go
    assert p.batch_info()[:2] == (0, 0)
    step(meth, p, "l1", None, x, x, 1, batch=1)
    assert p.batch_info()[0] == 1                      # ... and the next step builds one of the new kind
    p.set_multi_sparse_batches(False)                  # the switch off: the list goes with its views
    assert p.batch_info()[:2] == (0, 0)
    with pytest.raises(scsopt.ScsError):
        p.select_batch(0)
    p.set_multi_sparse_batches(True)
    p.set_batches(rows)
    step(meth, p, "l1", None, x, x, 1, batch=0)
    assert p.batch_info()[0] == 1
    p.set_batches(None)
    assert p.batch_info()[:2] == (0, 0)
    step(meth, p, "l1", None, x, x, 1)
    assert p.data_info()[2] == bytes0
    p.ctx.close()
