"""GPU: minibatches of a sparse A kept sparse under ProxLQNSCORE (scs_set_sparse_batches,
Problem(..., sparse_batches=True)).

The contract of a sparse view is exact: it holds, bit for bit, the two blocked copies that the host
door (scs_set_sparse) builds from A[rows_b, :] -- rows in batch order, a repeated row kept twice, the
stored value type unchanged -- with y[rows_b] and a workspace of its own.  So k consecutive steps on
the selected batch of the big context equal, bit for bit, the same steps of a second context whose
whole data is A[rows_b], y[rows_b] (same loss constant): the first section.  The rest: the loop's
trajectory against the oracle (the bounds of tests/test_gpu_batch.py), the Gram methods untouched,
the view cache, the memory a view takes, two ranks.

The shapes and their edges are stated, and checked on the CPU, in tests/sparse_batch_data.py /
tests/test_sparse_batches_host.py.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch.multiprocessing as mp

import scsopt
from scsopt import losses
from scsopt.iterate import device_optim_loop, init_method, optim_loop, step

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import scsopt_oracle as O  # noqa: E402
import sparse_batch_data as D  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")
HIST = ("obj", "fval", "pri_res_norm", "rel", "objrel", "fvaltest")
LAM = 1e-3
K_STEPS = 3   # the L-BFGS memory and the BB step take part from the second step on


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def hmu():
    return scsopt.PHuberSmootherL1L2(1.0)


def lqn():
    return scsopt.ProxLQNSCORE(m=5)


def hist_of(sol):
    out = {k: np.array([np.nan if v is None else v for v in getattr(sol, k)], dtype=np.float64) for k in HIST}
    out["x"] = np.array(sol.x)
    out["epochs"] = sol.epochs
    return out


def assert_same(a, b, what="", loops_differ=False):
    """Bit equality of x and every history.  loops_differ: one run in the library's loop, one in the
    Python loop -- `rel` is then ‖x − x*‖ summed in another order (scs_iterate's note; the steps, and
    so x, obj, fval and pri_res_norm, are the same device calls), and is held to 4 ulp instead."""
    assert a["epochs"] == b["epochs"], what
    for k in HIST + ("x",):
        if loops_differ and k == "rel":
            np.testing.assert_allclose(a[k], b[k], rtol=4 * np.finfo(float).eps, atol=0)
            continue
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, a[k], b[k])


# ---- 1. the bits of a view ---------------------------------------------------------------------------
def _steps(p, x0, batch=None):
    """K_STEPS consecutive ProxLQNSCORE steps from x0 (fresh memory): the iterates and pri_res_norm."""
    meth = lqn()
    p.configure("l1", hmu())
    init_method(meth, p)
    x_prev, x, out = x0, x0, []
    for it in range(1, K_STEPS + 1):
        xn, pri = step(meth, p, "l1", None, x, x_prev, it, batch=batch)
        out.append((xn, pri))
        x_prev, x = x, xn
    return out


def _check_views(case, sparse_f32=False, compute_f32=False):
    A, y, x0, batches = D.case(case)
    N = A.shape[0]
    f = losses.least_squares(1.0 / N)
    big = scsopt.Problem(A, y, x0, f, LAM, sparse_batches=True, sparse_f32=sparse_f32)
    if compute_f32:
        big.set_compute_f32(True)
    big.set_batches(batches)
    try:
        for bi, rows in enumerate(batches):
            got = _steps(big, x0, batch=bi)
            ref_p = scsopt.Problem(A[rows], y[rows], x0, f, LAM, sparse_f32=sparse_f32)   # the same loss constant
            if compute_f32:
                ref_p.set_compute_f32(True)
            ref = _steps(ref_p, x0)
            ref_p.ctx.close()
            for it, ((xg, pg), (xr, pr)) in enumerate(zip(got, ref)):
                assert np.all(np.isfinite(xr)), (case, bi, it)
                assert np.array_equal(bits(xg), bits(xr)), (case, bi, len(rows), it, np.max(np.abs(xg - xr)))
                assert np.array_equal(bits(pg), bits(pr)), (case, bi, len(rows), it, pg, pr)
        nviews, vbytes, builds = big.batch_info()
        assert builds == len(batches) and nviews >= 1 and vbytes > 0
    finally:
        big.set_batches(None)
        big.ctx.close()


@pytest.mark.parametrize("case", ["partial", "two_col_blocks", "two_row_blocks"])
def test_view_steps_equal_the_sliced_problem(case):
    """partial: N = 1500, m = 96, shuffled batches of 400 (the last one 300 rows), one batch with a row
    twice, one batch of empty rows only (nnz_b = 0).  two_col_blocks: N = 2100, m = 16384 + 130 (two
    column blocks in the row copy, the edge of the x-slice staging), batches of 1, 63, 64, 65, 1024 and
    1025 rows (the wave edge and the workgroup edge of the slice kernel), a fully dense row in two of
    them.  two_row_blocks: N = 40000, m = 48, one batch of 16384 + 40 rows (two row blocks in the
    batch's column copy)."""
    _check_views(case)


@pytest.mark.parametrize("compute_f32", [False, True], ids=["fp64_arith", "fp32_arith"])
def test_view_steps_fp32_stored(compute_f32):
    """fp32-stored values (8-entry slots, 16-byte index granules), with and without fp32 arithmetic."""
    _check_views("partial", sparse_f32=True, compute_f32=compute_f32)


# ---- 2. trajectory -----------------------------------------------------------------------------------
def _traj_problem(**kw):
    """tests/test_gpu_batch.py::test_sparse_minibatches_gathered_dense[lqn]"""
    N, m = 1500, 96
    rng = np.random.default_rng(17)
    A = sp.random(N, m, density=0.08, random_state=3, format="csr") * 3.0
    x0 = rng.standard_normal(m) * 0.3
    y = rng.standard_normal(N)
    perm = np.random.default_rng(4).permutation(N)
    return A, y, x0, perm, N


def _traj_run(p, perm, device_loop=None):
    return scsopt.iterate(lqn(), p, "l1", hmu(), batch_size=400, batch_perm=perm, max_epoch=5, verbose=0,
                          device_loop=device_loop)


@pytest.mark.parametrize("held_out", [False, True], ids=["train_only", "held_out"])
def test_trajectory_vs_oracle(held_out):
    A, y, x0, perm, N = _traj_problem()
    kw, okw = {}, {}
    if held_out:
        rng = np.random.default_rng(23)
        At = sp.random(211, A.shape[1], density=0.08, random_state=5, format="csr") * 3.0
        yt = rng.standard_normal(211)
        kw, okw = dict(Atest=At, ytest=yt), dict(Atest=At.toarray(), ytest=yt)
    p = scsopt.Problem(A, y, x0, losses.least_squares(1.0 / N), LAM, sparse_batches=True, **kw)
    om = O.Problem(A.toarray(), y, x0, O.Loss("least_squares", 1.0 / N), LAM, **okw)
    a = _traj_run(p, perm, device_loop=True)
    b = _traj_run(p, perm, device_loop=False)
    o = O.iterate(O.ProxLQNSCORE(m=5), om, "l1", O.PHuberSmootherL1L2(1.0), max_epoch=5,
                  batches=O.loader_batches(N, 400, perm=perm))
    for s in (a, b):
        assert s.epochs == o.epochs and len(s.obj) == len(o.obj)
        np.testing.assert_allclose(s.obj, o.obj, rtol=1e-8)
        np.testing.assert_allclose(s.x, o.x, rtol=1e-6, atol=1e-9)
        if held_out:
            assert len(s.fvaltest) == len(s.obj)
            np.testing.assert_allclose(s.fvaltest, o.fvaltest, rtol=1e-8)
    assert_same(hist_of(a), hist_of(b), "device loop vs host loop", loops_differ=True)
    # f and get_reg of the histories come from the full data, whatever batch stepped last
    p.configure("l1", hmu())
    assert a.fval[0] == p.fx(x0) and a.obj[0] == p.fx(x0) + p.get_reg(x0)
    assert a.fval[-1] != a.fval[0]
    np.testing.assert_allclose(a.fval, o.fval, rtol=1e-8)
    # the steps ran on sparse views: the same loop with the switch off gives another rounding
    q = scsopt.Problem(A, y, x0, losses.least_squares(1.0 / N), LAM, **kw)
    d = _traj_run(q, perm)
    np.testing.assert_allclose(a.obj, d.obj, rtol=1e-8)


def test_trajectory_samplewise_host_equals_menu():
    """A sample-wise least-squares loss in host mode on sparse views equals the menu kind bit for bit, as
    tests/test_gpu_samplewise.py has it for dense batches: every history on that file's kind of data
    (the trajectory problem's pattern with small integers and a power-of-two constant, where both
    forms of the loss round alike), and x and pri_res_norm on the trajectory problem itself."""
    S, y, x0, perm, c8 = D.int_traj_data()

    def value(z, yy):
        r = z - yy
        return (0.5 * c8) * (r * r)
    sw = losses.samplewise(value, lambda z, yy: c8 * (z - yy), lambda z, yy: c8, device=False)
    ref = hist_of(_traj_run(scsopt.Problem(S, y, x0, losses.least_squares(c8), 2e-3, sparse_batches=True), perm))
    got = hist_of(_traj_run(scsopt.Problem(S, y, x0, sw, 2e-3, sparse_batches=True), perm))
    assert_same(got, ref)
    assert np.all(np.isfinite(got["x"])) and got["epochs"] == 5
    # the trajectory problem itself (real values, constant 1/N): every step, and so x and pri_res_norm,
    # bit for bit; f of the histories differs in the last bit there (1.1e-16 relative with dense
    # batches, 1.6e-16 with sparse views): 0.5·c·Σr² on the device against Σ 0.5·c·r² of the callable
    A, y, x0, perm, N = _traj_problem()
    c = 1.0 / N
    sw = losses.samplewise(lambda z, yy: (0.5 * c) * ((z - yy) * (z - yy)), lambda z, yy: c * (z - yy),
                           lambda z, yy: c, device=False)
    ref = hist_of(_traj_run(scsopt.Problem(A, y, x0, losses.least_squares(c), LAM, sparse_batches=True), perm))
    got = hist_of(_traj_run(scsopt.Problem(A, y, x0, sw, LAM, sparse_batches=True), perm))
    assert got["epochs"] == ref["epochs"]
    for k in ("x", "pri_res_norm"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    np.testing.assert_allclose(got["fval"], ref["fval"], rtol=4 * np.finfo(float).eps, atol=0)


# ---- 3. the other methods are untouched -------------------------------------------------------------
@pytest.mark.parametrize("method", ["ggn", "nscore"])
def test_gram_methods_keep_the_dense_view(method):
    A, _, x0, perm, N = _traj_problem()
    y = (np.random.default_rng(17).random(N) < 0.5).astype(float)
    if method == "ggn":
        f, out, meth = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N), scsopt.ProxGGNSCORE
    else:
        f, out, meth = losses.logistic_margin(1.0 / N), None, scsopt.ProxNSCORE
        y = 2.0 * y - 1.0
    batches = O.loader_batches(N, 400, perm=perm)
    res = []
    for on in (False, True):
        p = scsopt.Problem(A, y, x0, f, LAM, out_fn=out, sparse_batches=on)
        p.set_batches(batches)
        try:
            res.append(hist_of(optim_loop(meth(), p, "l1", hmu(), max_epoch=3, verbose=0, nbatch=len(batches))))
            assert p.batch_info() == (0, 0, 0)   # no sparse view was built
        finally:
            p.set_batches(None)
            p.ctx.close()
    assert_same(res[0], res[1], method)
    assert np.all(np.isfinite(res[1]["x"]))


# ---- 4. the cache -------------------------------------------------------------------------------------
def _cache_run(monkeypatch, cache_mb):
    A, y, x0, perm, N = _traj_problem()
    if cache_mb is None:
        monkeypatch.delenv("SCS_SPARSE_BATCH_CACHE_MB", raising=False)
    else:
        monkeypatch.setenv("SCS_SPARSE_BATCH_CACHE_MB", cache_mb)
    p = scsopt.Problem(A, y, x0, losses.least_squares(1.0 / N), LAM, sparse_batches=True)
    p.configure("l1", hmu())
    init_method(lqn(), p)
    step(lqn(), p, "l1", None, x0, x0, 1)      # the full-data step's own scratch exists before the baseline
    base = p.data_info()[2]
    batches = O.loader_batches(N, 400, perm=perm)
    assert len(batches) == 4
    p.set_batches(batches)
    sol = hist_of(device_optim_loop(lqn(), p, "l1", hmu(), max_epoch=3, verbose=0))
    info = p.batch_info()
    held = p.data_info()[2]
    p.set_batches(None)
    after = p.data_info()[2]
    assert p.batch_info()[0] == 0 and p.batch_info()[1] == 0
    p.ctx.close()
    return sol, info, (base, held, after)


def test_views_are_kept_per_batch(monkeypatch):
    sol, (nviews, vbytes, builds), (base, held, after) = _cache_run(monkeypatch, None)
    assert builds == 4 and nviews == 4          # three epochs over four batches: each view built once
    assert held >= base + vbytes > base
    assert after == base                         # set_batches(None) frees the views and their scratch
    sol0, (nv0, _, builds0), (base0, _, after0) = _cache_run(monkeypatch, "0")
    assert builds0 > 4 and nv0 == 2              # one refillable view per size (400 and 300 rows)
    assert after0 == base0
    assert_same(sol0, sol, "refilled views vs kept views")


# ---- 5. memory ------------------------------------------------------------------------------------------
def test_view_bytes_far_below_the_dense_view():
    """N = 8192, m = 131072, 8 entries per row, batches of 4096: the dense view is 4096·131072·8 B =
    4 GiB; the sparse view (a few MB by the layout's arithmetic) and its scratch stay under 1/16 of it."""
    A, y, x0, batches = D.case("wide")
    N, m = A.shape
    p = scsopt.Problem(A, y, x0, losses.least_squares(1.0 / N), LAM, sparse_batches=True)
    p.configure("l1", hmu())
    init_method(lqn(), p)
    base = p.data_info()[2]
    p.set_batches(batches)
    try:
        xn, pri = step(lqn(), p, "l1", None, x0, x0, 1, batch=0)
        grown = p.data_info()[2] - base
        nviews, vbytes, builds = p.batch_info()
    finally:
        p.set_batches(None)
        p.ctx.close()
    assert np.all(np.isfinite(xn)) and np.isfinite(pri)
    assert (nviews, builds) == (1, 1)
    assert 0 < vbytes <= grown < 4096 * 131072 * 8 // 16, (vbytes, grown)


# ---- 6. two ranks on one GPU --------------------------------------------------------------------------
SN = 1500


def _shard_data():
    A, y, x0, _, N = _traj_problem()
    rng = np.random.default_rng(31)
    # the first batch (300 rows) lies on rank 0 alone: rank 1 holds an empty view of it
    first = rng.permutation(N // 2)[:300]
    rest = rng.permutation(np.setdiff1d(np.arange(N), first))
    return A, y, x0, np.concatenate([first, rest])


def _shard_run(comm=None):
    A, y, x0, perm = _shard_data()
    f = losses.least_squares(1.0 / SN)
    if comm is None:
        p = scsopt.Problem(A, y, x0, f, LAM, sparse_batches=True)
    else:
        from scsopt.shard import row_range
        r0, r1 = row_range(SN, comm.world, comm.rank)
        assert perm[:300].max() < row_range(SN, comm.world, 0)[1]
        p = scsopt.Problem(A[r0:r1], y[r0:r1], x0, f, LAM, comm=comm, N_global=SN, row0=r0, sparse_batches=True)
    sol = scsopt.iterate(lqn(), p, "l1", hmu(), batch_size=300, batch_perm=perm, max_epoch=4, verbose=0)
    res = {"obj": list(sol.obj), "x": sol.x.copy(), "epochs": sol.epochs}
    p.ctx.close()
    return res


def _shard_worker(rank, world, store_path, out):
    sys.path.insert(0, PKG)
    import torch
    import torch.distributed as dist
    from scsopt import shard
    dist.init_process_group("gloo", store=dist.FileStore(store_path, world), rank=rank, world_size=world)
    out[rank] = _shard_run(shard.Comm(device=torch.device("cuda", 0)))
    dist.destroy_process_group()


def test_two_ranks_one_batch_on_rank_0_alone(tmp_path):
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(2, str(tmp_path / "store"), out), nprocs=2, join=True)
    full = _shard_run()
    r0, r1 = out[0], out[1]
    assert r0["epochs"] == r1["epochs"] == full["epochs"]
    assert r0["obj"] == r1["obj"] and np.array_equal(bits(r0["x"]), bits(r1["x"]))   # identical bits on both ranks
    np.testing.assert_allclose(r0["obj"], full["obj"], rtol=1e-10)
    np.testing.assert_allclose(r0["x"], full["x"], rtol=1e-8, atol=1e-12)


# ---- 7. the data in place comes back -------------------------------------------------------------------
# batch_info() after the two ProxLQNSCORE views, after the two sample-space views, at the end
VIEW_INFO = ((2, 26272, 2), (2, 29360, 2), (1, 8080, 3))


def test_data_in_place_restored_after_every_kind_of_view():
    """One context, every kind of view built and used on it in turn (a dense batch view, a sparse one,
    its sample-space form, a sparse held-out set, a step that fails with a batch view in place): after
    each, f(x0), ∇f(x0), the CSR and y read back and the dense block's data_info are, bit for bit,
    what they were before any view existed.  (data_info()[2], the bytes the context holds, grows with
    the views kept and is not part of the comparison.)

    N = 300, m = 40, 6 entries per row, row 7 empty, 17 held-out rows; batches of 64, 64, 64, 64 and 44
    rows.  With m = 40 none of those takes ProxGGNSCORE's sample-space branch (n_b + 1 <= m), so that
    step runs on a second list with batches of 30 and 39 = m - 1 rows.  The views' count, bytes and
    builds are the figures the commit before the view's one definition gives for this sequence."""
    N, m = 300, 40
    rng = np.random.default_rng(41)
    A = (sp.random(N, m, density=6.0 / m, random_state=9, format="csr") * 2.0).tolil()
    A[7, :] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    assert A[7].nnz == 0 and 5.0 < A.nnz / N < 7.0
    y = (rng.random(N) < 0.5).astype(float)
    x0 = rng.standard_normal(m) * 0.3
    At = sp.random(17, m, density=6.0 / m, random_state=10, format="csr") * 2.0
    yt = (rng.random(17) < 0.5).astype(float)
    perm = rng.permutation(N)
    batches = [perm[i:i + 64] for i in range(0, N, 64)]
    assert [b.size for b in batches] == [64, 64, 64, 64, 44]
    small = [perm[:30], perm[100:139]]
    p = scsopt.Problem(A, y, x0, losses.logistic_ce(1.0 / N), LAM, out_fn=losses.sigmoid_ce(1.0 / N), Atest=At, ytest=yt)
    p.configure("l1", hmu())

    def state():
        S, ys = p.get_sparse()
        return (bits(p.fx(x0)), bits(p.gradx(x0)), S.indptr.copy(), S.indices.copy(), bits(S.data), bits(ys),
                np.array(p.data_info()[:2]), np.array([p.N, p.nnz]))
    before = state()
    assert np.isfinite(p.fx(x0)) and np.all(np.isfinite(p.gradx(x0)))

    def unchanged(what):
        for i, (a, b) in enumerate(zip(before, state())):
            assert np.array_equal(a, b), (what, i)

    def one_step(meth, batch):
        init_method(meth, p)
        xn, pri = step(meth, p, "l1", hmu(), x0, x0, 1, batch=batch)
        assert np.all(np.isfinite(xn)) and np.isfinite(pri), (type(meth).__name__, batch)
    try:
        p.set_batches(batches)
        one_step(lqn(), 0)
        unchanged("dense batch view")
        assert p.batch_info() == (0, 0, 0)
        p.set_sparse_batches(True)
        one_step(lqn(), 1)
        unchanged("sparse batch view")
        one_step(lqn(), 4)
        unchanged("sparse batch view, 44 rows")
        info_lqn = p.batch_info()
        p.set_sparse_sample(True)
        p.set_batches(small)
        for b in (0, 1):
            one_step(scsopt.ProxGGNSCORE(), b)
            unchanged("sample-space view %d" % b)
        info_ggn = p.batch_info()
        ft = p.ftest(x0)
        unchanged("held-out set")
        assert np.isfinite(ft) and ft == p.ftest(x0)
        p.select_batch(1)
        p.select_batch(-1)
        unchanged("select_batch(-1)")
        init_method(scsopt.ProxGGNSCORE(ss_type=4), p)   # refused at the step size, with the view in place
        with pytest.raises(scsopt.ScsReferenceError, match="ss_type"):
            step(scsopt.ProxGGNSCORE(ss_type=4), p, "l1", hmu(), x0, x0, 1, batch=0)
        p.select_batch(-1)
        unchanged("a step that failed on a batch view")
        one_step(lqn(), 0)      # the context is still usable, and the data still comes back
        unchanged("the step after the failure")
        print("batch_info", info_lqn, info_ggn, p.batch_info())
        assert (info_lqn, info_ggn, p.batch_info()) == VIEW_INFO
    finally:
        p.set_batches(None)
        p.ctx.close()
