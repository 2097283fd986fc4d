"""GPU: minibatches of a multi-output loss on a dense A (scs_set_multi_batches / multi_batches=True).
csrc/multi.hip's one-launch gather of a batch's rows of A and of Y against exact integers (both arms of
SCS_MULTI_GATHER, both storage types), a step on a batch view against the step of a context holding
that batch, and the minibatch trajectories of the three methods -- ProxGGNSCORE choosing its branch per
batch -- against the oracle's optim_loop! over the same row lists (tests/multi_batches_data.py; the
oracle's side of every comparison is checked on the CPU in test_multi_batches_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scsopt
from scsopt import losses
from scsopt.iterate import init_method, step

import multi_batches_data as B
import multi_output_data as M
from multi_batches_data import O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "selfconcordantsmoothoptimization.jl_amd")
HM = lambda: scsopt.PHuberSmootherL1L2(0.5)      # noqa: E731
METHODS = {"ggn": scsopt.ProxGGNSCORE, "nscore": scsopt.ProxNSCORE, "lqn": lambda **kw: scsopt.ProxLQNSCORE(m=5, **kw)}
CASE_ID = lambda c: "x".join(map(str, c[0]))     # noqa: E731


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("SCS_"):
            monkeypatch.delenv(k)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_problem(kind, A, Y, x0, lam, c, **kw):
    f, out_fn = M.device_losses(losses, kind, Y.shape[1], c)
    kw.setdefault("multi_batches", True)
    return scsopt.Problem(A, Y, x0, f, lam, out_fn=out_fn, **kw)


def run(method, p, device_loop, max_epoch=6, **kw):
    return scsopt.iterate(METHODS[method](), p, "l1", HM(), max_epoch=max_epoch, verbose=0, device_loop=device_loop,
                          **kw)


def shuffled(N, bs):
    return dict(batch_size=bs, shuffle_batch=True, batch_perm=B.perm_of(N))


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
# 1. the gather, exactly
# ---------------------------------------------------------------------------------------------
def _gather_fails(got, ref, tag):
    fails = []
    for b, ((Ab, Yb), (Ar, Yr)) in enumerate(zip(got, ref)):
        if Ab.shape != Ar.shape or Yb.shape != Yr.shape:
            fails.append(f"{tag} batch {b}: shapes {Ab.shape} {Yb.shape}")
        elif not (np.array_equal(bits(Ab), bits(Ar)) and np.array_equal(bits(Yb), bits(Yr))):
            fails.append(f"{tag} batch {b} (n_b = {len(Ar)}): {int(np.sum(Ab != Ar))} entries of A, "
                         f"{int(np.sum(Yb != Yr))} of Y differ")
    return fails


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("d", B.GATHER_D)
def test_gather_exact_integers(d, f32):
    """get_batch_data(b) == (A[rows_b], Y[rows_b]) bit for bit: integer A (±8191, exact in fp32) and Y, N = 100
    (no multiple of 16), n_b = 33, 16, 16, 17, 15, 1 and the first 16-row batch again (B.gather_lists: row
    N - 1, repeated rows, unsorted lists, one pool view gathered three times, smaller after larger), d of
    one column, one short of / exactly / one past a panel and a third panel, K = 2, 3, 16."""
    fails = []
    for K in B.GATHER_K:
        got, ref = B.gather_all(scsopt, losses, d, K, f32)
        fails += _gather_fails(got, ref, f"K={K}")
    assert not fails, "\n".join(fails)


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import torch  # noqa: F401
import scsopt
from scsopt import losses
import multi_batches_data as B
out = {}
for f32 in (False, True):
    for d in B.GATHER_D:
        for K in B.GATHER_K:
            got, _ = B.gather_all(scsopt, losses, d, K, f32)
            for b, (Ab, Yb) in enumerate(got):
                out[f"A_{int(f32)}_{d}_{K}_{b}"] = Ab
                out[f"Y_{int(f32)}_{d}_{K}_{b}"] = Yb
np.savez(sys.argv[3], **out)
"""


def test_gather_arms_write_the_same_bits(tmp_path):
    """SCS_MULTI_GATHER=1 (multi.hip's one-launch kernel) and =0 (gather_rows_kernel over the d-column view
    plus one launch per further target column), each in a fresh process over the whole matrix of the test
    above: both exact, hence equal."""
    outs = []
    for arm in ("1", "0"):
        fout = tmp_path / f"arm{arm}.npz"
        env = {k: v for k, v in os.environ.items() if not k.startswith("SCS_")}
        env["SCS_MULTI_GATHER"] = arm
        subprocess.run([sys.executable, "-c", _CHILD, PKG, os.path.join(ROOT, "tests"), str(fout)], env=env,
                       check=True, timeout=300)
        outs.append(np.load(fout))
    assert sorted(outs[0].files) == sorted(outs[1].files) and len(outs[0].files) == 2 * 2 * 5 * 3 * 7
    lists = B.gather_lists()
    lists.append(lists[1])
    fails = []
    for f32 in (False, True):
        for d in B.GATHER_D:
            for K in B.GATHER_K:
                A, Y = B.gather_data(d, K, f32)
                for b, r in enumerate(lists):
                    for nm, want in ((f"A_{int(f32)}_{d}_{K}_{b}", A.astype(np.float64)[r]),
                                     (f"Y_{int(f32)}_{d}_{K}_{b}", Y[r])):
                        for arm in (0, 1):
                            if not np.array_equal(bits(outs[arm][nm]), bits(want)):
                                fails.append(f"{nm} arm {1 - arm}")
    assert not fails, fails[:20]


def test_gather_door_on_a_single_output_context():
    """The same door on a context without nout (the unchanged single-output gather), fp64 and fp32, and the
    selection is left as it was: a step after the read is the step on the batch selected before it."""
    N, d = B.GATHER_N, 129
    lists = B.gather_lists()
    for f32 in (False, True):
        A, _ = B.gather_data(d, 2, f32)
        y = np.random.default_rng(2).integers(-9, 10, size=N).astype(np.float64)
        p = scsopt.Problem(A, y, np.zeros(d), losses.least_squares(1.0 / N), 1e-3, dense_f32=f32)
        p.set_batches(lists)
        fails = []
        for b, r in enumerate(lists):
            Ab, yb = p.get_batch_data(b)
            if not (np.array_equal(bits(Ab), bits(A.astype(np.float64)[r])) and np.array_equal(bits(yb), bits(y[r]))):
                fails.append(b)
        assert not fails, (f32, fails)
        p.configure("l1", HM())
        meth = scsopt.ProxLQNSCORE(m=3)
        init_method(meth, p)
        x = 0.1 * np.random.default_rng(4).standard_normal(d)
        want = step(meth, p, "l1", None, x, x, 1, batch=3)
        p.select_batch(3)
        p.get_batch_data(0)                                    # another pool view, then batch 3 again
        p.get_batch_data(4)
        xn, pri = step(meth, p, "l1", None, x, x, 1)           # (no batch=: the selection made above)
        assert np.array_equal(bits(xn), bits(want[0])) and pri == want[1]
        with pytest.raises(IndexError):
            p.get_batch_data(len(lists))
        p.ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. a step on a view is the step on that data
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,shape,nrows,f32", [
    ("lqn", (300, 130, 3), 137, False), ("nscore", (300, 130, 3), 137, False), ("ggn", (300, 130, 3), 137, False),
    ("ggn", (129, 260, 2), 48, False), ("ggn", (40, 33, 16), 17, False), ("ggn", (300, 130, 3), 137, True),
    ("ggn", (129, 260, 2), 48, True)])
def test_step_on_a_view_is_the_step_on_that_data(method, shape, nrows, f32):
    """A pool view is sized by the functions that size a context holding n_b rows, and the gather writes the
    layout the data door writes: step(..., batch=b) equals bit for bit (x_new, pri) the step of a fresh
    Problem(A[rows_b], Y[rows_b]) with the same loss objects (scale 1/N of the full data), options and x.
    137 strided rows of (300, 130, 3): the feature branch; 48 rows of (129, 260, 2) and 17 of (40, 33, 16):
    ProxGGNSCORE's sample-space branch (multi_sample=True).  Two lists of the same size share one pool view
    (the second step re-gathers, and re-transposes the view's Aᵀ copy in the sample-space cases).  Then
    batch=-1 equals the step taken before any list was registered."""
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    if f32:
        A = A.astype(np.float32)
    sample = nrows * K + 1 <= d * K
    assert sample == (method == "ggn" and shape != (300, 130, 3))
    stride = N // nrows
    rows = [np.arange(0, stride * nrows, stride)[::-1].copy(), (np.arange(nrows) * 7 + 3) % N]
    assert all(len(r) == nrows for r in rows)
    x = x0 + 0.05 * np.random.default_rng(8).standard_normal(d * K)
    kw = dict(multi_sample=True, dense_f32=f32)
    meth = METHODS[method]()
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, **kw)
    p.configure("l1", HM())
    init_method(meth, p)
    full = step(meth, p, "l1", None, x, x, 1)
    p.set_batches(rows)
    got = [step(meth, p, "l1", None, x, x, 1, batch=b) for b in (0, 1, 0)]
    again = step(meth, p, "l1", None, x, x, 1)
    p.set_batches(None)
    p.ctx.close()
    assert np.array_equal(bits(again[0]), bits(full[0])) and again[1] == full[1]
    assert np.array_equal(bits(got[2][0]), bits(got[0][0])) and got[2][1] == got[0][1]
    for b, r in enumerate(rows):
        q = device_problem("softmax_ce", A[r], Y[r], x0, 2e-3, 1.0 / N, **kw)
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
TRAJ = [(c, m) for c in B.CASES for m in ("lqn", "ggn")] + [(c, "nscore") for c in B.NSCORE_CASES]


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("case,method", TRAJ, ids=lambda v: v if isinstance(v, str) else CASE_ID(v))
def test_minibatch_trajectory_vs_oracle(case, method, kind):
    """6 epochs of shuffled batches (default_rng(3).permutation(N)), "l1" with PHuberSmootherL1L2(0.5), λ = 2e-3,
    against the oracle on the same row lists; the device loop and the host loop agree bit for bit.
    ProxGGNSCORE (multi_sample=True) takes the branch of B.CASES on each batch -- (300, 130, 3) / 137 mixes
    both within an epoch; ProxNSCORE runs where every batch has n_b >= d."""
    (N, d, K), bs = case[0], case[1]
    A, Y, x0 = M.problem(N, d, K)
    osol = B.oracle_run(kind, method, case[0], bs)
    p = device_problem(kind, A, Y, x0, 2e-3, 1.0 / N, multi_sample=True)
    a = run(method, p, True, **shuffled(N, bs))
    b = run(method, p, False, **shuffled(N, bs))
    p.ctx.close()
    for s in (a, b):
        _compare(s, osol)
    assert a.obj == b.obj and a.pri_res_norm == b.pri_res_norm and np.array_equal(bits(a.x), bits(b.x))


def test_minibatch_prox_support_is_not_trivial():
    """λ = 2e-2, ProxGGNSCORE softmax on (300, 130, 3) / 137: some but not all entries of x are exactly zero."""
    (N, d, K), bs = B.CASES[0][0], B.CASES[0][1]
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-2, 1.0 / N, multi_sample=True)
    sol = run("ggn", p, True, **shuffled(N, bs))
    p.ctx.close()
    _compare(sol, B.oracle_run("softmax_ce", "ggn", (N, d, K), bs, 2e-2))
    zeros = int(np.sum(sol.x == 0.0))
    assert 0 < zeros < d * K, zeros


# ---------------------------------------------------------------------------------------------
# 4. loader options
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("method", ["ggn", "lqn"])
def test_slice_samples(method, device_loop):
    """slice_samples=True: one-row batches of which only the first ever steps (iterate.jl:127,136-138,146); a
    one-row batch is ProxGGNSCORE's sample-space shape (K + 1 <= d K)."""
    shape = (200, 17, 7)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    assert [len(r) for r in O.loader_batches(N, slice_samples=True)] == [1]
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, multi_sample=True)
    sol = run(method, p, device_loop, slice_samples=True)
    p.ctx.close()
    _compare(sol, B.oracle_run("softmax_ce", method, shape, None, loader=(("slice_samples", True),)))


@pytest.mark.parametrize("device_loop", [False, True])
def test_unshuffled_batches_and_local_max_iter(device_loop):
    """shuffle_batch=False keeps the row order (128, 128, 44 rows of (300, 130, 3)); local_max_iter = 2.7 forces
    max_epoch = 1 and runs the first two batches only (iterate.jl:66,124-128)."""
    shape = (300, 130, 3)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
    base = (("batch_size", 128), ("shuffle_batch", False))
    assert len(O.loader_batches(N, 128, shuffle_batch=False, local_max_iter=2.7)) == 2
    sol = run("lqn", p, device_loop, batch_size=128, shuffle_batch=False)
    _compare(sol, B.oracle_run("softmax_ce", "lqn", shape, None, 2e-3, 6, False, base))
    sol = scsopt.iterate(METHODS["lqn"](), p, "l1", HM(), verbose=0, device_loop=device_loop, batch_size=128,
                         shuffle_batch=False, local_max_iter=2.7)
    p.ctx.close()
    _compare(sol, B.oracle_run("softmax_ce", "lqn", shape, None, 2e-3, 1, False, base + (("local_max_iter", 2.7),)))


def test_one_shuffled_full_batch():
    """batch_size = N: one batch holding every row in the shuffled order (the feature branch)."""
    shape = (200, 17, 7)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N)
    sol = run("ggn", p, True, **shuffled(N, N))
    p.ctx.close()
    _compare(sol, B.oracle_run("softmax_ce", "ggn", shape, N))


# ---------------------------------------------------------------------------------------------
# 5. the held-out set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_loop", [False, True])
def test_heldout_fvaltest_with_batches(device_loop):
    """Atest / ytest (77 x K soft labels) with batches: fvaltest of every pushed point -- on the held-out set,
    not on a batch -- against the oracle, rtol 1e-8."""
    shape = (200, 17, 7)
    N, d, K = shape
    A, Y, x0 = M.problem(N, d, K)
    At, Yt, _ = M.problem(77, d, K, soft=True)
    osol = B.oracle_run("softmax_ce", "ggn", shape, 50, test=True)
    p = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, Atest=At, ytest=Yt)
    sol = run("ggn", p, device_loop, **shuffled(N, 50))
    p.ctx.close()
    _compare(sol, osol)
    assert len(sol.fvaltest) == len(sol.obj) == len(osol.fvaltest)
    np.testing.assert_allclose(sol.fvaltest, osol.fvaltest, rtol=1e-8)


# ---------------------------------------------------------------------------------------------
# 6. fp32 storage, 7. the device door, 8. run to run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ggn", "lqn"])
def test_dense_f32_equals_widened_values(method):
    """An fp32-stored context (fp32 batch views) gives bit for bit the minibatch trajectory of an fp64-stored
    context holding the same values widened; ProxGGNSCORE on (300, 130, 3) / 137 runs both branches."""
    N, d, K = 300, 130, 3
    A, Y, x0 = M.problem(N, d, K)
    A32 = A.astype(np.float32)
    sols = []
    for Ain, f32 in ((A32, True), (A32.astype(np.float64), False)):
        p = device_problem("softmax_ce", Ain, Y, x0, 2e-3, 1.0 / N, dense_f32=f32, multi_sample=True)
        assert p.data_info()[0] == (4 if f32 else 8)
        sols.append(run(method, p, True, max_epoch=4, **shuffled(N, 137)))
        p.ctx.close()
    _same_bits(sols[0], sols[1])


def test_device_door_equals_host_door_and_repeats():
    """A row-major fp64 torch A on the GPU gives bit for bit the host door's minibatch trajectory, and the
    same call twice on one context gives equal bits."""
    N, d, K = 300, 130, 3
    A, Y, x0 = M.problem(N, d, K)
    ph = device_problem("softmax_ce", A, Y, x0, 2e-3, 1.0 / N, multi_sample=True)
    sh = run("ggn", ph, True, max_epoch=4, **shuffled(N, 137))
    sh2 = run("ggn", ph, True, max_epoch=4, **shuffled(N, 137))
    ph.ctx.close()
    _same_bits(sh2, sh)
    At = torch.from_numpy(A).cuda()
    assert tuple(At.shape) == (N, d) and At.stride() == (d, 1) and At.dtype == torch.float64
    pd = device_problem("softmax_ce", At, Y, x0, 2e-3, 1.0 / N, multi_sample=True)
    sd = run("ggn", pd, True, max_epoch=4, **shuffled(N, 137))
    pd.ctx.close()
    _same_bits(sd, sh)


# ---------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals():
    import scipy.sparse as sp
    N, d, K = 60, 9, 3
    A, Y, x0 = M.problem(N, d, K)
    f, of = M.device_losses(losses, "softmax_ce", K, 1.0 / N)
    # the switch off: the old text, now with a pointer to the switch
    p = scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of)
    with pytest.raises(scsopt.ScsError, match=r"batch_size / slice_samples.*scs_set_outputs.*multi_batches"):
        scsopt.iterate(scsopt.ProxLQNSCORE(m=3), p, "l1", HM(), max_epoch=2, verbose=0, batch_size=20)
    p.set_multi_batches(True)       # ... switched on afterwards: accepted
    sol = scsopt.iterate(scsopt.ProxLQNSCORE(m=3), p, "l1", HM(), max_epoch=2, verbose=0, batch_size=20,
                         shuffle_batch=False)
    assert np.all(np.isfinite(sol.x))
    p.set_batches([np.arange(20)])
    p.set_multi_batches(False)      # ... and off again with a list registered: the list goes
    with pytest.raises(scsopt.ScsError):
        p.select_batch(0)
    with pytest.raises(IndexError):
        p.get_batch_data(0)
    p.ctx.close()
    # a sparse A, scs_set_sparse_outputs included: a dense A is needed
    ps = scsopt.Problem(sp.csr_matrix(A), Y, x0, f, 1e-3, out_fn=of, sparse_outputs=True, multi_batches=True)
    with pytest.raises(scsopt.ScsError, match=r"need a dense A"):
        scsopt.iterate(scsopt.ProxLQNSCORE(m=3), ps, "l1", HM(), max_epoch=2, verbose=0, batch_size=20)
    ps.ctx.close()
    # ProxGGNSCORE without multi_sample on a sample-shape batch: the sample-space refusal, naming the batch's N
    pg = scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of, multi_batches=True)
    assert N * K + 1 > d * K and 5 * K + 1 <= d * K
    with pytest.raises(scsopt.ScsError, match=r"N\*nout \+ 1 = 16 <= d\*nout = 27.*sample-space branch"):
        scsopt.iterate(scsopt.ProxGGNSCORE(), pg, "l1", HM(), max_epoch=2, verbose=0, batch_size=5, shuffle_batch=False)
    pg.ctx.close()
    with pytest.raises(ValueError, match=r"devices=\[\.\.\.\]"):
        scsopt.Problem(A, Y, x0, f, 1e-3, out_fn=of, multi_batches=True, devices=[0, 0], device_exchange="host")


# ---------------------------------------------------------------------------------------------
# 10. no drift without nout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ggn", "lqn"])
def test_no_drift_on_single_output_batches(method):
    """A single-output context with multi_batches=True (stored without effect) gives bit for bit the minibatch
    trajectory of one without it; ProxGGNSCORE's batches of 40 < m rows take its sample-space branch."""
    N, m = 150, 64
    rng = np.random.default_rng(31)
    A = rng.standard_normal((N, m)) / np.sqrt(m)
    y01 = (rng.random(N) < 0.5).astype(np.float64)
    x0 = 0.2 * rng.standard_normal(m)
    sols = []
    for mb in (False, True):
        if method == "ggn":
            p = scsopt.Problem(A, y01, x0, losses.logistic_ce(1.0 / N), 2e-3, out_fn=losses.sigmoid_ce(1.0 / N),
                               multi_batches=mb)
            meth = scsopt.ProxGGNSCORE()
        else:
            p = scsopt.Problem(A, y01, x0, losses.least_squares(1.0 / N), 2e-3, multi_batches=mb)
            meth = scsopt.ProxLQNSCORE(m=5)
        sols.append(scsopt.iterate(meth, p, "l1", HM(), max_epoch=4, verbose=0, **shuffled(N, 40)))
        p.ctx.close()
    _same_bits(sols[0], sols[1])
