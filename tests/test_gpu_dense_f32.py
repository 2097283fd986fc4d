"""GPU: a dense A stored as fp32 on the device (scs_set_dense_f32 / scs_set_data_f32,
Problem(..., dense_f32=True)).

The contract is exact: an fp32-stored context produces, bit for bit, what an fp64-stored context
produces from the same values widened to fp64 -- the kernels widen on load and keep the fp64
kernels' thread-to-element mapping and operation order.  So every comparison here is
np.array_equal between a dense_f32 problem on A32 and a default problem on A32.astype(float64);
the oracle comparisons use the tolerances of tests/test_gpu_parity.py (objective history rtol 1e-8,
x rtol 1e-6 / atol 1e-9).  Shapes are the smallest that reach each code path.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import scsopt
import scsopt_oracle as O
from scsopt import losses

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")
HIST = ("obj", "fval", "pri_res_norm", "rel", "objrel", "fvaltest")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_data(N, m, kind, seed):
    """float32 rows ~ N(0,1)/sqrt(m) and y from a sparse x_true (kind 1: {0,1}, 2: ±1, 3: real)."""
    rng = np.random.default_rng(seed)
    A32 = (rng.standard_normal((N, m)) / np.sqrt(m)).astype(np.float32)
    xt = rng.standard_normal(m) * (rng.random(m) < 0.1)
    z = A32.astype(np.float64) @ xt
    u = rng.random(N)
    if kind == 1:
        y = (u < 1.0 / (1.0 + np.exp(-z))).astype(np.float64)
    elif kind == 2:
        y = np.where(u < 1.0 / (1.0 + np.exp(-z)), 1.0, -1.0)
    else:
        y = z + 0.1 * rng.standard_normal(N)
    return A32, y


def pair(A32, y, x0, f, lam, **kw):
    """(fp32-stored problem on A32, fp64-stored problem on the same values widened)"""
    p32 = scsopt.Problem(A32, y, x0, f, lam, dense_f32=True, **kw)
    p64 = scsopt.Problem(A32.astype(np.float64), y, x0, f, lam, **kw)
    assert p32.data_info()[0] == 4 and p64.data_info()[0] == 8
    return p32, p64


def assert_same_solution(a, b, what=""):
    assert a.epochs == b.epochs, what
    assert np.array_equal(bits(a.x), bits(b.x)), what
    for k in HIST:
        va, vb = np.asarray(getattr(a, k), dtype=np.float64), np.asarray(getattr(b, k), dtype=np.float64)
        assert va.shape == vb.shape, (what, k)
        assert np.array_equal(bits(va), bits(vb)), (what, k, va, vb)


# ---------------------------------------------------------------------------
# 1. products
# ---------------------------------------------------------------------------
def test_products_bitwise(monkeypatch):
    """N = 4100: not a multiple of 16, two gemv_t row chunks; m = 200: two panels, the last with 56
    padded columns."""
    N, m = 4100, 200
    Npad, mpad = 4112, 256
    A32, y = make_data(N, m, 3, 1)
    x0 = np.zeros(m)
    rng = np.random.default_rng(2)
    # ctx_bytes right after construction: the contexts differ by A alone
    p32, p64 = pair(A32, y, x0, losses.least_squares(1.0 / N), 1e-3)
    e32, a32, c32 = p32.data_info()
    e64, a64, c64 = p64.data_info()
    assert (e32, a32) == (4, Npad * mpad * 4)
    assert (e64, a64) == (8, Npad * mpad * 8)
    assert c64 - c32 == Npad * mpad * 4
    x = rng.standard_normal(m)
    v = rng.standard_normal(N)
    w = rng.random(N) + 0.1
    assert np.array_equal(bits(p32.gemv_n(x)), bits(p64.gemv_n(x)))
    for env in (None, "0"):   # the panel kernel (default) and the column-group kernel
        if env is None:
            monkeypatch.delenv("SCS_GEMV_T", raising=False)
        else:
            monkeypatch.setenv("SCS_GEMV_T", env)
        assert np.array_equal(bits(p32.gemv_t(v)), bits(p64.gemv_t(v))), env
    lo = np.tril_indices(m)
    G32, G64 = p32.gram(w), p64.gram(w)
    assert np.array_equal(bits(G32[lo]), bits(G64[lo]))
    assert "float" in p32.ctx.kernel_names()[0] and "float" not in p64.ctx.kernel_names()[0]
    assert "float" in p32.ctx.kernel_names()[1]
    # and the products are the widened matrix's to the usual summation-order bound
    A = A32.astype(np.float64)
    assert np.all(np.abs(p32.gemv_n(x) - A @ x) <= 1e-13 * (np.abs(A) @ np.abs(x)) + 1e-300)
    cols = np.array([0, 127, 128, 199])
    assert np.array_equal(bits(p32.get_columns(cols)), bits(A[:, cols]))


# ---------------------------------------------------------------------------
# 2. Gram variants
# ---------------------------------------------------------------------------
def _gram_pair(m, seed=5):
    N = 3000
    A32, y = make_data(N, m, 3, seed)
    p32, p64 = pair(A32, y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3)
    rng = np.random.default_rng(seed + 1)
    return p32, p64, rng.random(N) + 0.1, rng.standard_normal(N)


@pytest.mark.parametrize("env", [{}, {"SCS_GRAM_FUSE": "2"}, {"SCS_GRAM_SCHED": "0"}])
def test_gram_128_tiles_bitwise(env, monkeypatch):
    """m = 384, 128 x 128 tiles: the scheduled launch, the fused Aᵀv on these tiles, the plain launch."""
    monkeypatch.setenv("SCS_GRAM_TALL", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = 384
    p32, p64, w, v = _gram_pair(m)
    pairs = [(i, j) for i in range(0, m, 37) for j in range(0, m, 41)]
    g32, t32, f32 = p32.gram_atv_sample(w, v, pairs)
    g64, t64, f64 = p64.gram_atv_sample(w, v, pairs)
    assert f32 == f64 == (env.get("SCS_GRAM_FUSE") == "2")
    assert np.array_equal(bits(g32), bits(g64)) and np.array_equal(bits(t32), bits(t64))
    lo = np.tril_indices(m)
    assert np.array_equal(bits(p32.gram(w)[lo]), bits(p64.gram(w)[lo]))
    name = p32.ctx.kernel_names()[0]
    assert "<float, 2," in name, name


@pytest.mark.parametrize("sched", ["1", "0"])
def test_gram_tall_tiles_fused_atv_bitwise(sched, monkeypatch):
    """m = 256 with SCS_GRAM_TALL=1: the 256 x 128 tiles with Aᵀv fused into the Gram launch."""
    monkeypatch.setenv("SCS_GRAM_TALL", "1")
    monkeypatch.setenv("SCS_GRAM_SCHED", sched)
    m = 256
    p32, p64, w, v = _gram_pair(m, seed=9)
    pairs = [(i, j) for i in range(0, m, 29) for j in range(0, m, 31)]
    g32, t32, f32 = p32.gram_atv_sample(w, v, pairs)
    g64, t64, f64 = p64.gram_atv_sample(w, v, pairs)
    assert f32 and f64
    assert np.array_equal(bits(g32), bits(g64)) and np.array_equal(bits(t32), bits(t64))
    name = p32.ctx.kernel_names()[0]
    assert "<float, 4, true>" in name, name
    lo = np.tril_indices(m)
    assert np.array_equal(bits(p32.gram(w)[lo]), bits(p64.gram(w)[lo]))


_SIA0_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import scsopt
from scsopt import losses
N, m = 3000, 384
rng = np.random.default_rng(5)
A32 = (rng.standard_normal((N, m)) / np.sqrt(m)).astype(np.float32)
w = rng.random(N) + 0.1
y = np.zeros(N)
p32 = scsopt.Problem(A32, y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3, dense_f32=True)
p64 = scsopt.Problem(A32.astype(np.float64), y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3)
G32, G64 = p32.gram(w), p64.gram(w)
np.savez(sys.argv[2], G32=G32, G64=G64, n32=p32.ctx.kernel_names()[0], n64=p64.ctx.kernel_names()[0])
p32.ctx.close(); p64.ctx.close()
"""


def test_gram_nondefault_switch_falls_back(tmp_path):
    """SCS_GRAM_SIA=0 (read once per process: a child) selects the register-staged kernel for fp64;
    fp32-stored data falls back to the default interleaved kernel, runs and agrees bit for bit."""
    f = tmp_path / "sia0.npz"
    e = dict(os.environ, SCS_GRAM_SIA="0", SCS_GRAM_TALL="0")
    subprocess.run([sys.executable, "-c", _SIA0_CHILD, PKG, str(f)], env=e, check=True, timeout=120)
    r = np.load(f)
    assert "float" in str(r["n32"]) and "gram_f64_kernel" in str(r["n64"])
    lo = np.tril_indices(384)
    assert np.array_equal(bits(r["G32"][lo]), bits(r["G64"][lo]))


# ---------------------------------------------------------------------------
# 3. trajectories
# ---------------------------------------------------------------------------
TN, TM = 2000, 150
CASES = {
    "nscore_margin_l1": dict(kind=2, reg="l1", lam=2e-3),
    "ggn_ce_l1": dict(kind=1, reg="l1", lam=2e-3),
    "ggn_ls_gl": dict(kind=3, reg="gl", lam=[1e-8, 0.05]),
    "lqn_ls_indbox": dict(kind=3, reg="indbox", lam=1e-4),
}


def _trajectory(case, p, solver):
    c = CASES[case]
    if solver == "reference":
        p.set_solver("reference")
    if case == "nscore_margin_l1":
        meth, hm = scsopt.ProxNSCORE(), scsopt.PHuberSmootherL1L2(1.0)
    elif case == "ggn_ce_l1":
        meth, hm = scsopt.ProxGGNSCORE(), scsopt.PHuberSmootherL1L2(1.0)
    elif case == "ggn_ls_gl":
        meth, hm = scsopt.ProxGGNSCORE(), scsopt.PHuberSmootherGL(1e-2, p)
    else:
        meth, hm = scsopt.ProxLQNSCORE(m=5), scsopt.PHuberSmootherIndBox(-1.0, 1.0, 0.6)
    return scsopt.iterate(meth, p, c["reg"], hm, max_epoch=8, verbose=0)


def _oracle(case, A, y, x0):
    c = CASES[case]
    ind = np.array([[1 + 10 * g for g in range(TM // 10)], [10 + 10 * g for g in range(TM // 10)], [1] * (TM // 10)])
    if case == "nscore_margin_l1":
        om = O.Problem(A, y, x0, O.Loss("logistic_margin", 1.0 / TN), c["lam"])
        return O.iterate(O.ProxNSCORE(), om, "l1", O.PHuberSmootherL1L2(1.0), max_epoch=8)
    if case == "ggn_ce_l1":
        om = O.Problem(A, y, x0, O.Loss("logistic_ce", 1.0 / TN, ggn="sigmoid_ce"), c["lam"])
        return O.iterate(O.ProxGGNSCORE(), om, "l1", O.PHuberSmootherL1L2(1.0), max_epoch=8)
    if case == "ggn_ls_gl":
        om = O.Problem(A, y, x0, O.Loss("least_squares", 1.0 / TN, ggn="linear_ls"), c["lam"],
                       P=O.GroupP(TM, ind, np.arange(1, TM + 1)))
        return O.iterate(O.ProxGGNSCORE(), om, "gl", O.PHuberSmootherGL(1e-2, om), max_epoch=8)
    om = O.Problem(A, y, x0, O.Loss("least_squares", 1.0 / TN), c["lam"], C_set=[-1.0, 1.0])
    return O.iterate(O.ProxLQNSCORE(m=5), om, "indbox", O.PHuberSmootherIndBox(-1.0, 1.0, 0.6), max_epoch=8)


def _problem_pair(case):
    c = CASES[case]
    A32, y = make_data(TN, TM, c["kind"], 11)
    x0 = 0.3 * np.random.default_rng(12).standard_normal(TM)
    kw = {}
    if case == "nscore_margin_l1":
        f = losses.logistic_margin(1.0 / TN)
    elif case == "ggn_ce_l1":
        f, kw["out_fn"] = losses.logistic_ce(1.0 / TN), losses.sigmoid_ce(1.0 / TN)
    elif case == "ggn_ls_gl":
        f, kw["out_fn"] = losses.least_squares(1.0 / TN), losses.linear_ls(1.0 / TN)
    else:
        f, kw["C_set"] = losses.least_squares(1.0 / TN), [-1.0, 1.0]
    p32, p64 = pair(A32, y, x0, f, c["lam"], **kw)
    if case == "ggn_ls_gl":
        ind = np.array([[1 + 10 * g for g in range(TM // 10)], [10 + 10 * g for g in range(TM // 10)],
                        [1] * (TM // 10)])
        for p in (p32, p64):
            p.P = scsopt.get_P(TM, np.arange(1, TM + 1), ind)
    return p32, p64, A32.astype(np.float64), y, x0


@pytest.mark.parametrize("case,solver", [("nscore_margin_l1", "default"), ("ggn_ce_l1", "default"),
                                         ("ggn_ls_gl", "default"), ("lqn_ls_indbox", "default"),
                                         ("nscore_margin_l1", "reference"), ("ggn_ce_l1", "reference")])
def test_trajectory_bitwise_and_on_the_oracle(case, solver):
    p32, p64, A, y, x0 = _problem_pair(case)
    s32 = _trajectory(case, p32, solver)
    s64 = _trajectory(case, p64, solver)
    assert_same_solution(s32, s64, (case, solver))
    osol = _oracle(case, A, y, x0)
    assert s32.epochs == osol.epochs and len(s32.obj) == len(osol.obj)
    np.testing.assert_allclose(s32.obj, osol.obj, rtol=1e-8, atol=0)
    np.testing.assert_allclose(s32.x, osol.x, rtol=1e-6, atol=1e-9)


# ---------------------------------------------------------------------------
# 4. GGN sample-space branch, 5. minibatches
# ---------------------------------------------------------------------------
def test_ggn_sample_space_bitwise():
    """N + 1 <= m: the Aᵀ copy (fp64, widened from the fp32 rows) and the (N+1) x (N+1) system."""
    N, m = 100, 300
    A32, y = make_data(N, m, 1, 21)
    x0 = 0.3 * np.random.default_rng(22).standard_normal(m)
    p32, p64 = pair(A32, y, x0, losses.logistic_ce(1.0 / N), 1e-3, out_fn=losses.sigmoid_ce(1.0 / N))
    run = lambda p: scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=4,
                                   verbose=0)
    assert_same_solution(run(p32), run(p64))


def test_minibatches_bitwise():
    """batch_size = 256 over N = 1000 (a partial last batch): the gathered batch views are fp32."""
    N, m = 1000, 130
    A32, y = make_data(N, m, 1, 31)
    x0 = 0.3 * np.random.default_rng(32).standard_normal(m)
    p32, p64 = pair(A32, y, x0, losses.logistic_ce(1.0 / N), 2e-3, out_fn=losses.sigmoid_ce(1.0 / N))
    perm = np.random.default_rng(3).permutation(N)
    run = lambda p: scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3,
                                   verbose=0, batch_size=256, batch_perm=perm)
    assert_same_solution(run(p32), run(p64))
    # the pooled batch views (256 rows; 232 rows padded to 240) hold float rows in the fp32 context
    grown = []
    for p in (p32, p64):
        before = p.data_info()[2]
        p.set_batches([perm[:256], perm[768:]])
        p.select_batch(0)
        p.select_batch(1)
        grown.append(p.data_info()[2] - before)
        p.set_batches(None)
    assert grown[1] - grown[0] == (256 + 240) * 256 * 4


# ---------------------------------------------------------------------------
# 6. rounding, 7. generator
# ---------------------------------------------------------------------------
def test_rounding_to_nearest_even_and_roundtrip():
    N, m = 37, 20
    rng = np.random.default_rng(41)
    A = rng.standard_normal((N, m))
    A[0, :6] = [1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -0.0, -(1.0 + 2.0 ** -24), 0.1, 3.0e38]
    y = rng.standard_normal(N)
    p = scsopt.Problem(A, y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3, dense_f32=True)
    assert p.data_info()[0] == 4
    got, gy = p.get_data()
    want = A.astype(np.float32).astype(np.float64)
    assert want[0, 0] == 1.0 and want[0, 1] == 1.0 + 2.0 ** -22   # the ties went to even
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(gy, y)
    # float32 input is stored as it is
    A32 = want.astype(np.float32)
    q = scsopt.Problem(A32, y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3, dense_f32=True)
    assert np.array_equal(bits(q.get_data()[0]), bits(A32.astype(np.float64)))
    # and without dense_f32 a float32 matrix is widened and stored fp64, as before
    d = scsopt.Problem(A32, y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3)
    assert d.data_info()[:2] == (8, 48 * 128 * 8)


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_generator_rounds_rows_and_labels_from_stored_rows(kind):
    N, m = 600, 140
    x0 = 0.3 * np.random.default_rng(51).standard_normal(m)
    f, out, meth = {1: (losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N), scsopt.ProxGGNSCORE),
                    2: (losses.logistic_margin(1.0 / N), None, scsopt.ProxNSCORE),
                    3: (losses.least_squares(1.0 / N), None, scsopt.ProxLQNSCORE)}[kind]
    p32 = scsopt.Problem.synthetic(N, m, x0, f, 2e-3, kind=kind, seed=77, out_fn=out, dense_f32=True)
    p64 = scsopt.Problem.synthetic(N, m, x0, f, 2e-3, kind=kind, seed=77, out_fn=out)
    assert p32.data_info()[0] == 4 and p64.data_info()[0] == 8
    A32, y32 = p32.get_data()
    A64, _ = p64.get_data()
    assert np.array_equal(bits(A32), bits(A64.astype(np.float32).astype(np.float64)))
    # an fp64 context loaded with the stored rows and labels runs the same trajectory
    q64 = scsopt.Problem(A32, y32, x0, f, 2e-3, out_fn=out)
    run = lambda p: scsopt.iterate(meth(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3, verbose=0)
    assert_same_solution(run(p32), run(q64), kind)


# ---------------------------------------------------------------------------
# 8. held-out data
# ---------------------------------------------------------------------------
def test_heldout_rows_bitwise():
    N, m, Nt = 500, 130, 75
    A32, y = make_data(N, m, 1, 61)
    At32, yt = make_data(Nt, m, 1, 62)
    x0 = 0.3 * np.random.default_rng(63).standard_normal(m)
    f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
    p32 = scsopt.Problem(A32, y, x0, f, 2e-3, out_fn=out, dense_f32=True, Atest=At32, ytest=yt)
    p64 = scsopt.Problem(A32.astype(np.float64), y, x0, f, 2e-3, out_fn=out, Atest=At32.astype(np.float64), ytest=yt)
    run = lambda p: scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3,
                                   verbose=0)
    c32, c64 = p32.data_info()[2], p64.data_info()[2]
    assert c64 - c32 == (512 + 80) * 256 * 4          # the held-out block is fp32 as well
    s32, s64 = run(p32), run(p64)
    assert len(s32.fvaltest) == len(s32.obj) > 0
    assert_same_solution(s32, s64)
    assert p32.ftest(x0) == p64.ftest(x0)


def test_generated_heldout_rows_bitwise():
    N, m, Nt = 500, 130, 75
    x0 = 0.3 * np.random.default_rng(64).standard_normal(m)
    f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
    p32 = scsopt.Problem.synthetic(N, m, x0, f, 2e-3, kind=1, seed=5, out_fn=out, dense_f32=True, test_N=Nt)
    A32, y32 = p32.get_data()
    # the held-out rows of the fp32 context are the generator's rows [N, N + Nt), rounded, with their labels
    g = scsopt.Problem.synthetic(N + Nt, m, x0, f, 2e-3, kind=1, seed=5, out_fn=out, dense_f32=True)
    Ag, yg = g.get_data()
    assert np.array_equal(bits(Ag[:N]), bits(A32)) and np.array_equal(yg[:N], y32)
    q64 = scsopt.Problem(A32, y32, x0, f, 2e-3, out_fn=out, Atest=Ag[N:], ytest=yg[N:])
    run = lambda p: scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3,
                                   verbose=0)
    s32, s64 = run(p32), run(q64)
    assert len(s32.fvaltest) == len(s32.obj) > 0
    assert_same_solution(s32, s64)


# ---------------------------------------------------------------------------
# 9. sharding
# ---------------------------------------------------------------------------
SN, SM = 1500, 140


def _shard_run(comm=None, devices=None, f32=False):
    A32, y = make_data(SN, SM, 1, 71)
    x0 = 0.3 * np.random.default_rng(72).standard_normal(SM)
    f, out = losses.logistic_ce(1.0 / SN), losses.sigmoid_ce(1.0 / SN)
    A = A32 if f32 else A32.astype(np.float64)
    kw = {}
    if comm is not None:
        from scsopt.shard import row_range
        r0, r1 = row_range(SN, comm.world, comm.rank)
        A, y = A[r0:r1], y[r0:r1]
        kw = dict(comm=comm, N_global=SN, row0=r0)
    if devices is not None:
        kw = dict(devices=devices, device_exchange="host")
    p = scsopt.Problem(A, y, x0, f, 2e-3, out_fn=out, dense_f32=f32, **kw)
    assert p.data_info()[0] == (4 if f32 else 8)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3, verbose=0)
    res = {k: np.asarray(getattr(sol, k), dtype=np.float64) for k in HIST}
    res["x"], res["epochs"] = sol.x.copy(), sol.epochs
    p.ctx.close()
    return res


def _shard_worker(rank, world, store_path, out):
    sys.path.insert(0, PKG)
    import torch
    import torch.distributed as dist
    from scsopt import shard
    dist.init_process_group("gloo", store=dist.FileStore(store_path, world), rank=rank, world_size=world)
    res = {}
    for f32 in (True, False):
        comm = shard.Comm(device=torch.device("cuda", 0))
        res[f32] = _shard_run(comm=comm, f32=f32)
    out[rank] = res
    dist.destroy_process_group()


def _assert_same_result(a, b, what):
    assert a["epochs"] == b["epochs"], what
    for k in HIST + ("x",):
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def test_two_ranks_bitwise(tmp_path):
    """Two processes on one GPU, each with its row block: fp32 against fp64 under the same split."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(2, str(tmp_path / "store"), out), nprocs=2, join=True)
    for r in (0, 1):
        _assert_same_result(out[r][True], out[r][False], r)
    _assert_same_result(out[0][True], out[1][True], "ranks")


def test_two_subcontexts_host_exchange_bitwise():
    """One process, a group of two sub-contexts on the one GPU (host-staged exchange): scs_set_data_f32
    forwarded to each sub-context's row block."""
    a = _shard_run(devices=[0, 0], f32=True)
    b = _shard_run(devices=[0, 0], f32=False)
    _assert_same_result(a, b, "group")


# ---------------------------------------------------------------------------
# 10. refusal
# ---------------------------------------------------------------------------
def test_quadratic_loss_is_refused():
    m = 8
    rng = np.random.default_rng(81)
    A = rng.standard_normal((m, m))
    with pytest.raises(scsopt.ScsError, match="quadratic loss needs an fp64-stored A"):
        scsopt.Problem(A, rng.standard_normal(m), np.zeros(m), losses.quadratic(), 1e-4, dense_f32=True)
    # the default storage still takes it
    p = scsopt.Problem(A, rng.standard_normal(m), np.zeros(m), losses.quadratic(), 1e-4)
    assert np.isfinite(p.fx(np.ones(m)))
