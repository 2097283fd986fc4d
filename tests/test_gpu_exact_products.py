"""GPU: the dense and sparse Gram Aᵀ diag(w) A, A·x, Aᵀ·v and the fused Aᵀv on integer data, against
int64 NumPy with np.array_equal -- no tolerance (tests/exact_data.py has the argument and the
precondition; tests/test_exact_products_host.py checks both on the CPU, and the census of the
pipeline shapes nk = 0, 1, 2, 3, >= 4 that this grid reaches per item kind).

One body judges every kernel variant against the truth: the interleaved 128 x 128 and 256 x 128
kernels with and without the tail-balanced schedule (whole-K items / K pieces + gram_combine_kernel),
pair tiles, the fp32-A twin, the fused Aᵀv and gram_vfinal_kernel, the previous kernels and the other
barrier-edge order (child processes: those switches are read once), the sparse Gram variants, the
mirror and the streaming ring, both Aᵀv kernels with the 4-way and the remainder loop of the
finalize, and the zeroed trailing split of A·x.  The same data gives the solvers a system the host
knows exactly (M = AᵀWA + diag(d) in int64) at the block edges m = 1 .. 385.

An inexact entry here is a wrong or missing term, never rounding: the failure message names the
128-blocks it lies in."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as E
import scsopt
from scsopt import losses

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(TESTS), "selfconcordantsmoothoptimization.jl_amd")

SIA128 = "gram_sia_kernel<1, 2, false, {}, false>"
SIA256 = "gram_sia_kernel<10, 4, false, {}, false>"
TA = "gram_sia_ta_kernel<float, {}, {}>"


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("SCS_"):
            monkeypatch.delenv(k)


def _problem(A, f32=False, **kw):
    N, m = A.shape
    if f32:
        A = A.astype(np.float32)
    return scsopt.Problem(A, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0, dense_f32=f32, **kw)


def _diff(got, ref):
    """'' if got == ref exactly, else where it differs: count, the 128-blocks, the first entries."""
    if got.shape == ref.shape and np.array_equal(got, ref):
        return ""
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    bad = np.argwhere(got != ref)
    blocks = sorted({tuple(int(v) // 128 for v in ix) for ix in bad})
    first = [(tuple(int(v) for v in ix), float(got[tuple(ix)]), int(ref[tuple(ix)])) for ix in bad[:4]]
    return f"{len(bad)} of {ref.size} entries differ, 128-blocks {blocks[:12]}, first (index, got, want) {first}"


def _gram_name(tall, f32, av):
    b = "true" if av else "false"
    if f32:
        return TA.format(4 if tall else 2, b)
    return (SIA256 if tall else SIA128).format(b)


# ---------------------------------------------------------------------------
# the dense Gram
# ---------------------------------------------------------------------------
_GRAM_CASES = [(tall, m, sched) for tall in (False, True) for m in E.GRAM_M[tall] for sched in (True, False)]


@pytest.mark.parametrize("tall,m,sched", _GRAM_CASES)
def test_dense_gram_exact(tall, m, sched, monkeypatch):
    """All m x m entries of G for N = 1 .. 4144 on an fp64- and an fp32-stored A; then w = 0 on the same
    context, which has just produced a non-zero G: exactly zero, nothing stale (partial slots, the
    combine, GRAM_ACCUMULATE) is left."""
    if tall:
        monkeypatch.setenv("SCS_GRAM_TALL", "1")
    if not sched:
        monkeypatch.setenv("SCS_GRAM_SCHED", "0")
    fails = []
    for N in E.GRAM_N:
        c = E.exact_case(N, m, E.case_seed(N, m))
        for f32 in (False, True):
            p = _problem(c.A, f32)
            d = _diff(p.gram(c.w), c.G)
            name = p.ctx.kernel_names()[0]
            if name != _gram_name(tall, f32, False):
                fails.append(f"N={N} f32={f32}: kernel {name}")
            if d:
                fails.append(f"N={N} f32={f32}: {d}")
            if N > 1 and not c.G.any():
                fails.append(f"N={N}: the reference G is zero")
            z = _diff(p.gram(np.zeros(N)), np.zeros((m, m), dtype=np.int64))
            if z:
                fails.append(f"N={N} f32={f32} after w = 0: {z}")
            p.ctx.close()
    assert not fails, "\n".join(fails)


def _sample_pairs(m, rng):
    """test_gpu_gram_diagpair's positions (paired D1 blocks, D0, L, off-diagonal tiles) where m holds
    them, the corners, the padded block's edge, and 32 random ones."""
    fixed = [(255, 128), (m - 1, m - 128), (200, 130), (m - 3, m - 100),
             (5, 3), (127, 0), (m - 129, m - 256), (300, 257),
             (200, 100), (m - 1, m - 200), (255, 0),
             (m - 1, 0), (300, 17), (m - 130, 140), (511, 129),
             (0, 0), (m - 1, m - 1), (m - 1, (m - 1) // 128 * 128), (m // 2, m // 2)]
    fixed = [(i, j) for i, j in fixed if 0 <= i < m and 0 <= j < m]
    return np.concatenate([np.array(fixed), rng.integers(0, m, size=(32, 2))])


@pytest.mark.parametrize("tall,m,sched", _GRAM_CASES)
def test_fused_atv_exact(tall, m, sched, monkeypatch):
    """gram_atv_sample: the production launch with the fused Aᵀv (256 x 128: the default; 128 x 128:
    SCS_GRAM_FUSE=2).  Aᵀv exact in all m entries -- K pieces write rows of the partial buffer that
    gram_vfinal_kernel sums, empty pieces included -- and the sampled G entries exact."""
    if tall:
        monkeypatch.setenv("SCS_GRAM_TALL", "1")
    else:
        monkeypatch.setenv("SCS_GRAM_FUSE", "2")
    if not sched:
        monkeypatch.setenv("SCS_GRAM_SCHED", "0")
    fails = []
    for N in E.FUSED_N:
        c = E.exact_case(N, m, E.case_seed(N, m))
        pairs = _sample_pairs(m, np.random.default_rng(N + m))
        want = c.G[pairs[:, 0], pairs[:, 1]]
        for f32 in (False, True):
            p = _problem(c.A, f32)
            g, atv, fused = p.gram_atv_sample(c.w, c.v, pairs)
            name = p.ctx.kernel_names()[0]
            p.ctx.close()
            if not fused or name != _gram_name(tall, f32, True):
                fails.append(f"N={N} f32={f32}: fused={fused} kernel {name}")
            d = _diff(atv, c.Atv)
            if d:
                fails.append(f"N={N} f32={f32} Aᵀv: {d}")
            if not np.array_equal(g, want):
                bad = np.nonzero(g != want)[0]
                fails.append(f"N={N} f32={f32} G samples: {[(tuple(pairs[k]), g[k], want[k]) for k in bad[:4]]}")
    assert not fails, "\n".join(fails)


# argv: package dir, input .npz (A_k, w_k per shape), output .npz.  Each shape with the schedule on and off.
_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import scsopt
from scsopt import losses
inp = np.load(sys.argv[2])
out = {}
for k in range(len(inp.files) // 2):
    A, w = inp[f"A_{k}"], inp[f"w_{k}"]
    for sched in ("1", "0"):
        os.environ["SCS_GRAM_SCHED"] = sched
        p = scsopt.Problem(A, np.zeros(A.shape[0]), np.zeros(A.shape[1]), losses.least_squares(), 1.0)
        out[f"G_{k}_{sched}"] = p.gram(w)
        out[f"name_{k}_{sched}"] = p.ctx.kernel_names()[0]
        p.ctx.close()
np.savez(sys.argv[3], **out)
"""

_SWITCHES = {
    "nopair": ({"SCS_GRAM_DIAGPAIR": "0"}, SIA256.format("false"), SIA128.format("false")),
    "previous": ({"SCS_GRAM_SIA": "0", "SCS_GRAM_GLDS": "2"}, "gram_glds_kernel<true, 1>",
                 "gram_f64_kernel<false, 2, true, false>"),
    "edge12": ({"SCS_GRAM_SIA": "12"}, "gram_sia_kernel<12, 4, false, false, false>", SIA128.format("false")),
}


@pytest.mark.parametrize("arm", sorted(_SWITCHES))
def test_per_process_switches_exact(arm, tmp_path):
    """The switches read once per process, one child process each: the unpaired [U; D1] list, the
    previous kernels (LDS-DMA 256 x 128, register-staged 128 x 128) and the other barrier-edge order,
    at (m, N) = (768, 40), (512, 700), (384, 300), schedule on and off, and (512, 1000), whose last
    K piece is not empty (in the first three the combine's last slot holds zeros).  The child returns
    G; the parent compares it with int64."""
    extra, name_tall, name_128 = _SWITCHES[arm]
    cases = [E.exact_case(N, m, E.case_seed(N, m)) for m, N in E.CHILD_SHAPES]
    fin, fout = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(fin, **{f"A_{k}": c.A for k, c in enumerate(cases)}, **{f"w_{k}": c.w for k, c in enumerate(cases)})
    env = {k: v for k, v in os.environ.items() if not k.startswith("SCS_")}
    env.update(extra, SCS_GRAM_TALL="1")                  # m = 384 has 3 blocks: 128 x 128 tiles all the same
    subprocess.run([sys.executable, "-c", _CHILD, PKG, str(fin), str(fout)], env=env, check=True, timeout=300)
    got = np.load(fout)
    fails = []
    for k, c in enumerate(cases):
        for sched in ("1", "0"):
            want_name = name_128 if c.m // 128 % 2 else name_tall
            if str(got[f"name_{k}_{sched}"]) != want_name:
                fails.append(f"m={c.m} N={c.N} sched={sched}: kernel {got[f'name_{k}_{sched}']}")
            d = _diff(got[f"G_{k}_{sched}"], c.G)
            if d:
                fails.append(f"m={c.m} N={c.N} sched={sched}: {d}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# the sparse Gram and products
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse_cases():
    return {(N, m): E.sparse_case(N, m, E.case_seed(N, m)) for N, m in E.SPARSE_SHAPES}


@pytest.mark.parametrize("N,m", E.SPARSE_SHAPES)
def test_sparse_gram_paths_exact(N, m, sparse_cases, monkeypatch):
    """A user CSR (unsorted, duplicates, empty rows / columns, a row dense in every column block;
    m = 4200 crosses a 4096-column block): the Gram priced by nnz in four kernel variants, the dense
    tiles on the mirror, and the streaming ring at 16, 48 and 256 rows per chunk (44 / 15 / 3 launches
    at N = 700, all but the first accumulating: GRAM_ACCUMULATE through the K pieces' combine; a
    256-row chunk is 16 stages, so every one of the 16 pieces, the last included, carries a term)."""
    s = sparse_cases[(N, m)]
    fails = []

    def check(tag, p, prefix):
        d = _diff(p.gram(s.w), s.G)
        name = p.ctx.kernel_names()[0]
        if d:
            fails.append(f"{tag}: {d}")
        if not name.startswith(prefix):
            fails.append(f"{tag}: kernel {name}")

    p = scsopt.Problem(s.coo, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0)
    monkeypatch.setenv("SCS_SPARSE_GRAM", "1")
    for var, name in (("8", "sparse_gram_seg_kernel<double, 0>"), ("6", "sparse_gram_flat_kernel<double>"),
                      ("5", "sparse_gram_pipe_kernel<double, 64, true>"), ("1", "sparse_gram_kernel<double>")):
        monkeypatch.setenv("SCS_SPARSE_GRAM_KERNEL", var)
        check(f"sparse kernel {var}", p, name)
    monkeypatch.delenv("SCS_SPARSE_GRAM_KERNEL")
    monkeypatch.setenv("SCS_SPARSE_GRAM", "0")
    check("mirror", p, "gram_sia_kernel<")
    p.ctx.close()
    monkeypatch.setenv("SCS_SPARSE_MIRROR_MAX_GB", "0")
    for rows in E.RING_ROWS:
        monkeypatch.setenv("SCS_SPARSE_CHUNK_ROWS", str(rows))
        p = scsopt.Problem(s.coo, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0)
        check(f"ring of {rows} rows", p, "gram_sia_kernel<")
        check(f"ring of {rows} rows, second call", p, "gram_sia_kernel<")
        p.ctx.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("N,m", E.SPARSE_SHAPES)
def test_sparse_products_exact(N, m, f32, sparse_cases):
    s = sparse_cases[(N, m)]
    p = scsopt.Problem(s.coo, np.zeros(N), np.zeros(m), losses.least_squares(), 1.0, sparse_f32=f32)
    assert not _diff(p.gemv_n(s.x), s.Ax)
    assert not _diff(p.gemv_t(s.v), s.Atv)
    assert not s.Ax[list(s.empty_rows)].any() and not s.Atv[list(s.empty_cols)].any()


# ---------------------------------------------------------------------------
# the streaming products of a dense A
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.GEMV_T_N)
def test_gemv_t_exact(N, monkeypatch):
    """Aᵀ v over 1, 1, 2, 4 and 5 chunks of 4096 rows (the finalize's remainder loop alone, its 4-way
    loop alone, and both; a short last chunk), m = 1, 127, 129, 640 (the odd-m pair store), the panel
    kernel and the column-group kernel (SCS_GEMV_T=0), fp64 and fp32 storage."""
    fails = []
    for m in E.GEMV_M:
        c = E.exact_case(N, m, E.case_seed(N, m))
        for f32 in (False, True):
            p = _problem(c.A, f32)
            for sw in (None, "0"):
                if sw is None:
                    monkeypatch.delenv("SCS_GEMV_T", raising=False)
                else:
                    monkeypatch.setenv("SCS_GEMV_T", sw)
                d = _diff(p.gemv_t(c.v), c.Atv)
                if d:
                    fails.append(f"m={m} f32={f32} SCS_GEMV_T={sw}: {d}")
            p.ctx.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N", E.GEMV_N_N)
def test_gemv_n_exact(N):
    """A x at the edges of the 512-row blocks and of the two-sample threads, 1 to 5 column panels
    (up to 5 column splits), fp64 and fp32 storage."""
    fails = []
    for m in E.GEMV_M:
        c = E.exact_case(N, m, E.case_seed(N, m))
        for f32 in (False, True):
            p = _problem(c.A, f32)
            d = _diff(p.gemv_n(c.x), c.Ax)
            if d:
                fails.append(f"m={m} f32={f32}: {d}")
            p.ctx.close()
    assert not fails, "\n".join(fails)


def test_streaming_products_large_exact():
    """N = 261 700, m = 520: 512 row blocks, so gemv_n_splits asks for 4 column splits of the 5 panels;
    launch_gemv_n runs 3 (2 panels each) and zeroes the fourth slice, which the epilogue sums.  Aᵀv
    on the same data runs 64 chunks (16 trips of the finalize's 4-way loop).  A is built as int16 and
    stored as fp32 (half the upload); the references are int64, by row blocks."""
    N, m = E.BIG
    rng = np.random.default_rng(E.case_seed(N, m))
    A16 = rng.integers(-8191, 8192, size=(N, m), dtype=np.int16)
    A16[::7, ::3] = 0
    x = rng.integers(-1000, 1001, size=m, dtype=np.int64)
    v = rng.integers(-1000, 1001, size=N, dtype=np.int64)
    Ax = np.empty(N, dtype=np.int64)
    Atv = np.zeros(m, dtype=np.int64)
    for r in range(0, N, 32768):
        blk = A16[r:r + 32768].astype(np.int64)
        Ax[r:r + 32768] = blk @ x
        Atv += blk.T @ v[r:r + 32768]
    p = scsopt.Problem(A16.astype(np.float32), np.zeros(N), np.zeros(m), losses.least_squares(), 1.0, dense_f32=True)
    del A16
    z = p.gemv_n(x.astype(np.float64))
    assert p.ctx.kernel_names()[1] == "gemv_n_kernel<float>"
    assert not _diff(z, Ax)
    assert not _diff(p.gemv_t(v.astype(np.float64)), Atv)
    p.ctx.close()


@pytest.mark.parametrize("N", E.COLUMNS_N)
def test_get_columns_exact(N):
    """The first and last column of every panel come back as the integers that went in."""
    for m in E.GEMV_M:
        c = E.exact_case(N, m, E.case_seed(N, m))
        cols = np.array(sorted({j for j in list(range(0, m, 128)) + list(range(127, m, 128)) + [m - 1]}))
        for f32 in (False, True):
            p = _problem(c.A, f32)
            got = p.get_columns(cols)
            p.ctx.close()
            assert got.shape == (N, cols.size)
            assert np.array_equal(got, c.A[:, cols]), (m, f32)


# ---------------------------------------------------------------------------
# the solvers on an exactly known system
# ---------------------------------------------------------------------------
def _residual_ratio(M, x, rhs, normM):
    """‖M x − rhs‖₂ / (‖M‖₂ ‖x‖₂), the residual evaluated in longdouble (M and rhs are integers)."""
    r = M.astype(np.longdouble) @ x.astype(np.longdouble) - rhs.astype(np.longdouble)
    return float(np.sqrt(np.sum(r * r))) / (normM * float(np.linalg.norm(x)))


@pytest.mark.parametrize("m", E.SOLVE_M)
def test_solvers_on_exact_system(m):
    """solve_eval builds M = AᵀWA + diag(d) on the device from integer A, w, d: the host forms the same
    M in int64.  Cholesky (mode 0, no fallback on this SPD system), LU (1) and Householder QR (2) at
    the block edges, residual <= 1e-12 ‖M‖₂ ‖x‖₂ (the bar test_householder_qr_solve holds the QR to).
    Then an indefinite M (w of mixed sign; a negative eigenvalue, checked here): mode 0 must fall back
    to the LU and meet the bar, and an SPD solve on the same context afterwards must meet it with no
    fallback -- the failed factor leaves nothing behind."""
    s = E.solve_case(m, E.case_seed(m + 77, m))
    Mf = s.M.astype(np.float64)
    assert np.array_equal(Mf.astype(np.int64), s.M)
    ev = np.linalg.eigvalsh(Mf)
    assert ev[0] > 0
    normM = float(ev[-1])
    p = _problem(s.A)
    for mode in (0, 1, 2):
        x, used_lu = p.solve_eval(s.w, s.d, s.rhs, mode)
        ratio = _residual_ratio(s.M, x, s.rhs, normM)
        print(f"m={m} mode={mode} used_lu={used_lu} residual / (|M| |x|) = {ratio:.2e}")
        assert np.all(np.isfinite(x))
        if mode == 0:
            assert not used_lu
        assert ratio <= 1e-12, (mode, ratio)
    p.ctx.close()

    t = E.solve_case(m, E.case_seed(m + 77, m), indefinite=True)
    Tf = t.M.astype(np.float64)
    evt = np.linalg.eigvalsh(Tf)
    assert evt[0] < 0
    normT = float(np.max(np.abs(evt)))
    p = _problem(t.A)
    x, used_lu = p.solve_eval(t.w, t.d, t.rhs, 0)
    ratio = _residual_ratio(t.M, x, t.rhs, normT)
    print(f"m={m} indefinite used_lu={used_lu} residual / (|M| |x|) = {ratio:.2e}")
    assert used_lu and np.all(np.isfinite(x))
    assert ratio <= 1e-12, ratio
    x, used_lu = p.solve_eval(s.w, s.d, s.rhs, 0)
    ratio = _residual_ratio(s.M, x, s.rhs, normM)
    print(f"m={m} SPD after the fallback used_lu={used_lu} residual / (|M| |x|) = {ratio:.2e}")
    assert not used_lu and np.all(np.isfinite(x))
    assert ratio <= 1e-12, ratio
    p.ctx.close()
