"""GPU: a sparse A that is already on the device (scs_set_sparse_device / scs_set_test_sparse_device,
Problem(A = a torch.sparse_csr_tensor or any object with device indptr / indices / data, ...)).

The contract is exact: after the device door the context holds, bit for bit and entry for entry, what
the host door (scs_set_sparse) holds from the same CSR arrays and scipy's tocsc() of them -- unsorted
rows and duplicate entries included -- so everything downstream is the host door's.  Every comparison
is np.array_equal on the bits, between one context fed through each door.  The sharded case follows
tests/test_gpu_device_data.py (its launch pattern and its tolerance against the unsharded run).

Shapes: N in {1, 3, 4, 5, 1000} (four rows per workgroup and its neighbours, many workgroups), m in
{1, 300, 16385, 20000} (one LDS block of 16384 columns, one column past it, two blocks), row lengths
0, 1, 63, 64, 65 and 200 (the 64-lane window and its neighbours); a row longer than m repeats columns.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.multiprocessing as mp

import scsopt
from scsopt import _lib, losses

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")
HIST = ("obj", "fval", "pri_res_norm", "rel", "objrel", "fvaltest")
NS = (1, 3, 4, 5, 1000)
MS = (1, 300, 16385, 20000)
LENS = (0, 1, 63, 64, 65, 200)
DEV = torch.device("cuda", 0)
err = lambda ctx: _lib.lib.scs_last_error(ctx.h).decode()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- host CSR triples (int64 pointers and indices, float64 values), built once --------------------
@functools.lru_cache(maxsize=None)
def boundary_csr(N, m):
    """row r holds LENS[(r + k) % 6] entries (k moves with the shape, so the short N meet every length
    over the four m), columns in random order; a row longer than m repeats columns"""
    rng = np.random.default_rng(1000 * N + m)
    k = MS.index(m) + NS.index(N)
    lens = np.array([LENS[(r + k) % 6] for r in range(N)], dtype=np.int64)
    indptr = np.zeros(N + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    cols = [rng.choice(m, n, replace=False) if n <= m else rng.integers(0, m, n) for n in lens]
    indices = np.concatenate(cols).astype(np.int64) if N else np.zeros(0, np.int64)
    data = rng.standard_normal(indices.size)         # does not survive a round trip through fp32
    return indptr, indices, data


def _rows_to_csr(rows, m):
    """rows: a list of (columns, values) per row, in storage order"""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(c) for c, _ in rows])
    indices = np.concatenate([np.asarray(c, dtype=np.int64) for c, _ in rows]) if indptr[-1] else np.zeros(0, np.int64)
    data = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows]) if indptr[-1] else np.zeros(0)
    return indptr, indices, data


NC_N, NC_M = 200, 300


@functools.lru_cache(maxsize=None)
def noncanonical_csr(kind):
    """N = 200, m = 300.  "runs": scrambled rows, a run of three duplicates, a duplicate run at sorted
    positions 63 and 64 of a 70-entry row, an empty row and an empty column.  "dense": a dense row (m
    entries) and a dense column (an entry in every row: all claims meet on one counter), scrambled.
    "zero": the all-zero matrix."""
    N, m = NC_N, NC_M
    rng = np.random.default_rng({"runs": 1, "dense": 2, "zero": 3}[kind])
    if kind == "zero":
        return _rows_to_csr([((), ())] * N, m)
    rows = []
    for r in range(N):
        n = int(rng.integers(0, 40))
        c = rng.choice(m, n, replace=False)
        if kind == "runs":
            c = c[c != 11]                                          # column 11 stays empty
        else:
            c = np.concatenate([[0], c[c != 0]])                    # column 0 in every row
        rows.append((rng.permutation(c), None))
    if kind == "runs":
        rows[10] = (np.zeros(0, np.int64), None)                    # an empty row
        rows[3] = (np.array([40, 7, 250, 7, 12, 7, 3]), None)       # three duplicates of (3, 7)
        c = np.sort(rng.choice(np.setdiff1d(np.arange(m), [11]), 69, replace=False))
        c = np.concatenate([c[:64], c[63:]])                        # sorted positions 63 and 64 hold one column
        assert c.size == 70 and c[63] == c[64] and c[62] < c[63] < c[65]
        rows[5] = (rng.permutation(c), None)
    else:
        rows[20] = (rng.permutation(m), None)                       # a dense row
    rows = [(c, rng.standard_normal(len(c))) for c, _ in rows]
    return _rows_to_csr(rows, m)


# ---- the two doors through the C ABI, on contexts that are reused across shapes -------------------
def host_load(ctx, N, m, indptr, indices, data, y, f32):
    """scs_set_sparse from the CSR as it is and scipy's tocsc() of it (Problem._set_sparse's arrays)"""
    S = sp.csr_matrix((np.asarray(data, dtype=np.float64), indices, indptr), shape=(N, m))
    T = S.tocsc()
    a = [np.ascontiguousarray(S.indptr, dtype=np.int64), np.ascontiguousarray(S.indices, dtype=np.int32),
         np.ascontiguousarray(S.data, dtype=np.float64), np.ascontiguousarray(T.indptr, dtype=np.int64),
         np.ascontiguousarray(T.indices, dtype=np.int32), np.ascontiguousarray(T.data, dtype=np.float64)]
    i64, i32 = _lib.c_i64p, _lib.c_i32p
    ctx.check(_lib.lib.scs_set_sparse(ctx.h, N, m, int(a[2].size), a[0].ctypes.data_as(i64), a[1].ctypes.data_as(i32),
                                      _lib.dptr(a[2]), a[3].ctypes.data_as(i64), a[4].ctypes.data_as(i32),
                                      _lib.dptr(a[5]), int(f32), _lib.dptr(y), N, 0))


class _Csr:
    """any object with device indptr / indices / data and a shape will do (CuPy's csr_matrix has them);
    here it carries the int32 arrays and the mixed widths torch's own CSR tensor does not take"""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape


def device_csr(N, m, indptr, indices, data, pw=8, iw=8):
    """data keeps its dtype (the source value type); torch's CSR tensor for int64 / int64"""
    ti = {4: np.int32, 8: np.int64}
    tp = torch.from_numpy(indptr.astype(ti[pw])).to(DEV)
    tc = torch.from_numpy(indices.astype(ti[iw])).to(DEV)
    tv = torch.from_numpy(np.ascontiguousarray(data)).to(DEV)
    if pw == iw == 8:
        return torch.sparse_csr_tensor(tp, tc, tv, size=(N, m))
    return _Csr(tp, tc, tv, (N, m))


def device_call(ctx, A, y, f32, test=False, nnz=None):
    """rc of scs_set_sparse_device (the producer is synchronised: src_stream NULL)"""
    assert _lib.is_device_csr(A)
    shape, ip, ix, dv = _lib.device_csr_arrays(A)
    d = _lib.parse_device_csr(shape, *(t.__cuda_array_interface__ for t in (ip, ix, dv)))
    torch.cuda.synchronize()
    src = (d["rowptr"], d["ptr_bytes"], d["colidx"], d["idx_bytes"], d["val"], d["val_bytes"], int(f32),
           y.ctypes.data, None)
    nnz = d["nnz"] if nnz is None else nnz
    if test:
        return _lib.lib.scs_set_test_sparse_device(ctx.h, d["N"], nnz, *src, d["N"], 0)
    return _lib.lib.scs_set_sparse_device(ctx.h, d["N"], d["m"], nnz, *src, d["N"], 0)


def view(ctx, m):
    """a Problem over a loaded context: its read-back and product helpers"""
    return scsopt.Problem(np.zeros(m), losses.least_squares(1.0), 0.1, _ctx=ctx)


def stored(ctx, N, m):
    """(rowptr, colidx, val bits, colptr, rowidx, valT bits, y bits) as the context holds them"""
    p = view(ctx, m)
    R, y = p.get_sparse()
    T = p.get_sparse_csc()
    return (R.indptr.astype(np.int64), R.indices.astype(np.int64), bits(R.data), T.indptr.astype(np.int64),
            T.indices.astype(np.int64), bits(T.data), bits(y))


@pytest.fixture(scope="module")
def doors():
    h, d = _lib.Context(0), _lib.Context(0)
    yield h, d
    h.close()
    d.close()


def check_parity(doors, N, m, csr, A, f32, what):
    """csr: the host triple holding the values the device source holds (float32 values widened)"""
    h, d = doors
    y = np.random.default_rng(N * 1000 + m).standard_normal(N)
    host_load(h, N, m, *csr, y, f32)
    d.check(device_call(d, A, y, f32))
    sh, sd = stored(h, N, m), stored(d, N, m)
    names = ("rowptr", "colidx", "val", "colptr", "rowidx", "valT", "y")
    for k, a, b in zip(names, sh, sd):
        assert np.array_equal(a, b), (what, k)
    # the stored values are the source's, cast once; rows sorted by column, duplicates in storage order
    indptr, indices, data = csr
    want = data.astype(np.float32).astype(np.float64) if f32 else np.asarray(data, dtype=np.float64)
    rowid = np.repeat(np.arange(N), np.diff(indptr))
    order = np.lexsort((np.arange(indices.size), indices, rowid))      # by row, then column, then position
    assert np.array_equal(sd[1], indices[order]) and np.array_equal(sd[2], bits(want[order])), what
    ph, pd = view(h, m), view(d, m)
    rng = np.random.default_rng(N + m)
    for _ in range(2):
        x, v = rng.standard_normal(m), rng.standard_normal(N)
        assert np.array_equal(bits(pd.gemv_n(x)), bits(ph.gemv_n(x))), what
        assert np.array_equal(bits(pd.gemv_t(v)), bits(ph.gemv_t(v))), what


# ---- 1. stored arrays, both copies ---------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["store64", "store32"])
@pytest.mark.parametrize("vt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("iw", [4, 8], ids=["idx32", "idx64"])
@pytest.mark.parametrize("pw", [4, 8], ids=["ptr32", "ptr64"])
def test_bitwise_parity_with_the_host_door(doors, pw, iw, vt, f32):
    """every boundary N x every boundary m for each pointer width x index width x source type x storage"""
    for N in NS:
        for m in MS:
            indptr, indices, data = boundary_csr(N, m)
            data = data.astype(vt)
            if vt == np.float64 and data.size:
                assert not np.array_equal(data, data.astype(np.float32).astype(np.float64))
            A = device_csr(N, m, indptr, indices, data, pw, iw)
            check_parity(doors, N, m, (indptr, indices, data.astype(np.float64)), A, f32, (N, m, pw, iw, vt, f32))


def test_row_lengths_cover_the_window():
    seen = set()
    for N in NS:
        for m in MS:
            seen |= set(np.diff(boundary_csr(N, m)[0]).tolist())
    assert seen == set(LENS)


# ---- 2. non-canonical input ------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["store64", "store32"])
@pytest.mark.parametrize("kind", ["runs", "dense", "zero"])
def test_noncanonical_input(doors, kind, f32):
    N, m = NC_N, NC_M
    csr = noncanonical_csr(kind)
    S = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, m))
    if kind == "runs":
        assert not S.has_sorted_indices and S.indptr[11] == S.indptr[10] and not (S.indices == 11).any()
    if kind == "dense":
        assert np.diff(S.indptr)[20] == m and (np.bincount(S.indices, minlength=m)[0] == N)
    A = device_csr(N, m, *csr)
    if kind == "zero":   # torch hands out null pointers for the empty arrays
        assert A.values().data_ptr() == 0 and A.col_indices().data_ptr() == 0 and A.values().numel() == 0
    check_parity(doors, N, m, csr, A, f32, (kind, f32))
    if kind == "runs":   # the duplicates are kept, in storage order, in both copies
        T = view(doors[1], m).get_sparse_csc()
        col7 = slice(T.indptr[7], T.indptr[8])
        at3 = T.indices[col7] == 3
        want = csr[2][csr[0][3]:csr[0][4]][[1, 3, 5]]
        want = want.astype(np.float32).astype(np.float64) if f32 else want
        assert at3.sum() == 3 and np.array_equal(bits(T.data[col7][at3]), bits(want))
        assert T.nnz == S.nnz and np.all(np.diff(T.indices[col7]) >= 0)


# ---- 3. determinism ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["runs", "dense"])
def test_two_ingests_give_identical_csc(doors, kind):
    """the ranks the claims return depend on arrival; the stored CSC copy does not"""
    N, m = NC_N, NC_M
    csr = noncanonical_csr(kind)
    A = device_csr(N, m, *csr)
    y = np.zeros(N)
    got = []
    for ctx in doors:
        ctx.check(device_call(ctx, A, y, False))
        got.append(stored(ctx, N, m))
    for a, b in zip(*got):
        assert np.array_equal(a, b), kind


# ---- 4. the whole path through Problem -----------------------------------------------------------------
def assert_same_solution(a, b, what=""):
    assert a.epochs == b.epochs, what
    assert np.array_equal(bits(a.x), bits(b.x)), what
    for k in HIST:
        va, vb = np.asarray(getattr(a, k), dtype=np.float64), np.asarray(getattr(b, k), dtype=np.float64)
        assert va.shape == vb.shape, (what, k)
        assert np.array_equal(bits(va), bits(vb)), (what, k, va, vb)


def torch_csr(S):
    """a scipy CSR as it is (no sorting, no summing) -> torch.sparse_csr_tensor on the GPU, its arrays
    written by kernels on torch's current stream"""
    return torch.sparse_csr_tensor(torch.from_numpy(S.indptr.astype(np.int64)).to(DEV) + 0,
                                   torch.from_numpy(S.indices.astype(np.int64)).to(DEV) + 0,
                                   torch.from_numpy(S.data).to(DEV) * 1.0, size=S.shape)


def _sparse_data(N, m, rho, seed, kind):
    rng = np.random.default_rng(seed)
    S = sp.random(N, m, density=rho, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    xt = rng.uniform(-1.5, 1.5, m)
    z = S @ xt
    if kind == "ls":
        y = z + 0.1 * rng.standard_normal(N)
    else:
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-z))).astype(np.float64)
    return S, y


@pytest.mark.parametrize("f32", [False, True], ids=["store64", "store32"])
def test_lqn_box_least_squares_histories(f32):
    """the C5 form: ProxLQNSCORE + indbox + PHuberSmootherIndBox on the sparse products"""
    N, m = 2000, 500
    S, y = _sparse_data(N, m, 0.02, 5, "ls")
    x0 = 0.5 * np.random.default_rng(6).standard_normal(m)
    mk = lambda A: scsopt.Problem(A, y, x0, losses.least_squares(1.0 / N), 1e-4, C_set=[-1.0, 1.0], sparse_f32=f32)
    run = lambda p: scsopt.iterate(scsopt.ProxLQNSCORE(m=20), p, "indbox", scsopt.PHuberSmootherIndBox(-1.0, 1.0, 0.6),
                                   max_epoch=3, verbose=0)
    pd, ph = mk(torch_csr(S)), mk(S)
    assert pd.N == N and pd.nnz == ph.nnz == S.nnz
    assert_same_solution(run(pd), run(ph), f32)


@pytest.mark.parametrize("batched", [False, True], ids=["full", "batch256"])
def test_ggn_logistic_histories_on_the_sparse_gram(batched):
    N, m = 1500, 200
    S, y = _sparse_data(N, m, 0.05, 15, "logit")
    x0 = 0.3 * np.random.default_rng(16).standard_normal(m)
    f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
    kw = dict(batch_size=256, batch_perm=np.random.default_rng(3).permutation(N)) if batched else {}
    run = lambda p: scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3,
                                   verbose=0, **kw)
    pd = scsopt.Problem(torch_csr(S), y, x0, f, 2e-3, out_fn=out)
    ph = scsopt.Problem(S, y, x0, f, 2e-3, out_fn=out)
    assert_same_solution(run(pd), run(ph), batched)


def test_heldout_device_csr_from_a_side_stream():
    """Atest as a device CSR, y and ytest as device tensors, all produced on a side stream that the
    library is told about through torch's current stream"""
    N, m, Nt = 1500, 200, 90
    S, y = _sparse_data(N + Nt, m, 0.05, 25, "logit")
    Str, Ste = S[:N], S[N:]
    x0 = 0.3 * np.random.default_rng(26).standard_normal(m)
    f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        ty, tyt = torch.from_numpy(y[:N]).to(DEV) * 1.0, torch.from_numpy(y[N:]).to(DEV) * 1.0
        pd = scsopt.Problem(torch_csr(Str), ty, x0, f, 2e-3, out_fn=out, Atest=torch_csr(Ste), ytest=tyt)
    ph = scsopt.Problem(Str, y[:N], x0, f, 2e-3, out_fn=out, Atest=Ste, ytest=y[N:])
    assert np.array_equal(bits(pd.get_sparse()[1]), bits(y[:N]))
    run = lambda p: scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3,
                                   verbose=0)
    sd, sh = run(pd), run(ph)
    assert len(sd.fvaltest) == len(sd.obj) > 0
    assert_same_solution(sd, sh)
    assert pd.ftest(x0) == ph.ftest(x0)


def test_python_refusals():
    S, y = _sparse_data(8, 4, 0.5, 1, "ls")
    args = (y, np.zeros(4), losses.least_squares(1.0 / 8), 1e-3)
    A = torch_csr(S)
    with pytest.raises(ValueError, match="devices="):
        scsopt.Problem(A, *args, devices=[0, 0], device_exchange="host")
    with pytest.raises(ValueError, match=r"to_sparse_csr\(\)"):
        scsopt.Problem(A.to_sparse_coo(), *args)
    with pytest.raises(ValueError, match="CPU sparse torch tensor"):
        scsopt.Problem(A.cpu(), *args)
    with pytest.raises(ValueError, match="batched CSR"):
        scsopt.Problem(torch.stack([A.to_dense(), A.to_dense()]).to_sparse_csr(), *args)
    with pytest.raises(TypeError, match="<f2"):
        scsopt.Problem(_Csr(A.crow_indices(), A.col_indices(), A.values().to(torch.float16), (8, 4)), *args)
    with pytest.raises(ValueError, match="length"):
        scsopt.Problem(A, y, np.zeros(5), losses.least_squares(1.0 / 8), 1e-3)


# ---- 5. two ranks on one GPU, each the CSR of its own rows ---------------------------------------------
SN, SM = 1500, 140


def _shard_run(comm=None):
    S, y = _sparse_data(SN, SM, 0.05, 71, "logit")
    x0 = 0.3 * np.random.default_rng(72).standard_normal(SM)
    f, out = losses.logistic_ce(1.0 / SN), losses.sigmoid_ce(1.0 / SN)
    if comm is None:
        p = scsopt.Problem(S, y, x0, f, 2e-3, out_fn=out)
    else:
        from scsopt.shard import row_range
        r0, r1 = row_range(SN, comm.world, comm.rank)
        p = scsopt.Problem(torch_csr(S[r0:r1]), y[r0:r1], x0, f, 2e-3, out_fn=out, comm=comm, N_global=SN, row0=r0)
        assert (p.N, p.N_global, p.row0) == (r1 - r0, SN, r0)
    sol = scsopt.iterate(scsopt.ProxGGNSCORE(), p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=4, verbose=0)
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


def test_two_ranks_each_the_csr_of_its_rows(tmp_path):
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(2, str(tmp_path / "store"), out), nprocs=2, join=True)
    full = _shard_run()
    r0, r1 = out[0], out[1]
    assert r0["epochs"] == r1["epochs"] == full["epochs"]
    assert r0["obj"] == r1["obj"] and np.array_equal(r0["x"], r1["x"])            # identical bits on both ranks
    np.testing.assert_allclose(r0["obj"], full["obj"], rtol=1e-10)                # tests/test_gpu_shard.py's bound
    np.testing.assert_allclose(r0["x"], full["x"], rtol=1e-8, atol=1e-12)


# ---- 6. positions beyond 2^31 ------------------------------------------------------------------------
def test_positions_beyond_2_31():
    """N = 2^20 rows of 2049 entries (nnz = 2^31 + 2^20), m = 4096, int32 pointers cannot hold it (int64),
    int32 indices, fp32 values, fp32 storage.  Row r holds the columns (r + k) mod m, k = 0..2048, stored
    in that order (so a row that wraps is unsorted); entry (r, c) = (r mod 2039) + 2048 ((c - r) mod m)
    + 1, an integer below 2^23 that fp32 holds exactly.  About 17 GB in, about 100 GB at the peak."""
    N, m, K = 1 << 20, 4096, 2049
    nnz = N * K
    assert nnz > 2 ** 31
    r = torch.arange(N, device=DEV, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=DEV, dtype=torch.int64)[None, :]
    indices = ((r + k) % m).to(torch.int32).reshape(-1)
    data = ((r % 2039) + 2048 * k + 1).to(torch.float32).reshape(-1)
    indptr = torch.arange(N + 1, device=DEV, dtype=torch.int64) * K
    del r, k
    torch.cuda.empty_cache()
    A = _Csr(indptr, indices, data, (N, m))
    p = scsopt.Problem(A, np.zeros(N), np.zeros(m), losses.least_squares(1.0 / N), 1e-3, sparse_f32=True)
    assert p.nnz == nnz
    del A, indptr, indices, data
    torch.cuda.empty_cache()
    # the last row, stored past position 2^31: Aᵀ e_{N-1}
    e = np.zeros(N)
    e[N - 1] = 1.0
    want = np.zeros(m)
    kk = np.arange(K)
    want[(N - 1 + kk) % m] = ((N - 1) % 2039) + 2048 * kk + 1
    assert np.array_equal(p.gemv_t(e), want)
    # the last column: A e_{m-1}; row r holds it at k = (m - 1 - r) mod m when that is below K
    e = np.zeros(m)
    e[m - 1] = 1.0
    rr = np.arange(N)
    kc = (m - 1 - rr) % m
    want = np.where(kc < K, (rr % 2039) + 2048 * kc + 1, 0).astype(np.float64)
    assert np.array_equal(p.gemv_n(e), want)
    p.ctx.close()
    torch.cuda.empty_cache()


# ---- 7. refusals ---------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(doors):
    h, d = doors
    N, m = 5, 300
    indptr, indices, data = boundary_csr(N, m)
    nnz = int(indices.size)
    y = np.arange(N, dtype=np.float64)
    host_load(d, N, m, indptr, indices, data, y, False)             # something to keep
    kept = stored(d, N, m)
    tp, ti, tv = (torch.from_numpy(a).to(DEV) for a in (indptr, indices, data))
    torch.cuda.synchronize()
    ARG = _lib.SCS_ERR_ARG

    def call(ctx=d, ptr=tp, idx=ti, val=tv, pb=8, ib=8, vb=8, n=nnz, rows=N, test=False):
        p_ = lambda t: t if isinstance(t, int) else t.data_ptr()
        src = (p_(ptr), pb, p_(idx), ib, p_(val), vb, 0, y.ctypes.data, None)
        if test:
            return _lib.lib.scs_set_test_sparse_device(ctx.h, rows, n, *src, rows, 0)
        return _lib.lib.scs_set_sparse_device(ctx.h, rows, m, n, *src, rows, 0)

    def still_there():
        for a, b in zip(kept, stored(d, N, m)):
            assert np.array_equal(a, b)

    def changed(src, pos, value):
        t = src.clone()
        t[pos] = value
        torch.cuda.synchronize()
        return t

    cases = [
        (dict(pb=2), "ptr_bytes = 2"), (dict(ib=16), "idx_bytes = 16"), (dict(vb=2), "val_bytes = 2"),
        (dict(ptr=0), "d_rowptr is NULL"), (dict(idx=0), "d_colidx is NULL"), (dict(val=0), "d_val is NULL"),
        (dict(ptr=indptr.ctypes.data), "d_rowptr is not device memory"),          # a host pointer
        (dict(val=data.ctypes.data), "d_val is not device memory"),
        (dict(n=2 ** 32 - 1), "runs past the end of its allocation"),             # nnz beyond the allocation
        (dict(n=(2 ** 31 - 1) * 64 + 1), "nnz too large"),                        # above the host door's limit
        (dict(n=2 ** 32), "nnz too large"),                                       # above the sorts' 32-bit counts
        (dict(ptr=changed(tp, 0, 1)), "rowptr must start at 0 (row 0)"),
        (dict(ptr=changed(tp, N, nnz - 1)), f"rowptr must end at nnz = {nnz} (row {N - 1})"),
        (dict(ptr=changed(tp, 2, int(indptr[1]) - 1)), "rowptr not monotone at row 1"),
        (dict(idx=changed(ti, 17, -1)), "at position 17"),                        # a negative index
        (dict(idx=changed(ti, 40, m)), f"column index outside [0, {m}) at position 40"),   # an index equal to m
        (dict(idx=changed(ti, 3, 2 ** 32 + 5)), "at position 3"),                 # narrowed, it would read as 5
    ]
    assert np.diff(indptr)[1] > 0 and nnz > 40
    for kw, msg in cases:
        assert call(**kw) == ARG and msg in err(d), (kw, err(d))
        still_there()
    # two faults: the first offending row and the first offending position are the ones named
    two = changed(changed(ti, 30, -7), 9, m + 1)
    assert call(idx=two) == ARG and "at position 9" in err(d)
    # a multi-device context
    g = _lib.Context(devices=[0, 0], device_exchange="host")
    try:
        assert call(ctx=g) == ARG and "single-device context" in err(g)
        assert call(ctx=g, test=True) == ARG and "single-device context" in err(g)
    finally:
        g.close()
    # held-out rows: the same checks, and an earlier held-out set survives a refusal
    d.check(call(test=True))
    x = np.random.default_rng(1).standard_normal(m)
    ft = C.c_double()
    d.check(_lib.lib.scs_eval_ftest(d.h, _lib.dptr(x), C.byref(ft)))
    assert call(test=True, idx=changed(ti, 3, 2 ** 32 + 5)) == ARG and "at position 3" in err(d)
    assert call(test=True, pb=3) == ARG and "ptr_bytes = 3" in err(d)
    ft2 = C.c_double()
    d.check(_lib.lib.scs_eval_ftest(d.h, _lib.dptr(x), C.byref(ft2)))
    assert ft.value == ft2.value and ft.value != 0.0
    still_there()
    # and the door works after all of it
    A = device_csr(N, m, indptr, indices, data)
    check_parity(doors, N, m, (indptr, indices, data), A, True, "after the refusals")
