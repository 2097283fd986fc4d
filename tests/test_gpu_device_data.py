"""GPU: a dense A that is already on the device (scs_set_data_device / scs_set_test_data_device,
Problem(A = a torch-ROCm tensor, ...)).

The contract is exact: the device door stores, bit for bit, what the host door (scs_set_data /
scs_set_data_f32) stores from the same values, so everything downstream is the host door's.  Every
comparison is np.array_equal on the bits, between one context fed through each door.  The sharded case
follows tests/test_gpu_shard.py (its launch pattern and its tolerance against the unsharded run).

Shapes: N in {1, 15, 16, 17, 33, 1000} (one stage and its neighbours, three stages, many) and m in
{1, 127, 128, 129, 300} (one panel and its neighbours, three panels), the smallest that reach every
boundary of the 16-sample x 128-feature block; the two large shapes are there for the 64-bit offsets.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import scsopt
from scsopt import _lib, losses

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "selfconcordantsmoothoptimization.jl_amd")
HIST = ("obj", "fval", "pri_res_norm", "rel", "objrel", "fvaltest")
NS = (1, 15, 16, 17, 33, 1000)
MS = (1, 127, 128, 129, 300)
# (source type, fp32 storage)
PAIRS = {"f64_to_f64": (np.float64, False), "f64_to_f32": (np.float64, True),
         "f32_to_f64": (np.float32, False), "f32_to_f32": (np.float32, True)}
DEV = torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def values(N, m, dtype, seed):
    """values that do not survive a round trip through fp32 when dtype is float64"""
    return np.random.default_rng(seed).standard_normal((N, m)).astype(dtype)


# ---- the two doors through the C ABI, on contexts that are reused across shapes --------------------
def host_load(ctx, A, y, store32):
    """Problem's host rule: float32 rows as they are with fp32 storage, anything else as float64"""
    N, m = A.shape
    ctx.check(_lib.lib.scs_set_dense_f32(ctx.h, int(store32)))
    if A.dtype == np.float32 and store32:
        Af = np.asfortranarray(A)
        ctx.check(_lib.lib.scs_set_data_f32(ctx.h, N, m, Af.ctypes.data_as(C.c_void_p), N, _lib.dptr(y), N, 0))
    else:
        Af = np.asfortranarray(A.astype(np.float64))
        ctx.check(_lib.lib.scs_set_data(ctx.h, N, m, Af.ctypes.data_as(_lib.c_dp), N, _lib.dptr(y), N, 0))


def device_call(ctx, T, y, store32):
    """rc of scs_set_data_device for the tensor view T (the producer is synchronised: src_stream NULL)"""
    d = _lib.parse_device_matrix(T.__cuda_array_interface__)
    torch.cuda.synchronize()
    ctx.check(_lib.lib.scs_set_dense_f32(ctx.h, int(store32)))
    yp = y.data_ptr() if isinstance(y, torch.Tensor) else y.ctypes.data
    return _lib.lib.scs_set_data_device(ctx.h, d["N"], d["m"], d["ptr"], d["elem_bytes"], d["stride_n"],
                                        d["stride_m"], yp, None, d["N"], 0), d


def stored(ctx, N, m):
    A = np.zeros((m, N))
    y = np.zeros(N)
    ctx.check(_lib.lib.scs_get_data(ctx.h, 0, N, _lib.dptr(A), N, _lib.dptr(y)))
    eb = C.c_int()
    ctx.check(_lib.lib.scs_data_info(ctx.h, C.byref(eb), None, None))
    return A.T, y, eb.value


@pytest.fixture(scope="module")
def doors():
    h, d = _lib.Context(0), _lib.Context(0)
    yield h, d
    h.close()
    d.close()


def as_layout(A, layout):
    """a device tensor holding A (N x m) row-major or column-major"""
    T = torch.from_numpy(A).to(DEV)
    return T if layout == "rows" else T.t().contiguous().t()


def wide_loads_allowed(d, store32):
    """the library's rule (data.hip, launch_tile_device_t): base and leading stride aligned to the load"""
    es = d["elem_bytes"]
    if d["stride_m"] == 1 and (d["stride_n"] != 1 or d["N"] <= 1):
        al, lead = 16, d["stride_n"]
    else:
        al, lead = min(16, (4 if store32 else 2) * es), d["stride_m"]
    return d["ptr"] % al == 0 and (lead * es) % al == 0


def check_parity(doors, A, T, store32, what):
    h, d = doors
    N, m = A.shape
    y = np.random.default_rng(N * 1000 + m).standard_normal(N)
    host_load(h, A, y, store32)
    rc, desc = device_call(d, T, y, store32)
    d.check(rc)
    Ah, yh, eh = stored(h, N, m)
    Ad, yd, ed = stored(d, N, m)
    assert eh == ed == (4 if store32 else 8), (what, eh, ed)      # the mode decides, whatever the source type
    assert np.array_equal(bits(Ad), bits(Ah)), (what, desc)
    assert np.array_equal(bits(yd), bits(yh)), what
    want = A.astype(np.float32).astype(np.float64) if store32 else A.astype(np.float64)
    assert np.array_equal(bits(Ad), bits(want)), what


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("layout", ["rows", "cols"])
def test_bitwise_parity_with_the_host_door(doors, layout, pair):
    """every boundary N x every boundary m, in both layouts, for each source x storage pair"""
    dtype, store32 = PAIRS[pair]
    paths = set()
    for N in NS:
        for m in MS:
            A = values(N, m, dtype, 7 * N + m)
            T = as_layout(A, layout)
            d = _lib.parse_device_matrix(T.__cuda_array_interface__)
            if N > 1 and m > 1:
                assert (d["stride_n"], d["stride_m"]) == ((m, 1) if layout == "rows" else (1, N))
            paths.add(wide_loads_allowed(d, store32))
            check_parity(doors, A, T, store32, (layout, pair, N, m))
    assert paths == {True, False}      # m = 128, 300 / N = 16, 1000 load 16 bytes at a time, odd extents do not


VIEW_SHAPES = ((17, 129), (33, 300), (1000, 127), (16, 128))


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("view", ["row_slice", "col_slice", "offset_one"])
def test_views_take_the_scalar_path_to_the_same_bits(doors, view, pair):
    """row_slice: T[:, 3:3+m] of a wider row-major tensor (padded stride, a start aligned to one element
    only); col_slice: its transpose analogue; offset_one: a view that starts one element into a buffer
    (for fp32: 4-byte alignment only).  None of them allows 16-byte loads."""
    dtype, store32 = PAIRS[pair]
    tt = torch.float32 if dtype == np.float32 else torch.float64
    for N, m in VIEW_SHAPES:
        A = values(N, m, dtype, 31 * N + m)
        src = torch.from_numpy(A).to(DEV)
        if view == "row_slice":
            W = torch.full((N, m + 7), float("nan"), dtype=tt, device=DEV)
            T = W[:, 3:3 + m]
            T.copy_(src)
        elif view == "col_slice":
            W = torch.full((m + 7, N + 5), float("nan"), dtype=tt, device=DEV)
            T = W[3:3 + m, 3:3 + N].t()
            T.copy_(src)
        else:
            buf = torch.full((N * m + 1,), float("nan"), dtype=tt, device=DEV)
            T = buf[1:].view(N, m)
            T.copy_(src)
        d = _lib.parse_device_matrix(T.__cuda_array_interface__)
        assert not wide_loads_allowed(d, store32), (view, pair, N, m, d)
        if view != "col_slice":
            assert d["stride_m"] == 1 and d["stride_n"] == (m if view == "offset_one" else m + 7)
        else:
            assert d["stride_n"] == 1 and d["stride_m"] == N + 5
        check_parity(doors, A, T, store32, (view, pair, N, m))


# ---- stale destination memory ---------------------------------------------------------------------
def _traj(p, meth, **kw):
    return scsopt.iterate(meth, p, "l1", scsopt.PHuberSmootherL1L2(1.0), max_epoch=3, verbose=0, **kw)


def assert_same_solution(a, b, what=""):
    assert a.epochs == b.epochs, what
    assert np.array_equal(bits(a.x), bits(b.x)), what
    for k in HIST:
        va, vb = np.asarray(getattr(a, k), dtype=np.float64), np.asarray(getattr(b, k), dtype=np.float64)
        assert va.shape == vb.shape, (what, k)
        assert np.array_equal(bits(va), bits(vb)), (what, k, va, vb)


@pytest.mark.parametrize("layout", ["rows", "cols"])
def test_padding_is_written_over_stale_memory(layout):
    """Best effort: the context first holds a NaN-filled matrix of the same shape; the device door then
    frees that block and allocates its own, which the allocator is likely (not guaranteed) to place on
    the same memory.  The door runs no memset, so any padding element the kernel did not write would
    still be NaN and poison the products (the padding rows enter A·x and the Gram, the padding features
    Aᵀv).  That the kernel writes every element is also to be read from its code (data.hip)."""
    N, m = 17, 129
    rng = np.random.default_rng(5)
    A = rng.standard_normal((N, m)) / np.sqrt(m)
    y = (rng.random(N) < 0.5).astype(np.float64)
    x0 = 0.3 * rng.standard_normal(m)
    f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
    ph = scsopt.Problem(A, y, x0, f, 2e-3, out_fn=out)
    pd = scsopt.Problem(np.full((N, m), np.nan), y, x0, f, 2e-3, out_fn=out)
    assert np.isnan(pd.gemv_n(x0)).all()
    T = as_layout(A, layout)
    assert pd._set_device(T, y, False, None, 0) == N
    x, v, w = rng.standard_normal(m), rng.standard_normal(N), np.ones(N)
    lo = np.tril_indices(m)
    for got, want in ((pd.gemv_n(x), ph.gemv_n(x)), (pd.gemv_t(v), ph.gemv_t(v)), (pd.gram(w)[lo], ph.gram(w)[lo])):
        assert not np.isnan(got).any()
        assert np.array_equal(bits(got), bits(want))
    sd, sh = _traj(pd, scsopt.ProxGGNSCORE()), _traj(ph, scsopt.ProxGGNSCORE())
    assert not np.isnan(sd.x).any() and not np.isnan(np.asarray(sd.obj)).any()
    assert_same_solution(sd, sh)


# ---- the whole path through Problem ---------------------------------------------------------------
def _logit_data(N, m, seed):
    rng = np.random.default_rng(seed)
    A32 = (rng.standard_normal((N, m)) / np.sqrt(m)).astype(np.float32)
    xt = rng.standard_normal(m) * (rng.random(m) < 0.1)
    z = A32.astype(np.float64) @ xt
    y = np.where(rng.random(N) < 1.0 / (1.0 + np.exp(-z)), 1.0, -1.0)
    return A32, y


@pytest.mark.parametrize("method", ["nscore", "lqn"])
def test_trajectories_from_a_row_major_fp32_tensor(method):
    N, m = 1000, 150
    A32, y = _logit_data(N, m, 11)
    x0 = 0.3 * np.random.default_rng(12).standard_normal(m)
    f = losses.logistic_margin(1.0 / N)
    T = torch.from_numpy(A32).to(DEV)                       # row-major, the torch default
    pd = scsopt.Problem(T, y, x0, f, 2e-3, dense_f32=True)
    ph = scsopt.Problem(A32, y, x0, f, 2e-3, dense_f32=True)
    assert pd.N == N and pd.data_info()[:2] == ph.data_info()[:2] == (4, 1008 * 256 * 4)
    meth = scsopt.ProxNSCORE if method == "nscore" else (lambda: scsopt.ProxLQNSCORE(m=5))
    assert_same_solution(_traj(pd, meth()), _traj(ph, meth()), method)
    # without dense_f32 the float32 tensor is widened, as a float32 host array is
    pw = scsopt.Problem(T, y, x0, f, 2e-3)
    assert pw.data_info()[0] == 8
    assert np.array_equal(bits(pw.get_data()[0]), bits(A32.astype(np.float64)))


def test_minibatches_and_heldout_device_arrays():
    """batch_size over the device-door rows; Atest / ytest (and y) as device arrays, produced on a
    side stream that the library is told about through torch's current stream"""
    N, m, Nt = 1000, 130, 75
    A32, y = _logit_data(N, m, 31)
    At32, yt = _logit_data(Nt, m, 32)
    y, yt = (y + 1.0) / 2.0, (yt + 1.0) / 2.0
    x0 = 0.3 * np.random.default_rng(33).standard_normal(m)
    f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        T = torch.from_numpy(A32.astype(np.float64)).to(DEV, non_blocking=True)
        Tt = torch.from_numpy(At32).to(DEV).t().contiguous().t()      # column-major float32
        ty, tyt = torch.from_numpy(y).to(DEV), torch.from_numpy(yt).to(DEV)
        pd = scsopt.Problem(T, ty, x0, f, 2e-3, out_fn=out, Atest=Tt, ytest=tyt)
    ph = scsopt.Problem(A32.astype(np.float64), y, x0, f, 2e-3, out_fn=out, Atest=At32, ytest=yt)
    assert np.array_equal(bits(pd.get_data()[1]), bits(y))
    perm = np.random.default_rng(3).permutation(N)
    run = lambda p: _traj(p, scsopt.ProxGGNSCORE(), batch_size=256, batch_perm=perm)
    sd, sh = run(pd), run(ph)
    assert len(sd.fvaltest) == len(sd.obj) > 0
    assert_same_solution(sd, sh)
    assert pd.ftest(x0) == ph.ftest(x0)


class _Iface:
    """any object with __cuda_array_interface__ will do (here: a tensor's, with a stream entry added)"""

    def __init__(self, T, stream):
        self.keep = T
        self.__cuda_array_interface__ = dict(T.__cuda_array_interface__, version=3, stream=stream)


@pytest.mark.parametrize("stream", [1, 2, "side"])
def test_interface_stream_values(stream):
    """the interface's stream entry becomes src_stream: 1 (legacy default stream) and 2 (per-thread
    default stream) are resolved by the library, anything else is a stream handle"""
    N, m = 33, 129
    A = values(N, m, np.float64, 91)
    y = np.random.default_rng(92).standard_normal(N)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side if stream == "side" else torch.cuda.default_stream(DEV)):
        T = torch.from_numpy(A).to(DEV) * 1.0          # produced by a kernel on that stream
    obj = _Iface(T, side.cuda_stream if stream == "side" else stream)
    assert _lib.parse_device_matrix(obj.__cuda_array_interface__)["stream"] == (side.cuda_stream if stream == "side"
                                                                                else stream)
    p = scsopt.Problem(obj, y, np.zeros(m), losses.least_squares(1.0 / N), 1e-3)
    got, gy = p.get_data()
    assert np.array_equal(bits(got), bits(A)) and np.array_equal(bits(gy), bits(y))


def test_devices_with_a_device_array_is_refused_in_python():
    T = torch.zeros((8, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="devices="):
        scsopt.Problem(T, np.zeros(8), np.zeros(4), losses.least_squares(1.0 / 8), 1e-3, devices=[0, 0],
                       device_exchange="host")
    with pytest.raises(ValueError, match="contiguous"):
        scsopt.Problem(torch.zeros((16, 8), dtype=torch.float64, device=DEV)[::2, ::2], np.zeros(8), np.zeros(4),
                       losses.least_squares(1.0 / 8), 1e-3)
    with pytest.raises(TypeError, match="<f2"):
        scsopt.Problem(T.to(torch.float16), np.zeros(8), np.zeros(4), losses.least_squares(1.0 / 8), 1e-3)


# ---- two ranks on one GPU, each a row slice view of one device tensor -------------------------------
SN, SM = 1500, 140


def _shard_run(comm=None):
    A32, y = _logit_data(SN, SM, 71)
    y = (y + 1.0) / 2.0
    x0 = 0.3 * np.random.default_rng(72).standard_normal(SM)
    f, out = losses.logistic_ce(1.0 / SN), losses.sigmoid_ce(1.0 / SN)
    if comm is None:
        p = scsopt.Problem(A32.astype(np.float64), y, x0, f, 2e-3, out_fn=out)
    else:
        from scsopt.shard import row_range
        r0, r1 = row_range(SN, comm.world, comm.rank)
        T = torch.from_numpy(A32.astype(np.float64)).to(torch.device("cuda", 0))    # the whole tensor
        p = scsopt.Problem(T[r0:r1], y[r0:r1], x0, f, 2e-3, out_fn=out, comm=comm, N_global=SN, row0=r0)
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


def test_two_ranks_row_slices_of_one_tensor(tmp_path):
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(2, str(tmp_path / "store"), out), nprocs=2, join=True)
    full = _shard_run()
    r0, r1 = out[0], out[1]
    assert r0["epochs"] == r1["epochs"] == full["epochs"]
    assert r0["obj"] == r1["obj"] and np.array_equal(r0["x"], r1["x"])            # identical bits on both ranks
    np.testing.assert_allclose(r0["obj"], full["obj"], rtol=1e-10)                # tests/test_gpu_shard.py's bound
    np.testing.assert_allclose(r0["x"], full["x"], rtol=1e-8, atol=1e-12)


# ---- 64-bit offsets -------------------------------------------------------------------------------
def _check_columns(p, T, cols):
    got = p.get_columns(np.array(cols))
    for k, j in enumerate(cols):
        want = T[:, j].to("cpu").numpy().astype(np.float64)
        assert np.array_equal(bits(got[:, k]), bits(want)), j


def _big_pattern(N, m, tt):
    """element (n, j) = 4096 j + n mod 4093: below 2^24, so float32 holds it exactly, and every column
    differs from every other and from a copy of itself shifted by a power of two"""
    T = torch.empty((N, m), dtype=tt, device=DEV)
    T.copy_((torch.arange(N, device=DEV, dtype=torch.int64) % 4093).to(tt)[:, None])
    T.add_((torch.arange(m, device=DEV, dtype=torch.int64) * 4096).to(tt)[None, :])
    return T


def test_offsets_beyond_2_31_elements():
    """fp32 row-major, N·m = 2^31 + 2048 elements, fp32 storage: about 8 GiB in, 8 GiB stored"""
    N, m = 986896, 2176
    assert N * m > 2 ** 31 and N % 16 == 0 and m % 128 == 0
    T = _big_pattern(N, m, torch.float32)
    p = scsopt.Problem(T, np.zeros(N), np.zeros(m), losses.least_squares(1.0 / N), 1e-3, dense_f32=True)
    assert p.data_info()[:2] == (4, N * m * 4)
    _check_columns(p, T, [0, m - 1, m - 100])       # first, last, one more in the last panel
    p.ctx.close()
    del T
    torch.cuda.empty_cache()


def test_source_beyond_2_32_bytes():
    """fp64 row-major with an odd leading stride (the scalar path): above 2^32 bytes, below 2^31 elements"""
    N, m = 4200000, 129
    assert N * m * 8 > 2 ** 32 and N * m < 2 ** 31
    T = _big_pattern(N, m, torch.float64)
    p = scsopt.Problem(T, np.zeros(N), np.zeros(m), losses.least_squares(1.0 / N), 1e-3, dense_f32=True)
    assert p.data_info()[:2] == (4, N * 256 * 4)
    _check_columns(p, T, [0, m - 1, 127])
    p.ctx.close()
    del T
    torch.cuda.empty_cache()


# ---- refusals -------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(doors):
    h, d = doors
    N, m = 33, 129
    A = values(N, m, np.float64, 3)
    y = np.zeros(N)
    T = torch.from_numpy(A).to(DEV)
    wide = torch.zeros((2 * N, 2 * m), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    call = lambda ctx, eb, sn, sm, ptr=None: _lib.lib.scs_set_data_device(
        ctx.h, N, m, T.data_ptr() if ptr is None else ptr, eb, sn, sm, y.ctypes.data, None, N, 0)
    err = lambda ctx: _lib.lib.scs_last_error(ctx.h).decode()
    host_load(d, A, y, False)                                  # something to keep
    assert call(d, 2, m, 1) == _lib.SCS_ERR_ARG and "elem_bytes = 2" in err(d)
    assert call(d, 8, 2 * m, 2, wide.data_ptr()) == _lib.SCS_ERR_ARG and "both strides are non-unit" in err(d)
    assert call(d, 8, m - 1, 1) == _lib.SCS_ERR_ARG and "smaller than the extent" in err(d)
    assert call(d, 8, 1, N - 1) == _lib.SCS_ERR_ARG and "smaller than the extent" in err(d)
    assert call(d, 8, m, 1, 0) == _lib.SCS_ERR_ARG and "dA is NULL" in err(d)
    # nothing was freed or launched: the earlier data is still there
    assert np.array_equal(bits(stored(d, N, m)[0]), bits(A))
    g = _lib.Context(devices=[0, 0], device_exchange="host")   # scs_create_multi_ex(SCS_MULTI_HOST_EXCHANGE)
    try:
        assert call(g, 8, m, 1) == _lib.SCS_ERR_ARG and "single-device context" in err(g)
        rc = _lib.lib.scs_set_test_data_device(g.h, N, T.data_ptr(), 8, m, 1, y.ctypes.data, None, N, 0)
        assert rc == _lib.SCS_ERR_ARG and "single-device context" in err(g)
        Af = np.asfortranarray(A)                               # and the group still takes host rows
        g.check(_lib.lib.scs_set_data(g.h, N, m, Af.ctypes.data_as(_lib.c_dp), N, _lib.dptr(y), N, 0))
    finally:
        g.close()
    # held-out rows: refused without data of the same door's checks, accepted after
    rc = _lib.lib.scs_set_test_data_device(d.h, N, T.data_ptr(), 2, m, 1, y.ctypes.data, None, N, 0)
    assert rc == _lib.SCS_ERR_ARG and "elem_bytes = 2" in err(d)
    check_parity(doors, A, T, True, "after the refusals")
