"""Time the ingestion of a sparse A at one shape (N rows of k entries, m columns), on one MI355X:

  * the device door (scs_set_sparse_device) from a CSR built on the device with torch: int64 and int32
    pointers / indices, an fp64 source stored as fp64 and an fp32 source stored as fp32;
  * the host door on the same matrix, as its bindings run it: scipy's tocsc() of the host CSR, then
    scs_set_sparse (both timed, one after the other);
  * hipMemcpyAsync device-to-device (torch's Tensor.copy_) of a buffer whose copy moves as many bytes as
    the ingest pass reads plus writes: the yardstick.

A call's time is a host clock around the whole C call, which ends in a stream synchronise: it holds what
a user waits for -- the ingest and validation pass, the row sort, the transposition (claim, scan, place),
the column sort, both blocked copies, every hipMalloc / hipFree in between, and freeing the previous
data.  After a warm-up of every arm the arms are alternated over --rounds rounds; the median, the range
and every round are printed.  Per-kernel times come from running this script under
`rocprofv3 --kernel-trace --stats` in a run of its own (--no-host --rounds 1 --arms i64_f64).

The matrix: row r holds the columns (h(r) + 97 j) mod m, j = 0..k-1, in that order (m a power of two:
distinct within a row, unsorted where the row wraps), values N(0, 1) / sqrt(k).

    python tools/sparse_ingest_time.py [N m k] [--rounds 5] [--host-rounds 1] [--no-host] [--arms a,b]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # before scsopt: one HIP runtime (scsopt/_lib.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "selfconcordantsmoothoptimization.jl_amd"))
from scsopt import _lib  # noqa: E402

DEV = torch.device("cuda", 0)
# arm: (pointer / index bytes, source value bytes, stored fp32)
ARMS = {"i64_f64": (8, 8, 0), "i32_f64": (4, 8, 0), "i64_f32": (8, 4, 1), "i32_f32": (4, 4, 1)}


def build(N, m, k):
    """(indptr int64, indices int64, values fp64) on the device"""
    assert m & (m - 1) == 0 and k <= m, "m must be a power of two and k <= m"
    r = torch.arange(N, device=DEV, dtype=torch.int64)
    h = (r * 2654435761 + (r >> 7) * 40503) % m
    indices = torch.empty((N, k), device=DEV, dtype=torch.int64)
    step = max(1, (1 << 26) // k)
    j = torch.arange(k, device=DEV, dtype=torch.int64)[None, :] * 97
    for a in range(0, N, step):          # in row chunks: the int64 temporaries stay small
        indices[a:a + step] = (h[a:a + step, None] + j) % m
    gen = torch.Generator(device=DEV).manual_seed(7)
    values = torch.randn(N * k, device=DEV, dtype=torch.float64, generator=gen) / np.sqrt(k)
    indptr = torch.arange(N + 1, device=DEV, dtype=torch.int64) * k
    return indptr, indices.reshape(-1), values


def device_door(ctx, N, m, src, y, f32):
    ip, ix, dv = src
    t0 = time.perf_counter()
    rc = _lib.lib.scs_set_sparse_device(ctx.h, N, m, ix.numel(), ip.data_ptr(), ip.element_size(), ix.data_ptr(),
                                        ix.element_size(), dv.data_ptr(), dv.element_size(), f32, y.ctypes.data,
                                        None, N, 0)
    t1 = time.perf_counter()
    ctx.check(rc)
    return (t1 - t0) * 1e3


def host_door(ctx, N, m, S, y, f32):
    """(scipy tocsc ms, scs_set_sparse ms): what Problem._set_sparse does with a scipy CSR"""
    t0 = time.perf_counter()
    T = S.tocsc()
    t1 = time.perf_counter()
    a = [np.ascontiguousarray(S.indptr, dtype=np.int64), np.ascontiguousarray(S.indices, dtype=np.int32),
         np.ascontiguousarray(S.data, dtype=np.float64), np.ascontiguousarray(T.indptr, dtype=np.int64),
         np.ascontiguousarray(T.indices, dtype=np.int32), np.ascontiguousarray(T.data, dtype=np.float64)]
    i64, i32 = _lib.c_i64p, _lib.c_i32p
    t2 = time.perf_counter()
    rc = _lib.lib.scs_set_sparse(ctx.h, N, m, int(a[2].size), a[0].ctypes.data_as(i64), a[1].ctypes.data_as(i32),
                                 _lib.dptr(a[2]), a[3].ctypes.data_as(i64), a[4].ctypes.data_as(i32), _lib.dptr(a[5]),
                                 f32, _lib.dptr(y), N, 0)
    t3 = time.perf_counter()
    ctx.check(rc)
    return (t1 - t0) * 1e3, (t3 - t2) * 1e3, (t2 - t1) * 1e3


def d2d_copy(dst, src):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def products(ctx, N, m):
    """A x and Aᵀ v of two fixed vectors, as bits: the cheap full-size check that two doors agree"""
    rng = np.random.default_rng(3)
    x, v = rng.standard_normal(m), rng.standard_normal(N)
    on, ot = np.empty(N), np.empty(m)
    ctx.check(_lib.lib.scs_gemv_n_eval(ctx.h, _lib.dptr(x), _lib.dptr(on)))
    ctx.check(_lib.lib.scs_gemv_t_eval(ctx.h, _lib.dptr(v), _lib.dptr(ot)))
    return on.view(np.int64).copy(), ot.view(np.int64).copy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", type=int, nargs="?", default=1 << 20)
    ap.add_argument("m", type=int, nargs="?", default=1 << 16)
    ap.add_argument("k", type=int, nargs="?", default=655)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--arms", default=",".join(ARMS))
    args = ap.parse_args()
    N, m, k = args.N, args.m, args.k
    arms = [a for a in args.arms.split(",") if a]
    nnz = N * k
    y = np.zeros(N)
    ip64, ix64, v64 = build(N, m, k)
    src = {}
    for a in arms:
        ib, vb, _ = ARMS[a]
        src[a] = (ip64 if ib == 8 else ip64.to(torch.int32) if nnz < 2 ** 31 else ip64,
                  ix64 if ib == 8 else ix64.to(torch.int32), v64 if vb == 8 else v64.to(torch.float32))
    # the ingest pass reads the source once and writes int64 pointers, int32 indices and the stored values
    byts = {a: (N + 1) * src[a][0].element_size() + nnz * (ARMS[a][0] + ARMS[a][1])
            + (N + 1) * 8 + nnz * (4 + (4 if ARMS[a][2] else 8)) for a in arms}
    half = max(byts.values()) // 2     # a copy of B / 2 bytes reads B / 2 and writes B / 2
    c0, c1 = (torch.zeros(half, dtype=torch.uint8, device=DEV) for _ in range(2))
    cbuf = {a: (c0[:byts[a] // 2], c1[:byts[a] // 2]) for a in arms}
    torch.cuda.synchronize()
    ctx = _lib.Context(0)
    res = {"N": N, "m": m, "k": k, "nnz": nnz, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ingest_bytes": byts, "door_ms": {}, "copy_ms": {}, "host_ms": {}}
    try:
        stored = {}
        for a in arms:   # warm-up of every arm, and the products for the check below
            device_door(ctx, N, m, src[a], y, ARMS[a][2])
            stored[a] = products(ctx, N, m)
            d2d_copy(*cbuf[a])
        for r in range(args.rounds):
            for a in arms:
                res["door_ms"].setdefault(a, []).append(device_door(ctx, N, m, src[a], y, ARMS[a][2]))
                w, e = d2d_copy(*cbuf[a])
                res["copy_ms"].setdefault(a, []).append(w)
                res["copy_ms"].setdefault(a + "_events", []).append(e)
            print(f"round {r}: " + ", ".join(f"{a} {res['door_ms'][a][-1]:.1f} ms" for a in arms), flush=True)
        if not args.no_host:
            import scipy.sparse as sp
            print("host door: copying the CSR to the host ...", flush=True)
            S = sp.csr_matrix((v64.cpu().numpy(), ix64.to(torch.int32).cpu().numpy(), ip64.cpu().numpy()), shape=(N, m))
            same = True
            for a in [a for a in ("i64_f64", "i64_f32") if a in arms] or arms[:1]:
                f32 = ARMS[a][2]
                for r in range(args.host_rounds):
                    t_csc, t_set, t_conv = host_door(ctx, N, m, S, y, f32)
                    res["host_ms"].setdefault(a, []).append({"tocsc": t_csc, "scs_set_sparse": t_set,
                                                              "dtype_conversions": t_conv})
                    print(f"host door {a}: tocsc {t_csc:.0f} ms, scs_set_sparse {t_set:.0f} ms", flush=True)
                hp = products(ctx, N, m)
                same = same and all(np.array_equal(p, q) for p, q in zip(hp, stored[a]))
            res["same_products_as_host_door"] = bool(same)
    finally:
        ctx.close()   # before the runtime (and any profiler) tears down, as bench.py does

    def line(tag, ts, nbytes):
        ts = np.array(ts)
        med = float(np.median(ts))
        print(f"  {tag:24s} {med:9.2f} ms ({ts.min():8.2f} .. {ts.max():8.2f})  {nbytes / (med * 1e6):8.1f} GB/s   rounds: "
              + " ".join(f"{t:.2f}" for t in ts))
        return med

    print(f"N = {N}, m = {m}, k = {k} (nnz = {nnz}) on {res['device']}; {args.rounds} alternated rounds after a warm-up; "
          "median (min .. max); GB/s = the ingest pass's bytes (read + written) / the median time")
    print("device door (scs_set_sparse_device), host clock around the call:")
    res["door_median_ms"] = {a: line(a, res["door_ms"][a], byts[a]) for a in arms} if args.rounds else {}
    print("hipMemcpyAsync device-to-device moving the same bytes, host clock / device events:")
    for a in arms if args.rounds else []:
        line(f"copy {a} (host clock)", res["copy_ms"][a], byts[a])
        line(f"copy {a} (events)", res["copy_ms"][a + "_events"], byts[a])
    if res["host_ms"]:
        print("host door (scipy tocsc() + scs_set_sparse), host clock:")
        for a, rs in res["host_ms"].items():
            tot = float(np.median([r["tocsc"] + r["scs_set_sparse"] for r in rs]))
            print(f"  {a:24s} {tot:9.0f} ms = tocsc {np.median([r['tocsc'] for r in rs]):.0f} + scs_set_sparse "
                  f"{np.median([r['scs_set_sparse'] for r in rs]):.0f}  (int32 / float64 array conversions, not counted: "
                  f"{np.median([r['dtype_conversions'] for r in rs]):.0f} ms)")
            if a in res["door_median_ms"]:
                print(f"  {'':24s} device door {res['door_median_ms'][a]:.1f} ms: {tot / res['door_median_ms'][a]:.1f} x")
        print("products A x, Aᵀ v equal the host door's bit for bit:", res["same_products_as_host_door"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
