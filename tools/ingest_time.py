"""Time the ingestion of a dense A at one shape (N, m), on one MI355X:

  * the device door (scs_set_data_device) from a device tensor, row-major and column-major, for the four
    source x storage type pairs;
  * the host door (scs_set_data / scs_set_data_f32) from the same values in host memory;
  * hipMemcpyAsync device-to-device (torch's Tensor.copy_) of the same byte counts in the same process:
    the yardstick.

A call's time is a host clock around the whole C call, which ends in a stream synchronise: it holds
what a user waits for -- freeing the previous block, hipMalloc of the new one, the re-tile kernel, the
N- and m-sized work buffers.  The copy is timed the same way into a buffer that exists already (and by
device events, printed beside it).  After a warm-up of every arm the arms are alternated over --rounds
rounds; the median, the range and every round are printed.  GB/s counts the bytes read plus the bytes written:
N·m source elements + Npad·mpad stored ones for a door, twice the buffer for the copy.  Kernel-only
times come from running this script under `rocprofv3 --kernel-trace --stats` (--no-host --rounds 1).

    python tools/ingest_time.py [N m] [--rounds 5] [--host-rounds 2] [--no-host]
"""
import argparse
import ctypes as C
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
PAIRS = (("f64", "f64"), ("f64", "f32"), ("f32", "f64"), ("f32", "f32"))
ES = {"f64": 8, "f32": 4}


def device_door(ctx, T, y, store32):
    d = _lib.parse_device_matrix(T.__cuda_array_interface__)
    ctx.check(_lib.lib.scs_set_dense_f32(ctx.h, int(store32)))
    t0 = time.perf_counter()
    rc = _lib.lib.scs_set_data_device(ctx.h, d["N"], d["m"], d["ptr"], d["elem_bytes"], d["stride_n"], d["stride_m"],
                                      y.ctypes.data, None, d["N"], 0)
    t1 = time.perf_counter()
    ctx.check(rc)
    return (t1 - t0) * 1e3


def host_door(ctx, Af, y, store32):
    """Af: N x m, Fortran order (the layout scs_set_data takes; no host transpose is timed)"""
    N, m = Af.shape
    ctx.check(_lib.lib.scs_set_dense_f32(ctx.h, int(store32)))
    t0 = time.perf_counter()
    if Af.dtype == np.float32:
        rc = _lib.lib.scs_set_data_f32(ctx.h, N, m, Af.ctypes.data_as(C.c_void_p), N, _lib.dptr(y), N, 0)
    else:
        rc = _lib.lib.scs_set_data(ctx.h, N, m, Af.ctypes.data_as(_lib.c_dp), N, _lib.dptr(y), N, 0)
    t1 = time.perf_counter()
    ctx.check(rc)
    return (t1 - t0) * 1e3


def d2d_copy(dst, src):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def columns(ctx, N, cols):
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    out = np.empty((cols.size, N))
    ctx.check(_lib.lib.scs_get_columns(ctx.h, cols.ctypes.data_as(_lib.c_i64p), cols.size, _lib.dptr(out)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", type=int, nargs="?", default=1 << 20)
    ap.add_argument("m", type=int, nargs="?", default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    N, m = args.N, args.m
    Npad, mpad = max(-(-N // 16) * 16, 16), -(-m // 128) * 128
    rng = np.random.default_rng(7)
    an, bm = rng.standard_normal(N), rng.standard_normal(m) / np.sqrt(m)
    y = np.zeros(N)
    # element (n, j) = an[n] * bm[j]: one fp64 product, the same bits on the host and on the device
    ta, tb = torch.from_numpy(an).to(DEV), torch.from_numpy(bm).to(DEV)
    src = {("rows", "f64"): torch.outer(ta, tb)}
    src[("cols", "f64")] = torch.outer(tb, ta).t()
    src[("rows", "f32")] = src[("rows", "f64")].to(torch.float32)
    src[("cols", "f32")] = src[("cols", "f64")].t().to(torch.float32).t()
    for (lay, _), T in src.items():
        d = _lib.parse_device_matrix(T.__cuda_array_interface__)
        assert (d["stride_n"], d["stride_m"]) == ((m, 1) if lay == "rows" else (1, N)), d
    dst = {t: torch.empty(N * m, dtype=src[("rows", t)].dtype, device=DEV) for t in ("f64", "f32")}
    torch.cuda.synchronize()
    ctx = _lib.Context(0)
    cols = [0, m // 2, m - 1]
    res = {"N": N, "m": m, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "door_ms": {}, "copy_ms": {},
           "host_ms": {}}
    arms = [(lay, s, a) for lay in ("rows", "cols") for s, a in PAIRS]
    byts = lambda s, a: N * m * ES[s] + Npad * mpad * ES[a]
    try:
        stored = {}
        for lay, s, a in arms:   # warm-up of every arm, and the stored columns for the check below
            device_door(ctx, src[(lay, s)], y, a == "f32")
            stored[(lay, s, a)] = columns(ctx, N, cols)
        for t in ("f64", "f32"):
            d2d_copy(dst[t], src[("rows", t)].view(-1))
        for r in range(args.rounds):
            for lay, s, a in arms:
                res["door_ms"].setdefault(f"{lay} {s}->{a}", []).append(device_door(ctx, src[(lay, s)], y, a == "f32"))
            for t in ("f64", "f32"):
                w, e = d2d_copy(dst[t], src[("rows", t)].view(-1))
                res["copy_ms"].setdefault(t, []).append(w)
                res["copy_ms"].setdefault(t + "_events", []).append(e)
        same = True
        if not args.no_host:
            Af64 = np.multiply.outer(bm, an).T          # N x m, Fortran order
            Af32 = np.asfortranarray(Af64.astype(np.float32))
            for s, a, Af in (("f64", "f64", Af64), ("f64", "f32", Af64), ("f32", "f32", Af32)):
                for r in range(args.host_rounds + 1):   # the first is the warm-up
                    t = host_door(ctx, Af, y, a == "f32")
                    if r:
                        res["host_ms"].setdefault(f"{s}->{a}", []).append(t)
                hc = columns(ctx, N, cols)
                for lay in ("rows", "cols"):
                    same = same and np.array_equal(hc.view(np.int64), stored[(lay, s, a)].view(np.int64))
            res["same_bits_as_host_door"] = bool(same)
    finally:
        ctx.close()   # before the runtime (and any profiler) tears down, as bench.py does

    def line(tag, ts, nbytes):
        # the median, not the mean: a call that frees one multi-GiB block and allocates another now and
        # then spends seconds in hipMalloc (every round is listed, so such a round shows)
        ts = np.array(ts)
        med = float(np.median(ts))
        print(f"  {tag:22s} {med:9.2f} ms ({ts.min():8.2f} .. {ts.max():8.2f})  {nbytes / (med * 1e6):8.1f} GB/s   rounds: "
              + " ".join(f"{t:.2f}" for t in ts))
        return nbytes / (med * 1e6)

    print(f"N = {N}, m = {m} on {res['device']}: fp64 matrix {N * m * 8 / 2**30:.2f} GiB; {args.rounds} alternated rounds "
          f"after a warm-up; median (min .. max); GB/s = (bytes read + bytes written) / the median time")
    print("hipMemcpyAsync device-to-device, host clock / device events:")
    res["copy_gbs"] = {}
    for t in ("f64", "f32"):
        res["copy_gbs"][t] = line(f"copy {t} (host clock)", res["copy_ms"][t], 2 * N * m * ES[t])
        line(f"copy {t} (events)", res["copy_ms"][t + "_events"], 2 * N * m * ES[t])
    print("device door (scs_set_data_device), host clock around the call:")
    res["door_gbs"], res["door_over_copy"] = {}, {}
    for lay, s, a in arms:
        k = f"{lay} {s}->{a}"
        res["door_gbs"][k] = line(k, res["door_ms"][k], byts(s, a))
        # against the copy that moves the source's type (the larger of the two streams when they differ)
        res["door_over_copy"][k] = res["door_gbs"][k] / res["copy_gbs"][s if ES[s] >= ES[a] else a]
    print("device door GB/s over the copy's GB/s (host clocks): "
          + ", ".join(f"{k} {v:.2f}" for k, v in res["door_over_copy"].items()))
    if res["host_ms"]:
        print("host door (scs_set_data / scs_set_data_f32), Fortran-order host rows, host clock:")
        for k, ts in res["host_ms"].items():
            s, a = k.split("->")
            line(k, ts, byts(s, a))
        print("stored columns equal the host door's bit for bit:", res["same_bits_as_host_door"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
