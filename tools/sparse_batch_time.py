"""Time minibatches of a sparse A under ProxLQNSCORE at one shape, on one MI355X: the dense batch view
(the yardstick: scs_set_sparse_batches off, the reference's Matrix(As')) against the sparse view
(switch on).

    python tools/sparse_batch_time.py N m k batch_size [--rounds 5] [--arms off,on] [--f32]

The data is scs_gen_sparse's (N a power of two, m | N, k entries per row).  Both arms run in one
process on one context.  A round of an arm: set the switch (which drops the pooled views), then two
epochs over the shuffled loader's batches -- the first builds every view, the second is the steady
state -- each batch as select_batch (host clock around the call, which ends in a stream synchronise)
and one ProxLQNSCORE step on the selected view (host clock around scs_step).  After one warm-up round
of every arm the arms alternate, off then on, over --rounds rounds; the range over rounds of an arm is
its spread.  Reported per arm: the view build per batch (select_batch in the first epoch: memset +
densify, or the sparse build), select_batch on a held view, the step on a held view (second epoch),
both epochs, and the device bytes of the views.

Per-kernel times come from running this script under `rocprofv3 --kernel-trace --stats` in a run of its
own (--rounds 1 --arms on).
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
import scsopt  # noqa: E402
from scsopt import _lib, losses  # noqa: E402
from scsopt.iterate import init_method, loader_batches  # noqa: E402


def epoch(p, nb, x, x_prev, it):
    """One pass over the batches: per-batch select_batch and scs_step times (ms), the new (x, x_prev)"""
    sel, stp = np.empty(nb), np.empty(nb)
    x_new, pri = np.empty_like(x), C.c_double()
    for b in range(nb):
        t0 = time.perf_counter()
        p.select_batch(b)
        t1 = time.perf_counter()
        p.ctx.check(_lib.lib.scs_step(p.ctx.h, _lib.dptr(x), _lib.dptr(x_prev), it, _lib.dptr(x_new), None,
                                      C.byref(pri)))
        t2 = time.perf_counter()
        sel[b], stp[b] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        x_prev, x, x_new = x, x_new, x_prev
    p.select_batch(-1)
    return sel, stp, x, x_prev


def arm_round(p, on, nb, x0, meth):
    base = p.data_info()[2]
    p.set_sparse_batches(not on)       # a change of the switch drops the pooled views: every round
    p.set_sparse_batches(on)           # of an arm starts without any
    base = min(base, p.data_info()[2])
    init_method(meth, p)
    x, xp = x0.copy(), x0.copy()
    out = {}
    for name, it in (("first", 1), ("steady", 2)):
        t0 = time.perf_counter()
        sel, stp, x, xp = epoch(p, nb, x, xp, it)
        out[name] = {"epoch_ms": (time.perf_counter() - t0) * 1e3, "select_ms": sel.tolist(), "step_ms": stp.tolist()}
    nv, vb, builds = p.batch_info()
    out["sparse_views"], out["sparse_view_bytes"], out["builds"] = nv, vb, builds
    out["ctx_bytes"] = p.data_info()[2]
    assert np.all(np.isfinite(x))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", type=int)
    ap.add_argument("m", type=int)
    ap.add_argument("k", type=int)
    ap.add_argument("batch_size", type=int)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default="off,on")
    ap.add_argument("--f32", action="store_true", help="fp32-stored values")
    args = ap.parse_args()
    N, m, k, bs = args.N, args.m, args.k, args.batch_size
    arms = [a for a in args.arms.split(",") if a]
    x0 = np.zeros(m)
    t0 = time.perf_counter()
    p = scsopt.Problem.synthetic_sparse(N, m, x0, losses.least_squares(1.0 / N), 1e-3, density=k / m, f32=args.f32)
    gen_ms = (time.perf_counter() - t0) * 1e3
    p.configure("l1", scsopt.PHuberSmootherL1L2(1.0))
    meth = scsopt.ProxLQNSCORE(m=5)
    init_method(meth, p)
    batches = loader_batches(N, bs, perm=np.random.default_rng(4).permutation(N))
    nb = len(batches)
    data_bytes = p.data_info()[2]
    p.set_batches(batches)
    res = {"N": N, "m": m, "k": k, "nnz": p.nnz, "batch_size": bs, "nbatch": nb, "rounds": args.rounds, "f32": args.f32,
           "device": torch.cuda.get_device_name(0), "gen_ms": gen_ms, "ctx_bytes_before_batches": data_bytes,
           "dense_view_bytes": min(bs, N) * ((m + 127) // 128 * 128) * 8, "arms": {a: [] for a in arms}}
    try:
        for a in arms:                                   # warm-up: one round of every arm
            arm_round(p, a == "on", nb, x0, meth)
        for r in range(args.rounds):
            for a in arms:
                o = arm_round(p, a == "on", nb, x0, meth)
                res["arms"][a].append(o)
                print(f"round {r} {a:3s}: first epoch {o['first']['epoch_ms']:9.1f} ms, steady epoch "
                      f"{o['steady']['epoch_ms']:9.1f} ms, steady step {np.median(o['steady']['step_ms']):7.3f} ms",
                      flush=True)
    finally:
        p.set_batches(None)
        p.ctx.close()   # before the runtime (and any profiler) tears down, as bench.py does

    def line(tag, per_round):
        ts = np.array(per_round)
        print(f"  {tag:34s} {np.median(ts):10.3f} ms ({ts.min():10.3f} .. {ts.max():10.3f})   rounds: "
              + " ".join(f"{t:.3f}" for t in ts))
        return float(np.median(ts)), float(ts.min()), float(ts.max())

    print(f"N = {N}, m = {m}, k = {k} (nnz = {res['nnz']}), {nb} batches of {bs} rows on {res['device']}; {args.rounds} "
          "alternated rounds after a warm-up; median (min .. max) over rounds; per-batch figures are a round's median")
    summ = {}
    for a in arms:
        rs = res["arms"][a]
        if not rs:
            continue
        print(f"switch {a}:")
        s = {}
        s["build"] = line("view build per batch", [np.median(o["first"]["select_ms"]) for o in rs])
        s["build_max"] = line("view build, slowest batch", [np.max(o["first"]["select_ms"]) for o in rs])
        s["select_steady"] = line("select_batch, second epoch", [np.median(o["steady"]["select_ms"]) for o in rs])
        s["step"] = line("step on a held view", [np.median(o["steady"]["step_ms"]) for o in rs])
        s["epoch_first"] = line("first epoch", [o["first"]["epoch_ms"] for o in rs])
        s["epoch_steady"] = line("steady epoch", [o["steady"]["epoch_ms"] for o in rs])
        vb = rs[-1]["sparse_view_bytes"] if a == "on" else rs[-1]["ctx_bytes"] - data_bytes
        print(f"  device bytes of the views: {vb / 2**20:.1f} MiB ({rs[-1]['sparse_views']} sparse views, "
              f"{rs[-1]['builds']} builds since set_batches)")
        s["view_bytes"] = vb
        summ[a] = s
    if "off" in summ and "on" in summ:
        d, s = summ["off"], summ["on"]
        for key, tag in (("step", "steady step"), ("epoch_steady", "steady epoch"), ("epoch_first", "first epoch")):
            spread = d[key][2] - d[key][1]
            print(f"{tag}: dense {d[key][0]:.3f} ms (spread {spread:.3f}), sparse {s[key][0]:.3f} ms: "
                  f"{d[key][0] / s[key][0]:.2f} x, gain {d[key][0] - s[key][0]:.3f} ms "
                  f"{'>' if d[key][0] - s[key][0] > spread else '<='} the dense arm's spread")
        # the dense step does not depend on the density, the sparse step's products scale with it
        print(f"density {k / m:.4f}; steps cross near density {k / m * d['step'][0] / s['step'][0]:.3f} if the sparse "
              "step scaled with nnz alone (it has a fixed part, so later)")
    res["summary"] = summ
    print(json.dumps(res))


if __name__ == "__main__":
    main()
