"""Time ProxGGNSCORE's sample-space step on minibatches of a sparse A at one shape, on one MI355X: the
dense path (the yardstick: scs_set_sparse_sample off -- a dense batch view, its Aᵀ copy and P on the
MFMA tiles) against P from the nonzeros on sparse views (switch on), plain and packed walk.

    python tools/sparse_sample_time.py N m k batch_size [--rounds 5] [--arms off,plain,packed]
                                       [--batches K] [--f32]

The data is scs_gen_sparse's (N a power of two, m | N, k entries per row), the loss logistic CE with the
sigmoid_ce GGN pieces; scs_set_sparse_batches is on in every arm (it changes nothing for ProxGGNSCORE
while scs_set_sparse_sample is off).  All arms run in one process on one context.  A round of an arm:
set the switches (which drops the pooled views and the system scratch), then two epochs over the first
K of the shuffled loader's batches (--batches; default all) -- the first builds every view, the second
is the steady state -- each batch as select_batch (host clock around the call, which ends in a stream
synchronise) and one ProxGGNSCORE step on the selected view (host clock around scs_step).  After one
warm-up round of every arm the arms alternate over --rounds rounds; the range over rounds of an arm is
its spread.  A last round per arm runs with the library's event timers on (T_GRAM: forming P, T_SOLVE:
the (n+1)² LU) and is not part of the host-clock figures.

Per-kernel times come from running this script under `rocprofv3 --kernel-trace --stats` in a run of its
own (--rounds 1 --arms packed).
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

ARMS = {"off": (False, None), "plain": (True, "0"), "packed": (True, "1")}


def epoch(p, nb, x, x_prev, it):
    """One pass over the first nb batches: per-batch select_batch and scs_step times (ms), the new (x, x_prev)"""
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


def arm_round(p, arm, nb, x0, meth, timers=False):
    on, kernel = ARMS[arm]
    if kernel is not None:
        os.environ["SCS_SPARSE_SAMPLE_KERNEL"] = kernel   # read per launch
    p.set_sparse_sample(not on)        # a change of the switch drops the pooled views and the system
    p.set_sparse_sample(on)            # scratch: every round of an arm starts without any
    base = p.data_info()[2]
    init_method(meth, p)
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1 if timers else 0))
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    x, xp = x0.copy(), x0.copy()
    out = {"ctx_bytes_base": base}
    for name, it in (("first", 1), ("steady", 2)):
        t0 = time.perf_counter()
        sel, stp, x, xp = epoch(p, nb, x, xp, it)
        out[name] = {"epoch_ms": (time.perf_counter() - t0) * 1e3, "select_ms": sel.tolist(), "step_ms": stp.tolist()}
    nv, vb, builds = p.batch_info()
    out["sparse_views"], out["sparse_view_bytes"], out["builds"] = nv, vb, builds
    out["ctx_bytes"] = p.data_info()[2]
    if timers:
        out["timers"] = p.ctx.timing()
        p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 0))
    out["gram_kernel"] = p.ctx.kernel_names()[0]
    assert np.all(np.isfinite(x))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", type=int)
    ap.add_argument("m", type=int)
    ap.add_argument("k", type=int)
    ap.add_argument("batch_size", type=int)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default="off,plain,packed")
    ap.add_argument("--batches", type=int, default=0, help="step on the first K batches of the list only")
    ap.add_argument("--f32", action="store_true", help="fp32-stored values")
    args = ap.parse_args()
    N, m, k, bs = args.N, args.m, args.k, args.batch_size
    arms = [a for a in args.arms.split(",") if a]
    assert all(a in ARMS for a in arms) and bs + 1 <= m, "arms off / plain / packed; the sample space needs batch_size + 1 <= m"
    x0 = np.zeros(m)
    t0 = time.perf_counter()
    p = scsopt.Problem.synthetic_sparse(N, m, x0, losses.logistic_ce(1.0 / N), 1e-3, density=k / m, f32=args.f32,
                                        out_fn=losses.sigmoid_ce(1.0 / N))
    gen_ms = (time.perf_counter() - t0) * 1e3
    p.set_sparse_batches(True)
    p.configure("l1", scsopt.PHuberSmootherL1L2(1.0))
    meth = scsopt.ProxGGNSCORE()
    init_method(meth, p)
    batches = loader_batches(N, bs, perm=np.random.default_rng(4).permutation(N))
    nb = min(args.batches, len(batches)) if args.batches > 0 else len(batches)
    data_bytes = p.data_info()[2]
    p.set_batches(batches)
    res = {"N": N, "m": m, "k": k, "nnz": p.nnz, "batch_size": bs, "nbatch": len(batches), "batches_stepped": nb,
           "rounds": args.rounds, "f32": args.f32, "device": torch.cuda.get_device_name(0), "gen_ms": gen_ms,
           "ctx_bytes_before_batches": data_bytes, "arms": {a: [] for a in arms}, "timed": {}}
    try:
        for a in arms:                                   # warm-up: one round of every arm
            arm_round(p, a, nb, x0, meth)
        for r in range(args.rounds):
            for a in arms:
                o = arm_round(p, a, nb, x0, meth)
                res["arms"][a].append(o)
                print(f"round {r} {a:6s}: first epoch {o['first']['epoch_ms']:9.1f} ms, steady epoch "
                      f"{o['steady']['epoch_ms']:9.1f} ms, steady step {np.median(o['steady']['step_ms']):9.3f} ms",
                      flush=True)
        for a in arms:                                   # the event timers, in a round of their own
            res["timed"][a] = arm_round(p, a, nb, x0, meth, timers=True)
    finally:
        p.set_batches(None)
        p.ctx.close()   # before the runtime (and any profiler) tears down, as bench.py does

    def line(tag, per_round):
        ts = np.array(per_round)
        print(f"  {tag:34s} {np.median(ts):10.3f} ms ({ts.min():10.3f} .. {ts.max():10.3f})   rounds: "
              + " ".join(f"{t:.3f}" for t in ts))
        return float(np.median(ts)), float(ts.min()), float(ts.max())

    print(f"N = {N}, m = {m}, k = {k} (nnz = {res['nnz']}), {len(batches)} batches of {bs} rows ({nb} stepped per epoch) on "
          f"{res['device']}; {args.rounds} alternated rounds after a warm-up; median (min .. max) over rounds; per-batch "
          "figures are a round's median")
    summ = {}
    for a in arms:
        rs = res["arms"][a]
        if not rs:
            continue
        print(f"arm {a}" + (f" (P by {rs[-1]['gram_kernel']}):" if ARMS[a][0] else " (P on the MFMA tiles):"))
        s = {}
        s["build"] = line("view build per batch", [np.median(o["first"]["select_ms"]) for o in rs])
        s["select_steady"] = line("select_batch, second epoch", [np.median(o["steady"]["select_ms"]) for o in rs])
        s["step"] = line("step on a held view", [np.median(o["steady"]["step_ms"]) for o in rs])
        s["epoch_first"] = line("first epoch", [o["first"]["epoch_ms"] for o in rs])
        s["epoch_steady"] = line("steady epoch", [o["steady"]["epoch_ms"] for o in rs])
        s["bytes"] = rs[-1]["ctx_bytes"] - rs[-1]["ctx_bytes_base"]
        print(f"  device bytes grown over the round (views, system scratch, build scratch): {s['bytes'] / 2**20:.1f} MiB "
              f"({rs[-1]['sparse_views']} sparse views of {rs[-1]['sparse_view_bytes'] / 2**20:.1f} MiB, "
              f"{rs[-1]['builds']} builds)")
        t = res["timed"].get(a, {}).get("timers")
        if t:
            print(f"  event timers over {t['step_calls']} steps: T_GRAM {t['gram_ms'] / max(t['gram_calls'], 1):.3f} ms x "
                  f"{t['gram_calls']}, T_SOLVE {t['solve_ms'] / max(t['solve_calls'], 1):.3f} ms x {t['solve_calls']}, "
                  f"T_STEP {t['step_ms'] / max(t['step_calls'], 1):.3f} ms")
        summ[a] = s

    def versus(a, b, key, tag):
        d, s = summ[a], summ[b]
        spread = (d[key][2] - d[key][1]) + (s[key][2] - s[key][1])
        gain = d[key][0] - s[key][0]
        print(f"{tag}: {a} {d[key][0]:.3f} ms, {b} {s[key][0]:.3f} ms: {d[key][0] / s[key][0]:.2f} x, gain {gain:.3f} ms "
              f"{'>' if gain > spread else '<='} the two arms' ranges together ({spread:.3f} ms)")
    for b in ("plain", "packed"):
        if "off" in summ and b in summ:
            for key, tag in (("step", "steady step"), ("epoch_steady", "steady epoch"), ("epoch_first", "first epoch")):
                versus("off", b, key, tag)
            print(f"bytes: off {summ['off']['bytes'] / 2**20:.1f} MiB, {b} {summ[b]['bytes'] / 2**20:.1f} MiB")
    if "plain" in summ and "packed" in summ:
        versus("plain", "packed", "step", "steady step")
    res["summary"] = summ
    print(json.dumps(res))


if __name__ == "__main__":
    main()
