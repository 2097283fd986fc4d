"""fp32-stored against fp64-stored dense A (scs_set_dense_f32) at one shape (N, m): the times of
A·x, Aᵀv, the main Gram (Aᵀv fused into it, and not) and a ProxLQNSCORE epoch, from the library's
own event timers (scs_timing) after a warm-up, for an fp64 and then an fp32 context on scs_gen_data
of the same seed.  Prints per repeat the times, the GB/s of the two streaming passes on their
algorithmic bytes (N·m elements of A) and the TF/s of the Gram on N·m·(m+1) flops, then the
fp32 / fp64 ratios with their spread over the repeats, and one JSON line.

    python tools/dense_f32_time.py N m [--repeats 3] [--calls 10] [--epochs 6] [--no-gram] [--no-lqn]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "selfconcordantsmoothoptimization.jl_amd"))
import scsopt  # noqa: E402
from scsopt import _lib, losses  # noqa: E402


def timed(p, fn, key):
    """ms per bracketed call of `key` ("gemv", "gram", "step") over what fn() launches"""
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    fn()
    t = p.ctx.timing()
    return t[key + "_ms"] / max(t[key + "_calls"], 1)


def measure(N, m, f32, args):
    x0 = np.zeros(m)
    p = scsopt.Problem.synthetic(N, m, x0, losses.least_squares(1.0 / N), 1e-3, kind=3, seed=args.seed, dense_f32=f32)
    p.C_set = [-1.0, 1.0]
    elem, a_bytes, ctx_bytes = p.data_info()
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
    rng = np.random.default_rng(1)
    xs = [rng.standard_normal(m) for _ in range(args.calls + 2)]
    w = rng.random(N) + 0.1
    v = rng.standard_normal(N)
    out = {"elem_bytes": elem, "a_bytes": a_bytes, "ctx_bytes": ctx_bytes, "ax_ms": [], "atv_ms": [],
           "gram_fused_ms": [], "gram_unfused_ms": [], "lqn_epoch_ms": []}

    def ax():
        for x in xs[2:]:
            p.fx(x)   # a new x each call: A·x is not served from the z cache

    def atv():
        for x in xs[2:]:
            p.fx(x)      # (its A·x lands in the z cache, so gradx below times Aᵀv alone)
            p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
            p.gradx(x)
            t = p.ctx.timing()
            acc.append(t["gemv_ms"] / max(t["gemv_calls"], 1))

    pairs = [(0, 0), (m - 1, m - 1)]
    for x in xs[:2]:   # warm-up
        p.fx(x)
        p.gradx(x)
    for _ in range(args.repeats):
        out["ax_ms"].append(timed(p, ax, "gemv"))
        acc = []
        atv()
        out["atv_ms"].append(float(np.mean(acc)))
    if not args.no_gram:
        for fuse, key in (("2", "gram_fused_ms"), ("0", "gram_unfused_ms")):
            os.environ["SCS_GRAM_FUSE"] = fuse   # read per call
            p.gram_atv_sample(w, v, pairs)       # warm-up
            for _ in range(args.repeats):
                out[key].append(timed(p, lambda: p.gram_atv_sample(w, v, pairs), "gram"))
        os.environ.pop("SCS_GRAM_FUSE", None)
        out["gram_kernel"] = p.ctx.kernel_names()[0]
    if not args.no_lqn:
        hm = scsopt.PHuberSmootherIndBox(-1.0, 1.0, 0.6)
        run = lambda k: scsopt.iterate(scsopt.ProxLQNSCORE(m=5), p, "indbox", hm, max_epoch=k, x_tol=0.0, f_tol=0.0,
                                       verbose=0)
        run(2)   # warm-up
        for _ in range(args.repeats):
            out["lqn_epoch_ms"].append(timed(p, lambda: run(args.epochs), "step"))
    p.ctx.close()   # before the runtime (and any profiler) tears down, as bench.py does
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", type=int)
    ap.add_argument("m", type=int)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-gram", action="store_true")
    ap.add_argument("--no-lqn", action="store_true")
    args = ap.parse_args()
    N, m = args.N, args.m
    res = {"N": N, "m": m, "repeats": args.repeats}
    for f32 in (False, True):
        tag = "fp32" if f32 else "fp64"
        r = res[tag] = measure(N, m, f32, args)
        eb = r["elem_bytes"]
        print(f"{tag}: A {r['a_bytes'] / 2**30:.2f} GiB ({eb} B/element), context {r['ctx_bytes'] / 2**30:.2f} GiB")
        for key, what in (("ax_ms", "A·x"), ("atv_ms", "Aᵀv")):
            for t in r[key]:
                print(f"  {what:6s} {t:9.3f} ms  {N * m * eb / (t * 1e6):8.1f} GB/s")
        for key, what in (("gram_fused_ms", "Gram + Aᵀv fused"), ("gram_unfused_ms", "Gram alone")):
            for t in r[key]:
                print(f"  {what:18s} {t:9.2f} ms  {N * m * (m + 1) / (t * 1e9):7.2f} TF/s")
        for t in r["lqn_epoch_ms"]:
            print(f"  ProxLQNSCORE epoch {t:9.3f} ms")
        sys.stdout.flush()
    res["ratio"] = {}
    for key in ("ax_ms", "atv_ms", "gram_fused_ms", "gram_unfused_ms", "lqn_epoch_ms"):
        a, b = np.array(res["fp64"][key]), np.array(res["fp32"][key])
        if a.size == 0 or b.size == 0:
            continue
        q = b / a.mean()   # each fp32 repeat against the fp64 mean; the fp64 spread is printed beside it
        res["ratio"][key] = {"fp32_over_fp64": float(b.mean() / a.mean()), "min": float(q.min()), "max": float(q.max()),
                             "fp64_spread": float((a.max() - a.min()) / a.mean())}
        print(f"fp32 / fp64 {key[:-3]:14s} {b.mean() / a.mean():.3f}  (repeats {q.min():.3f} .. {q.max():.3f}; "
              f"fp64 run-to-run spread {100 * (a.max() - a.min()) / a.mean():.1f} %)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
