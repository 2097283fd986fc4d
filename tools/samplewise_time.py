"""What a sample-wise loss (losses.samplewise, scs_set_loss_samplewise) costs against the menu kind for
the same loss, in one process, on device-generated data of one seed.

(1) one f + ∇f evaluation (scs_eval_grad: A·x, the loss epilogue, Aᵀg) of the logistic-margin loss at
    (N, m), three ways: the menu kind, a device-mode sample-wise loss written in torch, a host-mode one
    written in NumPy;
(2) one ProxGGNSCORE step of the sigmoid / cross-entropy problem at (N2, m2) (default: BASELINE
    configs[1]'s shape, 100000 x 8192), as the menu kind and as a device-mode sample-wise loss.

Every way has its own context on the same generated data; all are built and warmed up first and the
repeats alternate between them (--ways gives the order), every way at the same x per repeat (a new x per
repeat: an evaluation at a cached x would skip A·x).
Times are device event times on the context's stream around the call (they include the stream's idle
gaps while the host runs the caller's functions) beside the host wall time; the library's own event
timers give the A·x + Aᵀg share, so `other` = event time - products is the epilogue side: the extra z
pass, the callables' kernels (or copies and NumPy) and the launch gaps.

    python tools/samplewise_time.py N m [--N2 100000 --m2 8192] [--repeats 3] [--no-eval] [--no-step] [--ways menu,device,host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch   # before scsopt: one HIP runtime (device mode hands torch the library's buffers)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "selfconcordantsmoothoptimization.jl_amd"))
import scsopt  # noqa: E402
from scsopt import _lib, losses  # noqa: E402
from scsopt.iterate import init_method, step  # noqa: E402


def margin_samplewise(N, device):
    xp = torch if device else np

    def value(z, y):
        return xp.log1p(xp.exp(-y * z)) / N

    def d1(z, y):
        e = xp.exp(-y * z)
        return (-y * e / (1.0 + e)) / N
    return losses.samplewise(value, d1, device=device)


def sigmoid_ce_samplewise(N):
    sig = lambda z: 1.0 / (1.0 + torch.exp(-z))  # noqa: E731

    def value(z, y):
        yh = sig(z)
        return -(y * torch.log(yh) + (1 - y) * torch.log(1 - yh)) / N

    def link_d1(z):
        yh = sig(z)
        return yh * (1 - yh)
    return losses.samplewise(value, lambda z, y: (sig(z) - y) / N, link=sig, link_d1=link_d1,
                             grad_fy=lambda y, yh: (-(y / yh) + (1 - y) / (1 - yh)) / N,
                             hess_fy=lambda y, yh: (y / yh ** 2 + (1 - y) / (1 - yh) ** 2) / N, device=True)


def timed(p, fn):
    """(device event ms on the context's stream, host wall ms, the library timers' gemv ms) of fn()"""
    s = torch.cuda.ExternalStream(p.ctx.stream(), device=torch.device("cuda", p.ctx.device))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    p.ctx.check(_lib.lib.scs_sync(p.ctx.h))
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    t0 = time.perf_counter()
    e0.record(s)
    out = fn()
    e1.record(s)
    e1.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    t = p.ctx.timing()
    return e0.elapsed_time(e1), wall, t["gemv_ms"], t["gram_ms"], t["solve_ms"], out


def eval_ways(N, m, args):
    rng = np.random.default_rng(1)
    xs = [rng.standard_normal(m) * 0.3 for _ in range(args.repeats + 2)]
    mk = {"menu": lambda: losses.logistic_margin(1.0 / N), "device": lambda: margin_samplewise(N, True),
          "host": lambda: margin_samplewise(N, False)}
    probs = {}
    for name in args.ways:   # every way's problem first (its own copy of the same A), then the repeats alternated
        p = probs[name] = scsopt.Problem.synthetic(N, m, np.zeros(m), mk[name](), 1e-3, kind=2, seed=args.seed)
        p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
        for x in xs[:2]:   # warm-up: code objects, torch's allocator, the pinned buffers
            p.gradx(x)
    res, grads = {name: [] for name in args.ways}, {}
    for x in xs[2:]:
        for name, p in probs.items():
            ev, wall, gemv, _, _, g = timed(p, lambda: p.gradx(x))
            res[name].append({"event_ms": ev, "wall_ms": wall, "products_ms": gemv, "other_ms": ev - gemv})
            print(f"  f+grad {name:7s} event {ev:9.3f} ms  wall {wall:9.3f} ms  A·x + Aᵀg {gemv:8.3f} ms  "
                  f"other {ev - gemv:8.3f} ms")
            sys.stdout.flush()
            grads[name] = g
    for p in probs.values():
        p.ctx.close()
    for name in grads:
        if name != "menu" and "menu" in grads:   # the same loss: the three ways agree to rounding
            err = float(np.max(np.abs(grads[name] - grads["menu"])) / np.max(np.abs(grads["menu"])))
            res[name + "_vs_menu_max_rel"] = err
            print(f"  max |grad({name}) - grad(menu)| / max |grad(menu)| = {err:.2e}")
    return res


def step_ways(N, m, args):
    rng = np.random.default_rng(2)
    x0 = rng.standard_normal(m) * 0.1
    hm = scsopt.PHuberSmootherL1L2(1.0)
    probs, xs = {}, {}
    for name in [w for w in args.ways if w in ("menu", "device")]:
        if name == "menu":
            f, out = losses.logistic_ce(1.0 / N), losses.sigmoid_ce(1.0 / N)
        else:
            f, out = sigmoid_ce_samplewise(N), None
        p = scsopt.Problem.synthetic(N, m, x0, f, 1e-3, kind=1, seed=args.seed, out_fn=out)
        p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
        meth = scsopt.ProxGGNSCORE()
        p.configure("l1", hm)
        init_method(meth, p)
        x, _ = step(meth, p, "l1", hm, x0, x0, 1)   # warm-up; the timed steps start from its x
        probs[name] = (p, meth, x)
    res = {name: [] for name in probs}
    for k in range(args.repeats):
        for name, (p, meth, x) in probs.items():
            xk = x + 1e-3 * (k + 1)   # a new point per repeat, the same for both ways
            ev, wall, gemv, gram, solve, (xn, _) = timed(p, lambda: step(meth, p, "l1", hm, xk, xk, 2))
            res[name].append({"event_ms": ev, "wall_ms": wall, "products_ms": gemv, "gram_ms": gram,
                              "solve_ms": solve, "other_ms": ev - gemv - gram - solve})
            print(f"  GGN step {name:7s} event {ev:9.3f} ms  wall {wall:9.3f} ms  Gram {gram:8.3f}  solve {solve:8.3f}  "
                  f"A·x {gemv:7.3f}  other {ev - gemv - gram - solve:8.3f} ms")
            sys.stdout.flush()
            xs[name] = xn
    for p, _, _ in probs.values():
        p.ctx.close()
    if "menu" in xs and "device" in xs:
        err = float(np.max(np.abs(xs["device"] - xs["menu"])) / np.max(np.abs(xs["menu"])))
        res["device_vs_menu_max_rel"] = err
        print(f"  max |x_new(device) - x_new(menu)| / max |x_new(menu)| = {err:.2e}")
    return res


def summary(rows, key="event_ms"):
    a = np.array([r[key] for r in rows])
    return {"mean": float(a.mean()), "min": float(a.min()), "max": float(a.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("N", type=int)
    ap.add_argument("m", type=int)
    ap.add_argument("--N2", type=int, default=100_000)
    ap.add_argument("--m2", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--ways", default="menu,device,host", help="which of menu, device, host to run (a profiler "
                    "run takes one way at a time, so that its kernel statistics are that way's alone)")
    args = ap.parse_args()
    args.ways = args.ways.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("samplewise_time.py measures on the GPU: no HIP device here")
    res = {"N": args.N, "m": args.m, "repeats": args.repeats}
    if not args.no_eval:
        print(f"f + grad, logistic margin, N = {args.N}, m = {args.m}")
        res["eval"] = eval_ways(args.N, args.m, args)
        base = summary(res["eval"][args.ways[0]])
        for name in args.ways:
            s, o = summary(res["eval"][name]), summary(res["eval"][name], "other_ms")
            print(f"f+grad {name:7s} {s['mean']:9.3f} ms ({s['min']:.3f} .. {s['max']:.3f}), x{s['mean'] / base['mean']:.3f} "
                  f"of {args.ways[0]}; outside the two products {o['mean']:.3f} ms ({o['min']:.3f} .. {o['max']:.3f})")
    if not args.no_step:
        print(f"one ProxGGNSCORE step, sigmoid / cross-entropy, N = {args.N2}, m = {args.m2}")
        res["step"] = step_ways(args.N2, args.m2, args)
        names = [w for w in args.ways if w in ("menu", "device")]
        base = summary(res["step"][names[0]])
        for name in names:
            s = summary(res["step"][name])
            print(f"GGN step {name:7s} {s['mean']:9.3f} ms ({s['min']:.3f} .. {s['max']:.3f}), "
                  f"x{s['mean'] / base['mean']:.4f} of {names[0]}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
