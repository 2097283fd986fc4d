"""Time the multi-output products and one multi-output ProxGGNSCORE step on one MI355X.

    python tools/multi_output_time.py [--N 1048576] [--d 2048] [--K 2,4,8,16] [--rounds 7]
                                      [--step-N 131072] [--step-d 1024] [--step-K 8] [--skip-step]

Products, per storage type (fp64, fp32) and K: A X and Aᵀ V of csrc/multi.hip (A read once for all K
columns) against the only route without them, K launches of the single-vector product (gemv_n /
gemv_t_panel), and against one such launch, the floor (one pass over A).  A is generated on the device
(torch.randn) and handed to two contexts through the device door: one with scs_set_outputs(K), one
without.  Times are the library's device events (T_GEMV) around the product launches alone -- the
repack of X / V and the finalize included, the loss epilogue and every host copy excluded: f(x) at a
fresh x times A X (or A x), ∇f at the same x then times Aᵀ R (z is cached).  After a warm-up the arms
alternate over --rounds rounds; the range over rounds is the spread.  Requirement checked and printed:
for K >= 4 the whole range of the multi-output product lies below the whole range of K single products.

The step: ProxGGNSCORE on losses.softmax_ce at (--step-N, --step-d, --step-K), event timers on: its Gram
part (K (K + 1) / 2 weight + Gram + placement rounds) beside K (K + 1) / 2 times one (N, d) weighted
Gram of the unchanged kernel on a context without outputs.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch   # before scsopt: one HIP runtime (scsopt/_lib.py)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "selfconcordantsmoothoptimization.jl_amd"))
import scsopt  # noqa: E402
from scsopt import _lib, losses  # noqa: E402
from scsopt.iterate import init_method  # noqa: E402


def timers(p, on=True):
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1 if on else 0))
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))


def gemv_ms(p):
    """(ms, calls) of the product launches since the last reset."""
    t = p.ctx.timing()
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    return t["gemv_ms"], t["gemv_calls"]


def product_round(p, xs):
    """For each x of xs: f(x) (A X fresh) then ∇f(x) (Aᵀ R, z cached).  Returns (ms of the A X launches,
    ms of the Aᵀ launches), each summed over xs."""
    ax = at = 0.0
    for x in xs:
        p.fx(x)
        t, n = gemv_ms(p)
        assert n == 1, n
        ax += t
        p.gradx(x)
        t, n = gemv_ms(p)
        assert n == 1, n
        at += t
    return ax, at


def rng_line(tag, ts):
    ts = np.asarray(ts)
    print(f"  {tag:40s} {np.median(ts):9.3f} ms ({ts.min():9.3f} .. {ts.max():9.3f})")
    return [float(np.median(ts)), float(ts.min()), float(ts.max())]


def products(N, d, Ks, rounds, f32, res):
    dt = torch.float32 if f32 else torch.float64
    tag = "fp32" if f32 else "fp64"
    g = torch.Generator(device="cuda").manual_seed(11)
    A = torch.randn((N, d), dtype=dt, device="cuda", generator=g) / np.sqrt(d)
    rng = np.random.default_rng(2)
    y1 = rng.standard_normal(N)
    p1 = scsopt.Problem(A, y1, np.zeros(d), losses.least_squares(1.0 / N), 1e-3, dense_f32=f32)
    timers(p1)
    a_bytes = p1.data_info()[1]
    print(f"--- products, {tag} storage: N = {N}, d = {d}, A = {a_bytes / 2**30:.2f} GiB")
    for K in Ks:
        Y = np.eye(K)[rng.integers(0, K, size=N)]
        pk = scsopt.Problem(A, Y, np.zeros(d * K), losses.softmax_ce(K, 1.0 / N), 1e-3, dense_f32=f32)
        timers(pk)
        fresh = lambda n: [0.1 * rng.standard_normal(n) for _ in range(1)]     # noqa: E731
        singles = lambda: [0.1 * rng.standard_normal(d) for _ in range(K)]     # noqa: E731
        product_round(pk, fresh(d * K))                      # warm-up of both arms
        product_round(p1, singles())
        m_ax, m_at, s_ax, s_at, o_ax, o_at = [], [], [], [], [], []
        for _ in range(rounds):
            a, t = product_round(pk, fresh(d * K))
            m_ax.append(a)
            m_at.append(t)
            a, t = product_round(p1, singles())              # K launches of the single-vector product
            s_ax.append(a)
            s_at.append(t)
            a, t = product_round(p1, singles()[:1])          # one launch: the floor
            o_ax.append(a)
            o_at.append(t)
        print(f"K = {K} ({tag}); median (min .. max) over {rounds} alternated rounds")
        out = {}
        out["ax_multi"] = rng_line("A X, multi-output kernel", m_ax)
        out["ax_k_single"] = rng_line(f"A x, {K} single launches", s_ax)
        out["ax_one"] = rng_line("A x, one launch (floor)", o_ax)
        out["atv_multi"] = rng_line("A' V, multi-output kernel", m_at)
        out["atv_k_single"] = rng_line(f"A' v, {K} single launches", s_at)
        out["atv_one"] = rng_line("A' v, one launch (floor)", o_at)
        for nm in ("ax", "atv"):
            mu, ks, one = out[nm + "_multi"], out[nm + "_k_single"], out[nm + "_one"]
            below = mu[2] < ks[1]
            out[nm + "_below"] = bool(below)
            print(f"  {nm}: {ks[0] / mu[0]:.2f} x faster than {K} single launches, {mu[0] / one[0]:.2f} x the floor "
                  f"({a_bytes / mu[0] / 1e9:.2f} TB/s of A); ranges "
                  f"{'do not overlap (multi below)' if below else 'OVERLAP or multi above'}"
                  + ("" if K < 4 else f" -- requirement {'met' if below else 'NOT met'}"))
        res["products"][f"{tag}_K{K}"] = out
        pk.ctx.close()
    p1.ctx.close()
    del A
    torch.cuda.empty_cache()


def step(N, d, K, rounds, res):
    g = torch.Generator(device="cuda").manual_seed(12)
    A = torch.randn((N, d), dtype=torch.float64, device="cuda", generator=g) / np.sqrt(d)
    rng = np.random.default_rng(3)
    Y = np.eye(K)[rng.integers(0, K, size=N)]
    x0 = 0.05 * rng.standard_normal(d * K)
    p = scsopt.Problem(A, Y, x0, losses.softmax_ce(K, 1.0 / N), 1e-3, out_fn=losses.linear_softmax_ce(K, 1.0 / N))
    p.configure("l1", scsopt.PHuberSmootherL1L2(0.5))
    init_method(scsopt.ProxGGNSCORE(), p)
    x_new, pri = np.empty_like(x0), C.c_double()

    def one_step():
        p.ctx.check(_lib.lib.scs_step(p.ctx.h, _lib.dptr(x0), _lib.dptr(x0), 1, _lib.dptr(x_new), None, C.byref(pri)))
    one_step()                                               # warm-up (allocates the system, loads code)
    timers(p)
    p1 = scsopt.Problem(A, np.zeros(N), np.zeros(d), losses.least_squares(1.0 / N), 1e-3)
    w = rng.random(N) - 0.3
    p1.gram(w)
    timers(p1)
    gs, ss, ts, g1 = [], [], [], []
    for _ in range(rounds):
        one_step()
        t = p.ctx.timing()
        p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
        gs.append(t["gram_ms"])
        ss.append(t["solve_ms"])
        ts.append(t["step_ms"])
        p1.gram(w)
        t = p1.ctx.timing()
        p1.ctx.check(_lib.lib.scs_timing_reset(p1.ctx.h))
        g1.append(t["gram_ms"])
    npair = K * (K + 1) // 2
    print(f"--- ProxGGNSCORE softmax step: N = {N}, d = {d}, K = {K} (system order {d * K}, {npair} Grams), fp64; "
          f"{rounds} rounds; Gram kernel {p.ctx.kernel_names()[0]}")
    out = {"npair": npair}
    out["step"] = rng_line("whole step (T_STEP)", ts)
    out["gram_part"] = rng_line("its Gram part (weights, Grams, placement)", gs)
    out["solve"] = rng_line("its solve (order d K)", ss)
    out["one_gram"] = rng_line("one (N, d) weighted Gram, unchanged kernel", g1)
    print(f"  {npair} x one Gram = {npair * out['one_gram'][0]:.3f} ms; the Gram part is "
          f"{out['gram_part'][0] / (npair * out['one_gram'][0]):.3f} x that")
    res["step"] = out
    p.ctx.close()
    p1.ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--N", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--K", default="2,4,8,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-N", type=int, default=1 << 17)
    ap.add_argument("--step-d", type=int, default=1024)
    ap.add_argument("--step-K", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    args = ap.parse_args()
    Ks = [int(k) for k in args.K.split(",") if k]
    res = {"N": args.N, "d": args.d, "K": Ks, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "products": {}}
    if not args.skip_products:
        for f32 in (False, True):
            products(args.N, args.d, Ks, args.rounds, f32, res)
    if not args.skip_step:
        step(args.step_N, args.step_d, args.step_K, args.rounds, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
