"""Time minibatches of a multi-output loss on one MI355X.

    python tools/multi_batches_time.py [--shape 1048576x2048x8] [--batch 16384] [--sample-batch 1024]
                                       [--callback 4096x512x4] [--callback-batch 256] [--rounds 5] [--reps 20]
                                       [--out FILE.json]

losses.softmax_ce at scale 1/N, Problem(..., multi_batches=True, multi_sample=True), A generated on the
device (torch.randn) and handed over through the device door, fp64 and fp32 storage; shuffled batches.

  gather    one scs_select_batch (gather + synchronise) by the host clock, alternating between two batches
            that share a pool view so that every call gathers: multi.hip's one-launch kernel
            (SCS_MULTI_GATHER=1) against the other arm (=0: gather_rows_kernel over the d-column view plus
            one launch per further target column) on the same rows of the same context -- the arm is read
            where the list is registered, so each round registers the list again -- and a single-output
            context of the same N x d, which runs gather_rows_kernel as before.  Rounds alternate
            ref, new, single, ref, ...; the reference arm is therefore timed in separate rounds and the
            spread of its round medians is the run-to-run spread.  Bytes by count: 2 n_b d elements (the
            batch read once and written once; a source row uses 8 B (4 B) of every 128-B line it touches,
            which the count leaves out).
  lqn       a steady ProxLQNSCORE epoch through scs_select_batch + scs_step: per batch the gather (host
            clock) and the step's event timers (T_STEP, T_GEMV = A X and Aᵀ R together); the two products
            apart from scs_eval_f / scs_eval_grad on a context holding one batch's rows (the same kernels
            on the same shapes as a view).
  ggn       one ProxGGNSCORE step on a --batch batch (the feature branch) and on a --sample-batch batch
            (the sample-space branch): T_STEP, T_GRAM, T_SOLVE, T_GEMV and the gather.
  callback  one ProxGGNSCORE epoch over --callback-batch batches of --callback through losses.callback (one
            host-side problem per batch, J = I_K (x) A_b uploaded on every step) beside the device path on
            the same batches: wall time.

Every figure is the median (min .. max) over the timed calls after a warm-up; the last line is one JSON
object with all of them."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scsopt  # noqa: E402
from scsopt import _lib, losses  # noqa: E402
from scsopt.iterate import init_method  # noqa: E402
from multi_sample_time import softmax_closures  # noqa: E402

HM = lambda: scsopt.PHuberSmootherL1L2(0.5)   # noqa: E731


def line(tag, ts, extra=""):
    ts = np.asarray(ts, dtype=np.float64)
    print(f"  {tag:52s} {np.median(ts):10.3f} ms ({ts.min():10.3f} .. {ts.max():10.3f}){extra}", flush=True)
    return [float(np.median(ts)), float(ts.min()), float(ts.max())]


def data(N, d, K, seed, dtype=torch.float64):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn((N, d), dtype=torch.float64, device="cuda", generator=g) / np.sqrt(d)
    rng = np.random.default_rng(seed)
    Y = np.eye(K)[rng.integers(0, K, size=N)]
    x0 = 0.05 * rng.standard_normal(d * K)
    return A.to(dtype), Y, x0


def multi_problem(A, Y, x0, N, **kw):
    K = Y.shape[1]
    c = 1.0 / N
    return scsopt.Problem(A, Y, x0, losses.softmax_ce(K, c), 1e-3, out_fn=losses.linear_softmax_ce(K, c),
                          multi_batches=True, multi_sample=True, **kw)


def timing(p):
    t = p.ctx.timing()
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    return t


def select_ms(p, b):
    t0 = time.perf_counter()
    p.select_batch(b)
    return 1e3 * (time.perf_counter() - t0)


def stepper(p, m):
    x_new, pri = np.empty(m), C.c_double()

    def one_step(x, x_prev, it=1):
        p.ctx.check(_lib.lib.scs_step(p.ctx.h, _lib.dptr(x), _lib.dptr(x_prev), it, _lib.dptr(x_new), None,
                                      C.byref(pri)))
        return x_new.copy()
    return one_step


def gather_round(p, pair, reps, arm):
    """reps gathers alternating between the two equal-sized batches of `pair` (each call re-gathers)."""
    if arm is not None:
        os.environ["SCS_MULTI_GATHER"] = arm
    p.set_batches(pair)
    os.environ.pop("SCS_MULTI_GATHER", None)
    select_ms(p, 0), select_ms(p, 1)                       # warm-up: the pool view, both row lists
    ts = [select_ms(p, i & 1) for i in range(reps)]
    p.select_batch(-1)
    p.set_batches(None)
    return ts


def gather_section(A, Y, x0, N, d, nb, rounds, reps, f32):
    elem = 4 if f32 else 8
    perm = np.random.default_rng(3).permutation(N)
    pair = [perm[:nb], perm[nb:2 * nb]]
    pm = multi_problem(A, Y, x0, N, dense_f32=f32)
    ps = scsopt.Problem(A, Y[:, 0].copy(), x0[:d], losses.least_squares(1.0 / N), 1e-3, dense_f32=f32)
    assert pm.data_info()[0] == elem and ps.data_info()[0] == elem
    nbytes = 2.0 * nb * d * elem
    print(f"--- gather: N = {N}, d = {d}, K = {Y.shape[1]}, {'fp32' if f32 else 'fp64'} storage, n_b = {nb}: "
          f"{nbytes / 2**20:.0f} MiB by count (read + write); {rounds} rounds of {reps} calls per arm", flush=True)
    arms = {"ref": [], "new": [], "single": []}
    for _ in range(rounds):
        arms["ref"].append(gather_round(pm, pair, reps, "0"))
        arms["new"].append(gather_round(pm, pair, reps, "1"))
        arms["single"].append(gather_round(ps, pair, reps, None))
    out = {"f32": f32, "n_b": nb, "bytes": nbytes}
    names = {"new": "multi_gather_rows_kernel (one launch)", "ref": "gather_rows_kernel + K - 1 gather_y launches",
             "single": "single-output context (gather_rows_kernel)"}
    for k in ("new", "ref", "single"):
        meds = [float(np.median(r)) for r in arms[k]]
        allt = np.concatenate(arms[k])
        med = float(np.median(allt))
        out[k] = line(names[k], allt, f"  {nbytes / med / 1e9:.3f} TB/s by count; round medians "
                      + " ".join(f"{m:.3f}" for m in meds))
        out[k + "_round_medians"] = meds
    sp = out["ref_round_medians"]
    out["ref_spread"] = (max(sp) - min(sp)) / float(np.median(sp))
    print(f"  run-to-run spread of the reference arm's round medians: {100 * out['ref_spread']:.1f} %; new / ref = "
          f"{out['new'][0] / out['ref'][0]:.3f}", flush=True)
    ps.ctx.close()
    return pm, out


def lqn_section(p, A, Y, x0, N, d, K, nb, f32):
    perm = np.random.default_rng(3).permutation(N)
    batches = [perm[i * nb:(i + 1) * nb] for i in range(N // nb)]
    p.set_batches(batches)
    p.configure("l1", HM())
    meth = scsopt.ProxLQNSCORE(m=5)
    init_method(meth, p)
    one_step = stepper(p, d * K)
    x_prev, x = x0.copy(), x0.copy()
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
    rec = {"gather": [], "step": [], "gemv": []}
    for epoch in (1, 2):                                     # epoch 1 warms up (views, the L-BFGS memory)
        for b in range(len(batches)):
            tg = select_ms(p, b)
            timing(p)
            xn = one_step(x, x_prev, epoch)
            t = timing(p)
            x_prev, x = x, xn
            if epoch == 2:
                rec["gather"].append(tg)
                rec["step"].append(t["step_ms"])
                rec["gemv"].append(t["gemv_ms"])
                calls = t["gemv_calls"]
    p.select_batch(-1)
    p.set_batches(None)
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 0))
    print(f"--- steady ProxLQNSCORE epoch (the second): {len(batches)} batches of {nb}, "
          f"{'fp32' if f32 else 'fp64'} storage, per batch", flush=True)
    out = {"f32": f32, "batches": len(batches)}
    out["gather"] = line("gather (scs_select_batch, host clock)", rec["gather"])
    out["step"] = line("step (T_STEP)", rec["step"])
    out["gemv"] = line(f"its products (T_GEMV, {calls} calls)", rec["gemv"])
    # the two products apart, on a context holding one batch's rows
    idx = torch.from_numpy(np.sort(batches[0])).cuda()
    pb = multi_problem(A[idx].contiguous(), Y[np.sort(batches[0])], x0, N, dense_f32=f32)
    pb.ctx.check(_lib.lib.scs_timing_enable(pb.ctx.h, 1))
    ax, both = [], []
    rng = np.random.default_rng(9)
    for i in range(6):
        xa, xb = x0 + 1e-3 * rng.standard_normal(d * K), x0 + 1e-3 * rng.standard_normal(d * K)
        timing(pb)
        pb.fx(xa)
        t1 = timing(pb)
        pb.gradx(xb)
        t2 = timing(pb)
        if i:
            ax.append(t1["gemv_ms"])
            both.append(t2["gemv_ms"])
    elem = 4 if f32 else 8
    gb = nb * d * elem / 1e9
    out["ax"] = line("A X alone (scs_eval_f on the batch's rows)", ax, f"  {gb / np.median(ax):.2f} TB/s of A")
    out["ax_atr"] = line("A X + A' R (scs_eval_grad)", both)
    out["atr"] = float(np.median(both) - np.median(ax))
    print(f"  A' R by difference: {out['atr']:.3f} ms = {gb / out['atr']:.2f} TB/s of A", flush=True)
    pb.ctx.close()
    return out


def ggn_section(p, x0, N, d, K, sizes, f32):
    perm = np.random.default_rng(3).permutation(N)
    p.configure("l1", HM())
    init_method(scsopt.ProxGGNSCORE(), p)
    one_step = stepper(p, d * K)
    out = []
    for nb in sizes:
        p.set_batches([perm[:nb], perm[nb:2 * nb]])
        branch = "sample-space" if nb * K + 1 <= d * K else "feature"
        select_ms(p, 0)
        one_step(x0, x0)                                     # warm-up
        p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
        rec = {k: [] for k in ("gather", "step", "gram", "solve", "gemv")}
        for i in range(3):
            rec["gather"].append(select_ms(p, (i + 1) & 1))
            timing(p)
            one_step(x0, x0)
            t = timing(p)
            for k in ("step", "gram", "solve", "gemv"):
                rec[k].append(t[k + "_ms"])
        p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 0))
        order = nb * K + 1 if branch == "sample-space" else d * K
        print(f"--- one ProxGGNSCORE step on a batch of {nb} ({branch} branch, system order {order}), "
              f"{'fp32' if f32 else 'fp64'} storage: {t['gram_calls']} Grams", flush=True)
        o = {"n_b": nb, "branch": branch, "order": order, "f32": f32, "grams": t["gram_calls"]}
        for k, tag in (("gather", "gather (host clock)"), ("step", "whole step (T_STEP)"), ("gram", "Grams (T_GRAM)"),
                       ("solve", "factor + solve (T_SOLVE)"), ("gemv", "products (T_GEMV)")):
            o[k] = line(tag, rec[k])
        out.append(o)
        p.select_batch(-1)
        p.set_batches(None)
    return out


def callback_section(N, d, K, nb):
    A, Y, x0 = data(N, d, K, 13)
    Ah = A.cpu().numpy()
    c = 1.0 / N
    perm = np.random.default_rng(3).permutation(N)
    batches = [perm[i * nb:(i + 1) * nb] for i in range(N // nb)]
    print(f"--- one ProxGGNSCORE epoch, N = {N}, d = {d}, K = {K}, {len(batches)} batches of {nb} (Jacobian "
          f"{nb * K * d * K * 8 / 2**20:.0f} MiB per step on the callback route): wall time", flush=True)
    out = {"N": N, "d": d, "K": K, "n_b": nb}
    meth = scsopt.ProxGGNSCORE()
    # the device path
    p = multi_problem(A, Y, x0, N)
    p.configure("l1", HM())
    init_method(meth, p)
    p.set_batches(batches)
    one = stepper(p, d * K)
    xs = {}
    for arm in ("device", "callback"):
        if arm == "callback":
            probs = []
            for r in batches:
                q = scsopt.Problem(Ah[r], Y[r], x0, softmax_closures(d, K, c), 1e-3)
                q.configure("l1", HM())
                init_method(meth, q)
                probs.append((q, stepper(q, d * K)))
        ws = []
        for rnd in range(3):                                 # the first epoch warms up
            x = x0.copy()
            t0 = time.perf_counter()
            for b in range(len(batches)):
                if arm == "device":
                    p.select_batch(b)
                    x = one(x, x)
                else:
                    x = probs[b][1](x, x)
            if rnd:
                ws.append(1e3 * (time.perf_counter() - t0))
        xs[arm] = x
        out[arm] = line(f"{arm} route, one epoch (wall)", ws)
    err = float(np.max(np.abs(xs["device"] - xs["callback"])) / max(1.0, float(np.max(np.abs(xs["callback"])))))
    print(f"  x after the epoch differs by {err:.2e} (max, relative to max |x|); callback / device = "
          f"{out['callback'][0] / out['device'][0]:.1f} x", flush=True)
    out["x_diff"] = err
    p.ctx.close()
    for q, _ in probs:
        q.ctx.close()
    return out


def shape_of(s):
    return tuple(int(v) for v in s.lower().split("x"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", default="1048576x2048x8")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--sample-batch", type=int, default=1024)
    ap.add_argument("--callback", default="4096x512x4")
    ap.add_argument("--callback-batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_batches_time.py measures on a GPU: none found")
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "storage": []}
    N, d, K = shape_of(args.shape)
    for f32 in (False, True):
        A, Y, x0 = data(N, d, K, 12, torch.float32 if f32 else torch.float64)
        p, g = gather_section(A, Y, x0, N, d, args.batch, args.rounds, args.reps, f32)
        o = {"f32": f32, "gather": g}
        o["lqn"] = lqn_section(p, A, Y, x0, N, d, K, args.batch, f32)
        if not f32:
            o["ggn"] = ggn_section(p, x0, N, d, K, (args.batch, args.sample_batch), f32)
        p.ctx.close()
        del A
        torch.cuda.empty_cache()
        res["storage"].append(o)
        if args.out:                                         # what is done so far survives a later failure
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
    if args.callback:
        res["callback"] = callback_section(*shape_of(args.callback), args.callback_batch)
    out = json.dumps(res)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
