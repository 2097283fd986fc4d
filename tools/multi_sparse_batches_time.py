"""Time minibatches of a multi-output loss on a sparse A on one MI355X.

    python tools/multi_sparse_batches_time.py [--N 1048576] [--d 65536] [--nnz-row 655] [--K 8,16]
                                              [--storage fp64,fp32] [--batch 16384] [--rounds 5] [--reps 6]
                                              [--epoch-batches 64] [--skip-dense] [--skip-epochs] [--out FILE.json]

losses.softmax_ce at scale 1/N on Problem(..., sparse_outputs=True, multi_batches=True,
multi_sparse_batches=True, sparse_batches=True): the CSR is generated on the device (tools/multi_sparse_time.py's
generator: --nnz-row uniformly drawn columns per row, duplicates kept) and handed over through the device door;
--epoch-batches shuffled batches of --batch rows.

  forms     per round and per workgroup form of the one-pass kernel on views (SCS_MULTI_SPARSE_NARROW=0: 1024
            rows per workgroup, =1: 256; read where the list is registered, so each round registers the list
            again and builds its views again): the build of a sparse view (scs_select_batch on a batch without
            one, host clock, synchronised), scs_select_batch on a held view, and --reps ProxLQNSCORE steps on
            that view by the library's event timers (T_STEP; T_GEMV = its products A_b X and A_bᵀ R).  Rounds
            alternate 1024, 256, 1024, ...; median (min .. max) over all timed calls of a form, and the rule of
            DESIGN §2i / §2k evaluated: the 256-row form is the default for a (KP, storage) only where its whole
            range lies below the whole range of the 1024-row form.
  dense     the same step on the densified view of the same batch (sparse_batches off: n_b x d_pad doubles),
            with its build (memset + launch_densify_rows + the Y gather).
  epochs    the first epoch (every view built) and a steady one (views kept within the budget, or rebuilt)
            through scs_select_batch + scs_step, wall time; views held, their device bytes, builds.

Every figure is a first measurement of this path.  The last line is one JSON object with all of them."""
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
from multi_sparse_time import device_csr  # noqa: E402

HM = lambda: scsopt.PHuberSmootherL1L2(0.5)   # noqa: E731
FORM = "SCS_MULTI_SPARSE_NARROW"


def line(tag, ts, extra=""):
    ts = np.asarray(ts, dtype=np.float64)
    print(f"  {tag:58s} {np.median(ts):10.3f} ms ({ts.min():10.3f} .. {ts.max():10.3f}){extra}", flush=True)
    return [float(np.median(ts)), float(ts.min()), float(ts.max())]


def timing(p):
    t = p.ctx.timing()
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    return t


def select_ms(p, b):
    t0 = time.perf_counter()
    p.select_batch(b)                      # scs_select_batch synchronises before it returns
    return 1e3 * (time.perf_counter() - t0)


def stepper(p, m):
    x_new, pri = np.empty(m), C.c_double()

    def one_step(x, x_prev, it=1):
        p.ctx.check(_lib.lib.scs_step(p.ctx.h, _lib.dptr(x), _lib.dptr(x_prev), it, _lib.dptr(x_new), None,
                                      C.byref(pri)))
        return x_new.copy()
    return one_step


def register(p, batches, form):
    if form is None:
        os.environ.pop(FORM, None)
    else:
        os.environ[FORM] = form
    p.set_batches(batches)
    os.environ.pop(FORM, None)


def view_round(p, pair, x0, one_step, reps, form):
    """Register `pair` with `form`, build both views, then reps timed steps on view 0."""
    register(p, pair, form)
    builds = [select_ms(p, 0), select_ms(p, 1)]
    held = [select_ms(p, i & 1) for i in range(4)]
    p.select_batch(0)
    one_step(x0, x0)                                         # warm-up
    name = p.ctx.kernel_names()[1]
    timing(p)
    steps, gemvs = [], []
    for _ in range(reps):
        one_step(x0, x0)
        t = timing(p)
        steps.append(t["step_ms"])
        gemvs.append(t["gemv_ms"])
    info = p.batch_info()
    p.select_batch(-1)
    p.set_batches(None)
    return dict(build=builds, held=held, step=steps, gemv=gemvs, name=name, info=info, calls=t["gemv_calls"])


def section(A, N, d, K, nb, nbatch, rounds, reps, f32, skip_dense, skip_epochs):
    tag = "fp32" if f32 else "fp64"
    rng = np.random.default_rng(4)
    Y = np.eye(K)[rng.integers(0, K, size=N)]
    x0 = 0.05 * rng.standard_normal(d * K)
    c = 1.0 / N
    p = scsopt.Problem(A, Y, x0, losses.softmax_ce(K, c), 1e-3, out_fn=losses.linear_softmax_ce(K, c), sparse_f32=f32,
                       sparse_outputs=True, multi_batches=True, multi_sparse_batches=True, sparse_batches=True)
    p.configure("l1", HM())
    init_method(scsopt.ProxLQNSCORE(m=5), p)
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
    one_step = stepper(p, d * K)
    perm = np.random.default_rng(3).permutation(N)
    batches = [perm[i * nb:(i + 1) * nb] for i in range(min(nbatch, N // nb))]
    pair = batches[:2]
    print(f"--- K = {K}, {tag} values: N = {N}, d = {d}, batches of {nb}; the context holds "
          f"{p.data_info()[2] / 2**30:.2f} GiB; {rounds} alternated rounds of {reps} steps per form", flush=True)
    out = {"K": K, "f32": f32, "n_b": nb}
    view_round(p, pair, x0, one_step, 1, "0")                # warm-up of both forms (scratch, the L-BFGS buffers)
    view_round(p, pair, x0, one_step, 1, "1")
    rec = {"0": [], "1": []}
    for _ in range(rounds):
        for form in ("0", "1"):
            rec[form].append(view_round(p, pair, x0, one_step, reps, form))
    names = {"0": "1024 rows per workgroup", "1": "256 rows per workgroup"}
    for form in ("0", "1"):
        rs = rec[form]
        print(f"  {names[form]}: {rs[0]['name']}; view bytes {rs[0]['info'][1] / 2 / 2**20:.1f} MiB per batch", flush=True)
        o = {"kernel": rs[0]["name"], "view_bytes_per_batch": rs[0]["info"][1] / 2}
        o["build"] = line("view build per batch (scs_select_batch, host clock)", np.concatenate([r["build"] for r in rs]))
        o["held"] = line("scs_select_batch on a held view", np.concatenate([r["held"] for r in rs]))
        o["step"] = line("ProxLQNSCORE step on the sparse view (T_STEP)", np.concatenate([r["step"] for r in rs]))
        o["gemv"] = line(f"its products (T_GEMV, {rs[0]['calls']} calls)", np.concatenate([r["gemv"] for r in rs]),
                         "  round medians " + " ".join(f"{np.median(r['gemv']):.3f}" for r in rs))
        out["form" + form] = o
    w, n = out["form0"]["gemv"], out["form1"]["gemv"]
    out["narrow_below"] = bool(n[2] < w[1])
    print(f"  products, 256 / 1024: {n[0] / w[0]:.3f}; the 256-row form's whole range "
          f"{'lies below' if out['narrow_below'] else 'does NOT lie below'} the 1024-row form's", flush=True)
    if not skip_dense:
        p.set_sparse_batches(False)
        r = view_round(p, pair, x0, one_step, reps, None)
        o = {"view_bytes": r["info"][1], "views": r["info"][0]}     # one pool view serves both batches of the pair
        print(f"  densified view: {r['info'][1] / 2**30:.2f} GiB ({r['info'][0]} pool view for the batch size)", flush=True)
        o["build"] = line("view fill per batch (first: with its allocation)", r["build"])
        o["refill"] = line("scs_select_batch, the other batch (refill)", r["held"])
        o["step"] = line("ProxLQNSCORE step on the densified view (T_STEP)", r["step"])
        o["gemv"] = line(f"its products (T_GEMV, {r['calls']} calls)", r["gemv"])
        out["dense"] = o
        p.set_sparse_batches(True)
    if not skip_epochs:
        register(p, batches, None)
        x_prev, x = x0.copy(), x0.copy()
        walls = []
        for epoch in (1, 2, 3):
            t0 = time.perf_counter()
            for b in range(len(batches)):
                p.select_batch(b)
                xn = one_step(x, x_prev, epoch)
                x_prev, x = x, xn
            walls.append(1e3 * (time.perf_counter() - t0))
        nv, vb, bd = p.batch_info()
        out["epochs"] = {"batches": len(batches), "first_ms": walls[0], "steady_ms": walls[1:], "views": nv,
                         "view_bytes": vb, "builds": bd}
        print(f"  epochs of {len(batches)} batches (default form), wall: first {walls[0]:.1f} ms, then "
              + ", ".join(f"{w_:.1f}" for w_ in walls[1:]) + f" ms; {nv} views held, {vb / 2**30:.2f} GiB, {bd} builds",
              flush=True)
        p.select_batch(-1)
        p.set_batches(None)
    p.ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--N", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=1 << 16)
    ap.add_argument("--nnz-row", type=int, default=655)
    ap.add_argument("--K", default="8,16")
    ap.add_argument("--storage", default="fp64,fp32")
    ap.add_argument("--batch", type=int, default=1 << 14)
    ap.add_argument("--epoch-batches", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--skip-epochs", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_sparse_batches_time.py measures on a GPU: none found")
    res = {"device": torch.cuda.get_device_name(0), "N": args.N, "d": args.d, "nnz_row": args.nnz_row,
           "rounds": args.rounds, "reps": args.reps, "sections": []}
    for st in args.storage.split(","):
        f32 = st == "fp32"
        A = device_csr(args.N, args.d, args.nnz_row, f32, 11)
        for K in [int(k) for k in args.K.split(",") if k]:
            res["sections"].append(section(A, args.N, args.d, K, args.batch, args.epoch_batches, args.rounds,
                                           args.reps, f32, args.skip_dense, args.skip_epochs))
            if args.out:                                     # what is done so far survives a later failure
                with open(args.out, "w") as fh:
                    fh.write(json.dumps(res) + "\n")
        del A
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
