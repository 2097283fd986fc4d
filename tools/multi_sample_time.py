"""Time a multi-output ProxGGNSCORE step in the sample-space shape on one MI355X.

    python tools/multi_sample_time.py [--shapes 2048x16384x8,1024x8192x16] [--callback 512x4096x4]
                                      [--rounds 5] [--out FILE.json]

Per shape N x d x K (N K + 1 <= d K), losses.softmax_ce at scale 1/N, Problem(..., multi_sample=True), A
generated on the device (torch.randn) and handed over through the device door:

  step      scs_step with the library's event timers on: the whole step (T_STEP), its K Grams
            A diag(h_l) Aᵀ (T_GRAM), the factor and solve of the order-(N K + 1) system (T_SOLVE), the
            products A X, A X̃, Aᵀ V (T_GEMV); "rest" is the step minus those three (the mirrors of P_l,
            the assembly, the epilogues, the step's tail and its host copies).
  assembly  scs_multi_sample_system_eval without output arrays: the door brackets its K assembly launches
            and the tail launch with events of their own (reported under the step timer, which no step
            is using there).  Bytes moved by count: each launch reads P_l once and writes K blocks,
            (K + K²) N² 8 B in all; the rate is set against the 6.3 TB/s copy figure of
            MI355X_MICROARCH.md.
  callback  the same step through losses.callback at --callback (where the dense (N K) x (d K) Jacobian
            still fits): wall time of scs_step, the host closures and the upload included, beside the
            device path's wall time on the same data.

After one warm-up call per arm (allocations, code loading) every figure is the median (min .. max) over
--rounds calls; the last line is one JSON object with all of them."""
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
from scsopt.iterate import init_method  # noqa: E402

COPY_TBS = 6.3


def rng_line(tag, ts, extra=""):
    ts = np.asarray(ts, dtype=np.float64)
    print(f"  {tag:46s} {np.median(ts):10.3f} ms ({ts.min():10.3f} .. {ts.max():10.3f}){extra}", flush=True)
    return [float(np.median(ts)), float(ts.min()), float(ts.max())]


def data(N, d, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn((N, d), dtype=torch.float64, device="cuda", generator=g) / np.sqrt(d)
    rng = np.random.default_rng(seed)
    Y = np.eye(K)[rng.integers(0, K, size=N)]
    x0 = 0.05 * rng.standard_normal(d * K)
    return A, Y, x0


def stepper(p, x0):
    x_new, pri = np.empty_like(x0), C.c_double()

    def one_step():
        p.ctx.check(_lib.lib.scs_step(p.ctx.h, _lib.dptr(x0), _lib.dptr(x0), 1, _lib.dptr(x_new), None, C.byref(pri)))
        return x_new
    return one_step


def timing(p):
    t = p.ctx.timing()
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    return t


def device_shape(N, d, K, rounds):
    assert N * K + 1 <= d * K, "not the sample-space shape"
    A, Y, x0 = data(N, d, K, 12)
    c = 1.0 / N
    p = scsopt.Problem(A, Y, x0, losses.softmax_ce(K, c), 1e-3, out_fn=losses.linear_softmax_ce(K, c),
                       multi_sample=True)
    p.configure("l1", scsopt.PHuberSmootherL1L2(0.5))
    init_method(scsopt.ProxGGNSCORE(), p)
    one_step = stepper(p, x0)
    one_step()                                               # warm-up
    p.ctx.check(_lib.lib.scs_timing_enable(p.ctx.h, 1))
    timing(p)
    n1 = N * K + 1
    print(f"--- N = {N}, d = {d}, K = {K}: system order {n1}, fp64, {rounds} rounds; device bytes held "
          f"{p.data_info()[2] / 2**30:.2f} GiB", flush=True)
    ts, gs, ss, vs, rs = [], [], [], [], []
    for _ in range(rounds):
        one_step()
        t = timing(p)
        assert t["gram_calls"] == K and t["solve_calls"] == 1, t
        ts.append(t["step_ms"])
        gs.append(t["gram_ms"])
        ss.append(t["solve_ms"])
        vs.append(t["gemv_ms"])
        rs.append(t["step_ms"] - t["gram_ms"] - t["solve_ms"] - t["gemv_ms"])
    out = {"N": N, "d": d, "K": K, "order": n1}
    out["step"] = rng_line("whole step (T_STEP)", ts)
    flop = 2.0 * K * N * N * d
    out["gram"] = rng_line(f"its {K} Grams A diag(h_l) A' (T_GRAM)", gs,
                           f"  {flop / np.median(gs) / 1e9:.1f} TF/s by 2 K N² d")
    out["solve"] = rng_line(f"factor + solve, order {n1} (T_SOLVE)", ss)
    out["products"] = rng_line("products A X, A X~, A' V (T_GEMV)", vs)
    out["rest"] = rng_line("rest (mirrors, assembly, tail, host copies)", rs)
    # the assembly launches alone, through the door
    door = lambda: p.ctx.check(_lib.lib.scs_multi_sample_system_eval(p.ctx.h, _lib.dptr(x0), None, 0, None))  # noqa: E731
    door()
    timing(p)
    asm = []
    for _ in range(rounds):
        door()
        t = timing(p)
        assert t["step_calls"] == K + 1, t
        asm.append(t["step_ms"])
    nbytes = (K + K * K) * N * N * 8.0
    med = float(np.median(asm))
    rate = nbytes / med / 1e9
    out["assembly"] = rng_line(f"assembly: {K} block launches + tail", asm,
                               f"  {nbytes / 2**30:.2f} GiB by count, {rate:.2f} TB/s = {100 * rate / COPY_TBS:.0f} % of "
                               f"{COPY_TBS} TB/s")
    out["assembly_bytes"] = nbytes
    out["assembly_tbs"] = [nbytes / a / 1e9 for a in (med, max(asm), min(asm))]   # median, slowest, fastest
    p.ctx.close()
    del A
    torch.cuda.empty_cache()
    return out


def softmax_closures(d, K, c):
    """The softmax cross-entropy as host closures for losses.callback (J = I_K ⊗ A, dense)."""
    def X_of(x):
        return np.asarray(x).reshape(d, K, order="F")

    def probs(Z):
        E = np.exp(Z - Z.max(axis=1, keepdims=True))
        return E / E.sum(axis=1, keepdims=True)

    def f(A, Y, x):
        S = A @ X_of(x)
        S = S - S.max(axis=1, keepdims=True)
        return -c * float(np.sum(Y * (S - np.log(np.exp(S).sum(axis=1, keepdims=True)))))

    def resid(Y, Z):
        return c * (Y.sum(axis=1, keepdims=True) * probs(Z) - Y)

    def hess_fy(A, Y, Z):
        N = Z.shape[0]
        P = probs(Z)
        s = Y.sum(axis=1)
        Q = c * s[:, None, None] * (P[:, :, None] * np.eye(K)[None] - P[:, :, None] * P[:, None, :])
        D = np.zeros((N * K, N * K))
        for k in range(K):
            for l in range(K):
                D[k * N + np.arange(N), l * N + np.arange(N)] = Q[:, k, l]
        return D

    return losses.callback(f, lambda A, Y, x: (A.T @ resid(Y, A @ X_of(x))).ravel(order="F"), None,
                           out_fn=lambda A, x: A @ X_of(x), jac_yx=lambda A, Y, Z, x: np.kron(np.eye(K), A),
                           grad_fy=lambda A, Y, Z: resid(Y, Z), hess_fy=hess_fy)


def callback_shape(N, d, K, rounds):
    A, Y, x0 = data(N, d, K, 13)
    Ah = A.cpu().numpy()
    c = 1.0 / N
    print(f"--- callback route beside the device path: N = {N}, d = {d}, K = {K} (Jacobian "
          f"{N * K * d * K * 8 / 2**30:.2f} GiB per step), wall time of scs_step, {rounds} rounds", flush=True)
    out = {"N": N, "d": d, "K": K}
    xs = {}
    for arm in ("device", "callback"):
        if arm == "device":
            p = scsopt.Problem(A, Y, x0, losses.softmax_ce(K, c), 1e-3, out_fn=losses.linear_softmax_ce(K, c),
                               multi_sample=True)
        else:
            p = scsopt.Problem(Ah, Y, x0, softmax_closures(d, K, c), 1e-3)
        p.configure("l1", scsopt.PHuberSmootherL1L2(0.5))
        init_method(scsopt.ProxGGNSCORE(), p)
        one_step = stepper(p, x0)
        xs[arm] = one_step().copy()                          # warm-up
        ws = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            one_step()
            ws.append(1e3 * (time.perf_counter() - t0))
        out[arm] = rng_line(f"{arm} route, one step (wall)", ws)
        p.ctx.close()
    err = float(np.max(np.abs(xs["device"] - xs["callback"])) / max(1.0, float(np.max(np.abs(xs["callback"])))))
    print(f"  the two routes' x after the step differ by {err:.2e} (max, relative to max |x|); callback / device = "
          f"{out['callback'][0] / out['device'][0]:.1f} x", flush=True)
    out["x_diff"] = err
    return out


def shape_of(s):
    N, d, K = (int(v) for v in s.lower().split("x"))
    return N, d, K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="2048x16384x8,1024x8192x16")
    ap.add_argument("--callback", default="512x4096x4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "copy_tbs": COPY_TBS, "shapes": []}
    for s in (v for v in args.shapes.split(",") if v):
        res["shapes"].append(device_shape(*shape_of(s), args.rounds))
    if args.callback:
        res["callback"] = callback_shape(*shape_of(args.callback), args.rounds)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
