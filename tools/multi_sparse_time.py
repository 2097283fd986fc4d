"""Time the multi-output products of a sparse A and one multi-output ProxGGNSCORE step on one MI355X
(DESIGN §2i).

    python tools/multi_sparse_time.py [--N 1048576] [--d 65536] [--nnz-row 655] [--K 2,4,8,16] [--rounds 7]
                                      [--step-N 131072] [--step-d 1024] [--step-K 8] [--step-nnz-row 51]
                                      [--skip-step] [--skip-products] [--storage fp64,fp32]

Products, per storage type and K: A X and Aᵀ V of csrc/multi_sparse.hip (the nonzeros read once for all
K columns) against K launches of the single-vector product (spmv_blk_kernel) on a context without
outputs, and against one such launch, the floor of one pass over the nonzeros.  The CSR is generated on
the device (torch: --nnz-row uniformly drawn columns per row, duplicates kept, standard normal values
scaled by 1/√nnz-row) and handed through the device door to both contexts.  Times are the library's
device events (T_GEMV) around the product launches alone -- the repack of X / V and the finalize
included, the loss epilogue and every host copy excluded: f(x) at a fresh x times A X (or A x), ∇f at the
same x then times Aᵀ R (z is cached).  After a warm-up the arms alternate over --rounds rounds; median and
range are printed.  Condition checked and printed: for K in {8, 16} the whole range of the new product
lies below the whole range of K single products.  Beside it: padded nnz / nnz and the bytes of ptr of
the finer blocked copies (scs_data_info's context bytes before / after are printed too).

The step: ProxGGNSCORE on losses.softmax_ce at (--step-N, --step-d, --step-K), event timers on: its Gram
part beside K (K + 1) / 2 times one weighted sparse Gram on a context without outputs, and its solve.
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
    t = p.ctx.timing()
    p.ctx.check(_lib.lib.scs_timing_reset(p.ctx.h))
    return t["gemv_ms"], t["gemv_calls"]


def product_round(p, xs):
    """For each x of xs: f(x) (A X fresh) then ∇f(x) (Aᵀ R, z cached): (ms of A X, ms of Aᵀ), summed."""
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
    print(f"  {tag:44s} {np.median(ts):9.3f} ms ({ts.min():9.3f} .. {ts.max():9.3f})", flush=True)
    return [float(np.median(ts)), float(ts.min()), float(ts.max())]


def device_csr(N, d, k, f32, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cols = torch.randint(0, d, (N * k,), dtype=torch.int32, device="cuda", generator=g)
    vals = torch.randn((N * k,), dtype=torch.float32 if f32 else torch.float64, device="cuda", generator=g)
    vals /= np.sqrt(k)
    rowptr = torch.arange(0, N + 1, dtype=torch.int64, device="cuda") * k
    return torch.sparse_csr_tensor(rowptr, cols, vals, size=(N, d))


def padded_ratio(A, N, d, K, f32):
    """(padded nnz / nnz of the blocked CSR, of the blocked CSC, ptr bytes of both) for the layout cut
    for K columns (K = 1: the single-vector layout), restated from multi_spmm_shift / build_blocked:
    blocks of min(2^ceil(log2 ncols), 16384 / KP) indices, segments padded to slots of 4 (fp64) / 8 (fp32)."""
    kp = 1 if K == 1 else 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16
    slot = 8 if f32 else 4
    rows = torch.repeat_interleave(torch.arange(N, device="cuda"), A.crow_indices().diff())
    cols = A.col_indices().to(torch.int64)
    out, ptr_bytes = [], 0
    for r, c, nr, nc in ((rows, cols, N, d), (cols, rows, d, N)):
        shift = min(int(np.ceil(np.log2(max(nc, 1)))), 14 - int(np.log2(kp)))
        nsub = -(-nc // (1 << shift))
        cnt = torch.bincount(r * nsub + (c >> shift), minlength=nr * nsub)
        out.append(float(((cnt + slot - 1) // slot * slot).sum()) / max(int(cols.numel()), 1))
        ptr_bytes += 8 * (nr * nsub + 1)
        del cnt
    return out[0], out[1], ptr_bytes


def products(N, d, k, Ks, rounds, f32, res):
    tag = "fp32" if f32 else "fp64"
    A = device_csr(N, d, k, f32, 11)
    nnz = N * k
    rng = np.random.default_rng(2)
    p1 = scsopt.Problem(A, rng.standard_normal(N), np.zeros(d), losses.least_squares(1.0 / N), 1e-3, sparse_f32=f32)
    timers(p1)
    b1 = p1.data_info()[2]
    vb = 4 if f32 else 8
    print(f"--- products, {tag} storage: N = {N}, d = {d}, {k} nonzeros per row (nnz = {nnz}, "
          f"{nnz * (vb + 2) / 2**30:.2f} GiB of (value, index) per pass); single-vector context holds "
          f"{b1 / 2**30:.2f} GiB", flush=True)
    for K in Ks:
        Y = np.eye(K)[rng.integers(0, K, size=N)]
        pk = scsopt.Problem(A, Y, np.zeros(d * K), losses.softmax_ce(K, 1.0 / N), 1e-3, sparse_f32=f32,
                            sparse_outputs=True)
        timers(pk)
        bk = pk.data_info()[2]
        fresh = lambda n: [0.1 * rng.standard_normal(n) for _ in range(1)]     # noqa: E731
        singles = lambda: [0.1 * rng.standard_normal(d) for _ in range(K)]     # noqa: E731
        product_round(pk, fresh(d * K))                      # warm-up of both arms
        product_round(p1, singles()[:2])
        kname = pk.ctx.kernel_names()[1]
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
        print(f"K = {K} ({tag}), {kname}; context holds {bk / 2**30:.2f} GiB; median (min .. max) over {rounds} "
              f"alternated rounds")
        pr, pc, pb = padded_ratio(A, N, d, K, f32)
        pr1, pc1, pb1 = padded_ratio(A, N, d, 1, f32)
        print(f"  padded nnz / nnz: CSR {pr:.3f}, CSC {pc:.3f} (single-vector layout {pr1:.3f}, {pc1:.3f}); ptr of both "
              f"copies {pb / 2**30:.3f} GiB (single-vector layout {pb1 / 2**30:.3f} GiB)")
        out = {"kernel": kname, "ctx_bytes": bk, "single_ctx_bytes": b1, "padded_csr": pr, "padded_csc": pc,
               "padded_csr_single": pr1, "padded_csc_single": pc1, "ptr_bytes": pb, "ptr_bytes_single": pb1}
        out["ax_multi"] = rng_line("A X, one pass for K columns", m_ax)
        out["ax_k_single"] = rng_line(f"A x, {K} single launches", s_ax)
        out["ax_one"] = rng_line("A x, one launch (floor)", o_ax)
        out["atv_multi"] = rng_line("A' V, one pass for K columns", m_at)
        out["atv_k_single"] = rng_line(f"A' v, {K} single launches", s_at)
        out["atv_one"] = rng_line("A' v, one launch (floor)", o_at)
        for nm in ("ax", "atv"):
            mu, ks, one = out[nm + "_multi"], out[nm + "_k_single"], out[nm + "_one"]
            below = mu[2] < ks[1]
            out[nm + "_below"] = bool(below)
            print(f"  {nm}: {ks[0] / mu[0]:.2f} x faster than {K} single launches, {mu[0] / one[0]:.2f} x the floor; "
                  f"ranges {'do not overlap (new below)' if below else 'OVERLAP or new above'}"
                  + ("" if K < 8 else f" -- condition {'met' if below else 'NOT met'}"), flush=True)
        res["products"][f"{tag}_K{K}"] = out
        pk.ctx.close()
    p1.ctx.close()
    del A
    torch.cuda.empty_cache()


def step(N, d, K, k, rounds, res):
    A = device_csr(N, d, k, False, 12)
    rng = np.random.default_rng(3)
    Y = np.eye(K)[rng.integers(0, K, size=N)]
    x0 = 0.05 * rng.standard_normal(d * K)
    p = scsopt.Problem(A, Y, x0, losses.softmax_ce(K, 1.0 / N), 1e-3, out_fn=losses.linear_softmax_ce(K, 1.0 / N),
                       sparse_outputs=True)
    p.configure("l1", scsopt.PHuberSmootherL1L2(0.5))
    init_method(scsopt.ProxGGNSCORE(), p)
    x_new, pri = np.empty_like(x0), C.c_double()

    def one_step():
        p.ctx.check(_lib.lib.scs_step(p.ctx.h, _lib.dptr(x0), _lib.dptr(x0), 1, _lib.dptr(x_new), None, C.byref(pri)))
    one_step()                                               # warm-up (allocates the system, builds the Gram's copies)
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
    print(f"--- ProxGGNSCORE softmax step on a sparse A: N = {N}, d = {d}, K = {K}, {k} nonzeros per row (system order "
          f"{d * K}, {npair} Grams), fp64; {rounds} rounds; Gram kernel {p.ctx.kernel_names()[0]} "
          f"(without outputs: {p1.ctx.kernel_names()[0]})")
    out = {"npair": npair, "gram_kernel": p.ctx.kernel_names()[0]}
    out["step"] = rng_line("whole step (T_STEP)", ts)
    out["gram_part"] = rng_line("its Gram part (weights, Grams, placement)", gs)
    out["solve"] = rng_line("its solve (order d K)", ss)
    out["one_gram"] = rng_line("one (N, d) weighted sparse Gram, no outputs", g1)
    print(f"  {npair} x one Gram = {npair * out['one_gram'][0]:.3f} ms; the Gram part is "
          f"{out['gram_part'][0] / (npair * out['one_gram'][0]):.3f} x that")
    res["step"] = out
    p.ctx.close()
    p1.ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--N", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=1 << 16)
    ap.add_argument("--nnz-row", type=int, default=655)
    ap.add_argument("--K", default="2,4,8,16")
    ap.add_argument("--storage", default="fp64,fp32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-N", type=int, default=1 << 17)
    ap.add_argument("--step-d", type=int, default=1024)
    ap.add_argument("--step-K", type=int, default=8)
    ap.add_argument("--step-nnz-row", type=int, default=51)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    args = ap.parse_args()
    Ks = [int(k) for k in args.K.split(",") if k]
    res = {"N": args.N, "d": args.d, "nnz_row": args.nnz_row, "K": Ks, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "arm_env": os.environ.get("SCS_MULTI_SPARSE_KERNEL"),
           "products": {}}
    if not args.skip_products:
        for st in args.storage.split(","):
            products(args.N, args.d, args.nnz_row, Ks, args.rounds, st == "fp32", res)
    if not args.skip_step:
        step(args.step_N, args.step_d, args.step_K, args.step_nnz_row, args.rounds, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
