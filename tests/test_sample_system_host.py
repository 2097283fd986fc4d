"""CPU: the reference side of tests/test_gpu_sample_system.py, without a GPU.

The NumPy restatement of the single-output sample-space system (tests/sample_system_data.py) gives the
oracle's direction and satisfies the m-space identity it is derived from; every hard case meets the
preconditions the GPU file relies on; the error bounds are not vacuous (a small wrong system leaves
them); the new entry point is declared and bound."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import sample_system_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import scsopt_oracle as O  # noqa: E402

HDR = os.path.join(ROOT, "include", "scsopt.h")
PKG = os.path.join(ROOT, "selfconcordantsmoothoptimization.jl_amd", "scsopt")
CASES = [(k, N, m, hard) for k in D.KINDS for (N, m) in D.SHAPES for hard in (False, True)]
HARD = [(k, N, m) for k in D.KINDS for (N, m) in D.SHAPES]


def _oracle_loss(cs):
    if cs.kind == "logistic":
        return O.Loss("logistic_ce", cs.c, ggn="sigmoid_ce")
    return O.Loss("least_squares", cs.c, ggn="linear_ls")


@pytest.mark.parametrize("kind,N,m,hard", CASES)
def test_restatement_is_the_oracles_step(kind, N, m, hard):
    """s, r, q are the oracle's bits; the direction -h ∘ (Aᵀ(s ∘ B) + λ gr B_N) from M B = b is
    O.ggn_score_step's, and satisfies (diag(Hr) + Jt Q̃ Jtᵀ) d = -Jt [r; 1] (Jt = [Jᵀ λgr], Q̃ = diag(q, 0)),
    the m-space system the sample-space one is the Woodbury form of.  Both to 1e-13·cond(M), the bound the
    GPU file applies to the device's direction (the two solves differ by O(cond·ε))."""
    cs = D.case(kind, N, m, hard)
    hm = O.PHuberSmootherL1L2(cs.mu)
    gr, Hr = hm.grad(None, cs.x0), hm.hess(None, cs.x0)
    g2, H2 = D.huber(cs.x0, cs.mu)
    assert np.array_equal(gr, g2) and np.array_equal(Hr, H2)
    s, r, q = _oracle_loss(cs).ggn_parts(cs.A, cs.y, cs.x0)
    s2, r2, q2, _ = D.parts(kind, cs.A, cs.y, cs.x0, cs.c)
    assert np.array_equal(s, s2) and np.array_equal(r, r2) and np.array_equal(q, q2)
    lgr = cs.lam * gr
    M, b = D.system(cs.A, s, r, q, lgr, Hr)
    e_n = np.zeros(N + 1)
    e_n[N] = 1.0
    assert np.array_equal(M[N], e_n) and b[N] == 1.0
    cond = float(np.linalg.cond(M))
    B = np.linalg.solve(M, b)
    d = D.direction(cs.A, s, lgr, Hr, B)
    d_o = O.ggn_score_step(cs.A, s, r, q, lgr, Hr, cs.lam)
    scale = float(np.max(np.abs(d_o)))
    err = float(np.max(np.abs(d - d_o))) / scale
    Jt = np.hstack([(s[:, None] * cs.A).T, lgr[:, None]])
    Qt = np.concatenate([q, [0.0]])
    K = np.diag(Hr) + (Jt * Qt[None, :]) @ Jt.T
    rhs = -(Jt @ b)
    size = np.abs(K) @ np.abs(d) + np.abs(Jt) @ np.abs(b)
    res = float(np.max(np.abs(K @ d - rhs) / size))
    print(f"{kind} ({N}, {m}) hard={hard}: cond {cond:.3g}, |d - d_oracle| / max|d| = {err:.2e}, "
          f"m-space residual / (|K||d| + |Jt||b|) = {res:.2e}")
    assert err <= 1e-13 * cond
    assert res <= 1e-13 * cond


@pytest.mark.parametrize("kind,N,m", HARD)
def test_hard_preconditions(kind, N, m):
    """max |A x0| <= 8, 1e3 <= cond(M) <= 1e6 (N >= 127), a last-column entry >= 1, getrf interchanges rows
    (logistic, N >= 2) -- and the easy case of the same shape is the benign kind: cond < 3, no interchange."""
    f = D.hard_preconditions(D.case(kind, N, m, True))
    print(f"{kind} ({N}, {m}): " + ", ".join(f"{k} {v:.4g}" for k, v in f.items()))
    ce = D.case(kind, N, m, False)
    Me = ce.system_at(ce.x0)[0]
    assert np.linalg.cond(Me) < 3.0 and D.interchanges(Me) == 0


@pytest.mark.parametrize("route", ["dense", "dense_f32"])
@pytest.mark.parametrize("kind,N,m", HARD)
def test_bounds_are_not_vacuous(kind, N, m, route):
    """On every hard case a slightly wrong system leaves the bound: one entry of P off by 1e-9 relative;
    s_i² in place of s_i s_j in one off-diagonal entry (logistic: the linear out_fn has s = 1, where the
    two coincide); the last column dropped.  And the system itself lies within it (err 0)."""
    cs = D.case(kind, N, m, True)
    M, b, dM, db, s, lgr, Hr = cs.system_at(cs.x0, route)
    A = cs.stored(route)
    _, r, q, _ = D.parts(kind, A, cs.y, cs.x0, cs.c)
    assert np.all(np.isfinite(dM)) and np.all(np.isfinite(db)) and np.all(dM[:N] > 0)
    P = (A * (1.0 / Hr)[None, :]) @ A.T
    T = q[:, None] * (s[:, None] * s[None, :] * P)
    i = int(np.argmax(np.abs(np.diag(T))))
    wrong = M.copy()
    wrong[i, i] = 1.0 + T[i, i] * (1.0 + 1e-9)
    assert abs(wrong[i, i] - M[i, i]) > dM[i, i]
    wrong = M.copy()
    wrong[:N, N] = 0.0
    assert np.any(np.abs(wrong - M) > dM)
    if kind == "logistic" and N >= 2:
        off = np.abs(T - np.diag(np.diag(T)))
        i, j = np.unravel_index(int(np.argmax(off)), off.shape)
        bad = q[i] * (s[i] * s[i] * P[i, j])
        assert abs(bad - T[i, j]) > dM[i, j]


def test_bounds_stay_small():
    """The bounds are rounding-sized: relative to the largest entry of the system below 1e-9 on every case
    (1e-13 Σ|terms| and the conditioning of 1 - ŷ at |z| <= 8, about 3e3 ε)."""
    for kind, N, m, hard in CASES:
        cs = D.case(kind, N, m, hard)
        M, b, dM, db, _, _, _ = cs.system_at(cs.x0)
        assert dM.max() <= 1e-9 * np.abs(M).max() and db.max() <= 1e-9 * np.abs(b).max()


@pytest.mark.parametrize("N,m", D.SHAPES)
def test_exact_case_is_exact(N, m):
    """exact_case's expected system is the restatement's on the same integers, bit for bit, for mu = 0.5, 2."""
    for mu in (0.5, 2.0):
        A, y, M, b = D.exact_case(N, m, mu)
        x = np.zeros(m)
        gr, Hr = D.huber(x, mu)
        assert np.all(Hr == 1.0 / mu) and np.all(gr == 0.0)
        s, r, q, _ = D.parts("least_squares", A, y, x, 0.25)
        M2, b2 = D.system(A, s, r, q, 0.3 * gr, Hr)
        assert np.array_equal(M.view(np.int64), M2.view(np.int64))
        assert np.array_equal(b.view(np.int64), b2.view(np.int64))
        assert not np.any(np.signbit(M[:N, N]))


def test_entry_point_is_declared_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    mt = re.search(r"\bint\s+scs_sample_system_eval\s*\(([^)]*)\)\s*;", src)
    assert mt and [re.sub(r"\s*\w+$", "", a.strip()) for a in mt.group(1).split(",")] == \
        ["scs_ctx*", "const double*", "double*", "int64_t", "double*"]
    from scsopt import _lib
    fn = _lib.lib.scs_sample_system_eval
    assert "scs_sample_system_eval" in _lib.EXPORTED
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, _lib.c_dp, _lib.c_dp, C.c_int64, _lib.c_dp]
    assert "def sample_system(self, x)" in open(os.path.join(PKG, "problems.py")).read()
